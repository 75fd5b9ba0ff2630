#!/usr/bin/env python3
"""tools/pack_rates.py [OUT_PREFIX] -- what csic_pack_device and csic_unpack_device cost on one MI355X, and what they save.
Writes OUT_PREFIX.jsonl and OUT_PREFIX.md (default profiles/r12_pack_rates); the JSON lines also go to stdout.

Matrix: 8192 x 8192, 4:2:0 (order chroma, spatial, quant), factor 1 and 2, bits 8/8/8, 6/5/5 and 3/3/2; two contents --
  noise   : csic_synth_frame_device frames (residuals as wide as the codes: the coding cannot win, the payload is at its bound),
  natural : tests/golden/inputs/in512.png tiled 16 x 16 and rolled per frame.
Method: the frames are compressed on the device by the library itself into a ring of ROT PLANAR_BITS frames in separate buffers,
ROT chosen so that the ring exceeds 300 MiB (the Infinity Cache holds 256 MiB): no call finds its source cached.  Pack, unpack and
the two yardsticks -- csic_copy_device of the same payload (read once, written once) and csic_code_stats_device (k_cstat_bits: the
same source read once, the same lane-per-group mapping) -- take turns window by window after a warm-up round; a window is CALLS
calls back to back between two device events, the figure the median of REPS window means, with min and max.  A pack call is its
three passes (widths, scan, emit) through the C ABI, workspace and destinations allocated beforehand.  Before anything is timed
unpack(pack(x)) is compared with x on every frame of the ring.
Bytes: pack = 2 x source payload (read by the widths pass and again by the emit pass) + coded bytes written; unpack = coded bytes read
+ payload written; copy = 2 x payload; stats = payload.  Rates are those bytes over the time, also as a fraction of 8 TB/s."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import csic_amd as csic  # noqa: E402

N = csic._native
PREFIX = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r12_pack_rates")
CSQ = (3, 1, 2)
W = H = 8192
REPS, CALLS, WARM = 5, 8, 1
RING_BYTES = 300 << 20
PEAK = 8.0e12


def read_png(path):
    w, h = C.c_int32(), C.c_int32()
    N.check(N.lib().csic_png_info(path.encode(), C.byref(w), C.byref(h)))
    px = np.empty(w.value * h.value, dtype=np.uint32)
    N.check(N.lib().csic_png_read_argb(path.encode(), px.ctypes.data_as(C.c_void_p), px.size))
    return px.reshape(h.value, w.value)


def input_frame(content, k, tile):
    if content == "noise":
        d = torch.empty(W * H, dtype=torch.int32, device="cuda:0")
        N.check(N.lib().csic_synth_frame_device(C.c_void_p(d.data_ptr()), W * H, 0, 20251018 + k,
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return d
    return torch.roll(tile.repeat(H // tile.shape[0], W // tile.shape[1]), (37 * k, 11 * k), dims=(1, 0)).contiguous().reshape(-1)


def timed_alternating(fns, rot):
    times = {k: [] for k in fns}
    for rep in range(WARM + REPS):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(CALLS):
                fn((rep * CALLS + i) % rot)
            b.record()
            b.synchronize()
            if rep >= WARM:
                times[k].append(a.elapsed_time(b) * 1e3 / CALLS)
    return times


def cell(bits, f, content, tile):
    L = N.lib()
    rows = []
    with csic.Plan(csic.make_c_params(W, H, 2, 0, *bits, f, CSQ, out_format=N.FMT_PLANAR_BITS), 0) as pl:
        lay, pk = pl.planar_bits_layout, pl.pack_layout
        fb, bound, payload = lay.frame_bytes, pk.bound_bytes, lay.payload_bytes
        rot = max(5, -(-RING_BYTES // fb))
        src = [pl.process_device(input_frame(content, k, tile), torch.zeros(fb, dtype=torch.uint8, device="cuda:0")) for k in range(rot)]
        coded = [torch.empty(bound, dtype=torch.uint8, device="cuda:0") for _ in range(rot)]
        back = [torch.zeros(fb, dtype=torch.uint8, device="cuda:0") for _ in range(rot)]
        sizes = torch.zeros(rot, dtype=torch.int64, device="cuda:0")
        wsb = pl.pack_workspace_bytes(1)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
        hist = torch.empty((N.STATS_KINDS, N.STATS_PLANES, N.STATS_BINS), dtype=torch.int64, device="cuda:0")
        copy_px = payload // 16 * 4
        copy_dst = torch.empty(copy_px, dtype=torch.int32, device="cuda:0")
        stream = pl._stream()

        def pack(i):
            N.check(L.csic_pack_device(pl._h, C.c_void_p(src[i].data_ptr()), 1, C.c_void_p(coded[i].data_ptr()), C.c_void_p(sizes.data_ptr() + 8 * i),
                                       C.c_void_p(ws.data_ptr()), wsb, stream))

        def unpack(i):
            N.check(L.csic_unpack_device(pl._h, C.c_void_p(coded[i].data_ptr()), 1, C.c_void_p(back[i].data_ptr()), C.c_void_p(ws.data_ptr()), wsb, stream))

        def copy(i):
            N.check(L.csic_copy_device(C.c_void_p(copy_dst.data_ptr()), C.c_void_p(src[i].data_ptr()), copy_px, stream))

        def stats(i):
            N.check(L.csic_code_stats_device(pl._h, C.c_void_p(src[i].data_ptr()), N.FMT_PLANAR_BITS, 1, C.c_void_p(hist.data_ptr()), stream))

        # lossless on every frame of the ring before anything is timed (the buffers are zero outside the payload ranges)
        for i in range(rot):
            pack(i)
            unpack(i)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(src, back)), "unpack(pack(x)) != x"
        coded_bytes = float(sizes.double().mean())
        t = timed_alternating({"pack": pack, "unpack": unpack, "copy": copy, "stats": stats}, rot)
        moved = {"pack": 2 * payload + coded_bytes, "unpack": coded_bytes + payload, "copy": 2 * 4 * copy_px, "stats": payload}
        names = {"pack": pl.pack_kernel_name, "unpack": pl.pack_kernel_name.replace("k_pack", "k_unpack"), "copy": "csic_copy_device",
                 "stats": pl.code_stats_kernel_name(N.FMT_PLANAR_BITS)}
        for key, us in t.items():
            med = statistics.median(us)
            rows.append({"shape": f"{W}x{H}", "chroma": "4:2:0", "factor": f, "bits": list(bits), "content": content, "what": key,
                         "kernel": names[key], "ring": rot, "us": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
                         "payload_bytes": int(payload), "coded_bytes": round(coded_bytes), "ratio": round(coded_bytes / payload, 4),
                         "bytes_moved": round(moved[key]), "TBs": round(moved[key] / (med * 1e-6) / 1e12, 3),
                         "frac_of_8TBs": round(moved[key] / (med * 1e-6) / PEAK, 4)})
            print(json.dumps(rows[-1]), flush=True)
    torch.cuda.empty_cache()
    return rows


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/pack_rates.py measures on a GPU: no HIP device visible")
    tile = torch.from_numpy(read_png(os.path.join(ROOT, "tests", "golden", "inputs", "in512.png")).view(np.int32)).cuda()
    rows = []
    for f in (1, 2):
        for bits in ((8, 8, 8), (6, 5, 5), (3, 3, 2)):
            for content in ("noise", "natural"):
                rows += cell(bits, f, content, tile)
    os.makedirs(os.path.dirname(PREFIX) or ".", exist_ok=True)
    with open(PREFIX + ".jsonl", "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
    with open(PREFIX + ".md", "w") as fh:
        fh.write("# csic_pack_device / csic_unpack_device on 8192 x 8192, 4:2:0 (tools/pack_rates.py)\n\n"
                 f"One MI355X; per cell a ring of PLANAR_BITS frames in separate buffers larger than the Infinity Cache; median of {REPS} windows of "
                 f"{CALLS} calls, the four operations of a cell interleaved.  Bytes moved: pack = 2 x payload + coded, unpack = coded + payload, "
                 "copy = 2 x payload, stats = payload.\n\n"
                 "| f | bits | content | coded / raw | operation | us / frame (min - max) | MiB moved | TB/s | of 8 TB/s |\n"
                 "|---|---|---|---:|---|---:|---:|---:|---:|\n")
        for r in rows:
            fh.write(f"| {r['factor']} | {'/'.join(map(str, r['bits']))} | {r['content']} | {r['ratio']:.3f} | {r['what']} `{r['kernel']}` | {r['us']:.1f} "
                     f"({r['us_min']:.1f} - {r['us_max']:.1f}) | {r['bytes_moved'] / 2 ** 20:.1f} | {r['TBs']:.2f} | {100 * r['frac_of_8TBs']:.1f} % |\n")


if __name__ == "__main__":
    main()
