#!/usr/bin/env python3
"""tools/rows_rates.py [OUT_PREFIX] -- what csic_rows_device and csic_unrows_device cost on one MI355X, and what the row-prediction
layer saves.  Writes OUT_PREFIX.jsonl and OUT_PREFIX.md (default profiles/r23_rows_rates); the JSON lines also go to stdout.

Speed: frames of 8192 x 8192 (one per call) and of 3840 x 2160 (eight per call) at 4:2:0 6/5/5, factor 1 (order chroma, spatial,
quant), two contents --
  natural : tests/golden/inputs/in512.png tiled over the frame, shifted from frame to frame,
  noise   : csic_synth_frame_device frames (nothing to gain: both predictors are equally bad, about half of the groups take either).
Method (tools/delta_rates.py's): the library compresses the frames itself into a ring of ROT calls' worth of frames in separate
buffers, ROT chosen so that the ring exceeds 300 MiB (the Infinity Cache holds 256 MiB); rows, unrows and the yardsticks --
csic_copy_device of the same payload, and csic_delta_device / csic_undelta_device at gop 1 (every frame a key frame: the same bytes
through the same accessors without the layer's arithmetic) -- take turns window by window after a warm-up round; a window is CALLS
calls back to back between two device events, the figure the median of REPS window means, with min and max.  Before anything is timed
unrows(rows(x)) is compared with x on every buffer of the ring.
Bytes: rows = payload read + payload written + maps written (its reference groups are the neighbours' own groups: they come from the
caches); unrows = payload + maps read + payload written; delta / undelta the same; copy = 2 x payload.

Sizes: in512.png at four parameter sets and the three codings, processed on the device, written on the host with the layer (version 8)
and without (versions 3 / 4 / 7): the table of tests/test_rows_sizes.py from the library's own stored sizes."""
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
PREFIX = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r23_rows_rates")
CSQ = (3, 1, 2)
BITS = (6, 5, 5)
SHAPES = ((8192, 8192, 1), (3840, 2160, 8))
SETS = [(2, 0, (6, 5, 5)), (4, 4, (8, 8, 8)), (2, 0, (3, 3, 2)), (2, 0, (4, 4, 4))]
REPS, CALLS, WARM = 5, 4, 1
RING_BYTES = 300 << 20
PEAK = 8.0e12


def read_png(path):
    w, h = C.c_int32(), C.c_int32()
    N.check(N.lib().csic_png_info(path.encode(), C.byref(w), C.byref(h)))
    px = np.empty(w.value * h.value, dtype=np.uint32)
    N.check(N.lib().csic_png_read_argb(path.encode(), px.ctypes.data_as(C.c_void_p), px.size))
    return px.reshape(h.value, w.value)


def input_frame(content, W, H, seed, tile):
    if content == "noise":
        d = torch.empty(W * H, dtype=torch.int32, device="cuda:0")
        N.check(N.lib().csic_synth_frame_device(C.c_void_p(d.data_ptr()), W * H, 0, 20261021 + seed, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return d
    return torch.roll(tile.repeat(-(-H // tile.shape[0]), -(-W // tile.shape[1])), (97 * seed, 41 * seed), dims=(1, 0))[:H, :W].contiguous().reshape(-1)


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


def speed_cell(W, H, NF, content, tile):
    L = N.lib()
    rows = []
    with csic.Plan(csic.make_c_params(W, H, 2, 0, *BITS, 1, CSQ, out_format=N.FMT_PLANAR_BITS), 0) as pl:
        lay, ml = pl.planar_bits_layout, pl.rows_layout
        fb, payload, ms = lay.frame_bytes, lay.payload_bytes, ml.map_stride
        assert pl.delta_layout.map_stride == ms
        rot = max(2, -(-RING_BYTES // (NF * fb)))
        src = []
        for s in range(rot):
            buf = torch.zeros((NF, fb), dtype=torch.uint8, device="cuda:0")
            for k in range(NF):
                pl.process_device(input_frame(content, W, H, NF * s + k, tile), buf[k])
            src.append(buf)
        diff = [torch.zeros((NF, fb), dtype=torch.uint8, device="cuda:0") for _ in range(rot)]
        maps = [torch.zeros((NF, ms), dtype=torch.uint8, device="cuda:0") for _ in range(rot)]
        back = [torch.zeros((NF, fb), dtype=torch.uint8, device="cuda:0") for _ in range(rot)]
        kdiff = torch.zeros((NF, fb), dtype=torch.uint8, device="cuda:0")
        kmaps = torch.zeros((NF, ms), dtype=torch.uint8, device="cuda:0")
        copy_px = NF * fb // 4
        copy_dst = torch.empty(copy_px, dtype=torch.int32, device="cuda:0")
        stream = pl._stream()
        p = lambda t: C.c_void_p(t.data_ptr())

        def rows_(i):
            N.check(L.csic_rows_device(pl._h, p(src[i]), NF, p(diff[i]), p(maps[i]), stream))

        def unrows(i):
            N.check(L.csic_unrows_device(pl._h, p(diff[i]), p(maps[i]), NF, p(back[i]), stream))

        def delta(i):
            N.check(L.csic_delta_device(pl._h, p(src[i]), NF, 1, p(kdiff), p(kmaps), stream))

        def undelta(i):
            N.check(L.csic_undelta_device(pl._h, p(src[i]), p(kmaps), NF, 1, p(kdiff), stream))

        def copy(i):
            N.check(L.csic_copy_device(p(copy_dst), p(src[i]), copy_px, stream))

        for i in range(rot):
            rows_(i)
            unrows(i)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(src, back)), "unrows(rows(x)) != x"
        above = sum(int(np.unpackbits(m.cpu().numpy()[:, :ml.map_bytes]).sum()) for m in maps) / (rot * NF * sum(ml.groups))
        t = timed_alternating({"rows": rows_, "unrows": unrows, "delta_gop1": delta, "undelta_gop1": undelta, "copy": copy}, rot)
        moved = 2 * NF * payload + NF * ml.map_bytes
        names = {"rows": pl.rows_kernel_name, "unrows": pl.rows_kernel_name.replace("k_rows", "k_unrows"), "delta_gop1": pl.delta_kernel_name,
                 "undelta_gop1": pl.delta_kernel_name.replace("k_delta", "k_undelta"), "copy": "csic_copy_device"}
        copy_us = statistics.median(t["copy"])
        for key, us in t.items():
            med = statistics.median(us)
            b = 2 * 4 * copy_px if key == "copy" else moved
            rows.append({"shape": f"{W}x{H}", "frames": NF, "chroma": "4:2:0", "bits": list(BITS), "content": content, "what": key, "kernel": names[key], "ring": rot,
                         "us": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1), "payload_bytes": int(NF * payload),
                         "above_share": round(above, 4), "bytes_moved": int(b), "TBs": round(b / (med * 1e-6) / 1e12, 3),
                         "frac_of_8TBs": round(b / (med * 1e-6) / PEAK, 4), "times_copy": round(med / copy_us, 3)})
            print(json.dumps(rows[-1]), flush=True)
    torch.cuda.empty_cache()
    return rows


def size_rows():
    argb = read_png(os.path.join(ROOT, "tests", "golden", "inputs", "in512.png"))
    out = []
    tmp = PREFIX + ".tmp.csic"
    for a, b, bits in SETS:
        with csic.Plan(csic.make_c_params(512, 512, a, b, *bits, 1, CSQ, out_format=N.FMT_PLANAR_BITS), 0) as pl:
            buf = pl.process_device(torch.from_numpy(argb.reshape(-1).view(np.int32)).cuda()).cpu().numpy().reshape(1, -1)
            for coding in ("groups", "rice", "rans"):
                csic.write_container(tmp, pl.c_params, buf, coding=coding)
                alone = int(csic.container_coded_sizes(tmp)[0])
                csic.write_container(tmp, pl.c_params, buf, coding=coding, rows=True)
                got = int(csic.container_coded_sizes(tmp)[0])
                share = (csic.container_inter_groups(tmp)[0] / np.array(list(pl.rows_layout.groups))).round(3).tolist()
                out.append({"set": f"4:{a}:{b} {bits[0]}/{bits[1]}/{bits[2]}", "coding": coding, "today": alone, "with_rows": got, "ratio": round(got / alone, 4),
                            "above_share": share})
                print(json.dumps(out[-1]), flush=True)
    os.remove(tmp)
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/rows_rates.py measures on a GPU: no HIP device visible")
    tile = torch.from_numpy(read_png(os.path.join(ROOT, "tests", "golden", "inputs", "in512.png")).view(np.int32)).cuda()
    os.makedirs(os.path.dirname(PREFIX) or ".", exist_ok=True)
    rows = []
    for W, H, NF in SHAPES:
        for content in ("natural", "noise"):
            rows += speed_cell(W, H, NF, content, tile)
    sizes = size_rows()
    with open(PREFIX + ".jsonl", "w") as fh:
        for r in rows + sizes:
            fh.write(json.dumps(r) + "\n")
    with open(PREFIX + ".md", "w") as fh:
        fh.write("# csic_rows_device / csic_unrows_device at 4:2:0 6/5/5, factor 1 (tools/rows_rates.py)\n\n"
                 f"One MI355X; per cell a ring of buffers larger than the Infinity Cache; median of {REPS} windows of {CALLS} calls, the five operations of a "
                 "cell interleaved.  Bytes moved: rows, unrows, delta and undelta = 2 x payload + maps, copy = 2 x payload.  delta / undelta run at gop 1 "
                 "(every frame a key frame): the same bytes through the same accessors without the layer's arithmetic.  Nothing here is tuned and no "
                 "figure is a gate.\n\n"
                 "| shape x frames | content | groups from above | operation | us / call (min - max) | MiB moved | TB/s | of 8 TB/s | x copy |\n"
                 "|---|---|---:|---|---:|---:|---:|---:|---:|\n")
        for r in rows:
            fh.write(f"| {r['shape']} x {r['frames']} | {r['content']} | {r['above_share']:.3f} | {r['what']} `{r['kernel']}` | "
                     f"{r['us']:.1f} ({r['us_min']:.1f} - {r['us_max']:.1f}) | {r['bytes_moved'] / 2 ** 20:.1f} | {r['TBs']:.2f} | {100 * r['frac_of_8TBs']:.1f} % | "
                     f"{r['times_copy']:.2f} |\n")
        fh.write("\n## Sizes: in512.png, one frame, stored bytes without and with the layer (maps included)\n\n"
                 "| set | coding | today | with rows | ratio | groups from above Y / Cb / Cr |\n|---|---|---:|---:|---:|---|\n")
        for r in sizes:
            fh.write(f"| {r['set']} | {r['coding']} | {r['today']} | {r['with_rows']} | {r['ratio']:.3f} | " + " / ".join(f"{x:.2f}" for x in r["above_share"]) + " |\n")


if __name__ == "__main__":
    main()
