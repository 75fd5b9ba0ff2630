#!/usr/bin/env python3
"""tools/delta_rates.py [OUT_PREFIX] -- what csic_delta_device and csic_undelta_device cost on one MI355X, and what the temporal layer
saves.  Writes OUT_PREFIX.jsonl and OUT_PREFIX.md (default profiles/r16_delta_rates); the JSON lines also go to stdout.

Speed: sequences of 16 frames of 3840 x 2160 at 4:2:0 6/5/5, factor 1 (order chroma, spatial, quant), gop 16 and gop 1, two contents --
  patch : tests/golden/inputs/in512.png tiled over the frame, static, with a 96 x 96 patch moving 24 px per frame,
  noise : csic_synth_frame_device frames, every frame different (nothing to gain: every group stays intra).
Method (tools/pack_rates.py's): the library compresses the frames itself into a ring of ROT sequences in separate buffers, ROT chosen so
that the ring exceeds 300 MiB (the Infinity Cache holds 256 MiB); delta, undelta and the two yardsticks -- csic_copy_device of the same
payload (16 frames read once, written once) and csic_rice_pack_device of the same 16 frames -- take turns window by window after a
warm-up round; a window is CALLS calls back to back between two device events, the figure the median of REPS window means, with min and
max.  Before anything is timed undelta(delta(x)) is compared with x on every sequence of the ring.
Bytes: delta = payload read + payload written + maps written; undelta = payload + maps read + payload written; copy = 2 x payload; the
Rice coder = 2 x payload read + coded bytes written.  Rates are those bytes over the time, also as a fraction of 8 TB/s.

Sizes: the four sequences of tests/test_delta_sequences.py (8 frames from in512.png at 512 x 512, three parameter sets, both codings),
processed on the device, written on the host as version 5 (gop 8) and frame by frame: the stored bytes of all 8 frames over the same
frames each coded alone."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import csic_amd as csic  # noqa: E402

N = csic._native
PREFIX = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r16_delta_rates")
CSQ = (3, 1, 2)
W, H, BITS, NF = 3840, 2160, (6, 5, 5), 16
REPS, CALLS, WARM = 5, 4, 1
RING_BYTES = 300 << 20
PEAK = 8.0e12


def read_png(path):
    w, h = C.c_int32(), C.c_int32()
    N.check(N.lib().csic_png_info(path.encode(), C.byref(w), C.byref(h)))
    px = np.empty(w.value * h.value, dtype=np.uint32)
    N.check(N.lib().csic_png_read_argb(path.encode(), px.ctypes.data_as(C.c_void_p), px.size))
    return px.reshape(h.value, w.value)


def input_frame(content, seq, k, tile):
    if content == "noise":
        d = torch.empty(W * H, dtype=torch.int32, device="cuda:0")
        N.check(N.lib().csic_synth_frame_device(C.c_void_p(d.data_ptr()), W * H, 0, 20261020 + NF * seq + k, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return d
    base = torch.roll(tile.repeat(-(-H // tile.shape[0]), -(-W // tile.shape[1])), (97 * seq, 41 * seq), dims=(1, 0))[:H, :W].clone()
    base[64 + 24 * k:160 + 24 * k, 64 + 24 * k:160 + 24 * k] = tile[208:304, 208:304]
    return base.contiguous().reshape(-1)


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


def speed_cell(content, gop, tile):
    L = N.lib()
    rows = []
    with csic.Plan(csic.make_c_params(W, H, 2, 0, *BITS, 1, CSQ, out_format=N.FMT_PLANAR_BITS), 0) as pl:
        lay, ml, rl = pl.planar_bits_layout, pl.delta_layout, pl.rice_layout
        fb, payload, ms, bound = lay.frame_bytes, lay.payload_bytes, ml.map_stride, rl.bound_bytes
        rot = max(2, -(-RING_BYTES // (NF * fb)))
        src = []
        for s in range(rot):
            buf = torch.zeros((NF, fb), dtype=torch.uint8, device="cuda:0")
            for k in range(NF):
                pl.process_device(input_frame(content, s, k, tile), buf[k])
            src.append(buf)
        diff = [torch.zeros((NF, fb), dtype=torch.uint8, device="cuda:0") for _ in range(rot)]
        maps = [torch.zeros((NF, ms), dtype=torch.uint8, device="cuda:0") for _ in range(rot)]
        back = [torch.zeros((NF, fb), dtype=torch.uint8, device="cuda:0") for _ in range(rot)]
        coded = torch.empty((NF, bound), dtype=torch.uint8, device="cuda:0")
        sizes = torch.zeros(NF, dtype=torch.int64, device="cuda:0")
        wsb = pl.rice_workspace_bytes(NF)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
        copy_px = NF * fb // 4
        copy_dst = torch.empty(copy_px, dtype=torch.int32, device="cuda:0")
        stream = pl._stream()
        p = lambda t: C.c_void_p(t.data_ptr())

        def delta(i):
            N.check(L.csic_delta_device(pl._h, p(src[i]), NF, gop, p(diff[i]), p(maps[i]), stream))

        def undelta(i):
            N.check(L.csic_undelta_device(pl._h, p(diff[i]), p(maps[i]), NF, gop, p(back[i]), stream))

        def copy(i):
            N.check(L.csic_copy_device(p(copy_dst), p(src[i]), copy_px, stream))

        def rice(i):
            N.check(L.csic_rice_pack_device(pl._h, p(diff[i]), NF, p(coded), p(sizes), p(ws), wsb, stream))

        for i in range(rot):
            delta(i)
            undelta(i)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(src, back)), "undelta(delta(x)) != x"
        groups = sum(ml.groups)
        inter = sum(int(np.unpackbits(m.cpu().numpy()[:, :ml.map_bytes]).sum()) for m in maps) / (rot * NF * groups)
        rice(0)
        torch.cuda.synchronize()
        coded_bytes = float(sizes.double().sum())
        alone, _ = pl.rice_pack_device(src[0], NF)
        alone_bytes = float(_.double().sum())
        del alone
        t = timed_alternating({"delta": delta, "undelta": undelta, "copy": copy, "rice_pack": rice}, rot)
        mapb = NF * ml.map_bytes
        moved = {"delta": 2 * NF * payload + mapb, "undelta": 2 * NF * payload + mapb, "copy": 2 * 4 * copy_px, "rice_pack": 2 * NF * payload + coded_bytes}
        names = {"delta": pl.delta_kernel_name, "undelta": pl.delta_kernel_name.replace("k_delta", "k_undelta"), "copy": "csic_copy_device",
                 "rice_pack": pl.rice_kernel_name}
        copy_us = statistics.median(t["copy"])
        for key, us in t.items():
            med = statistics.median(us)
            rows.append({"shape": f"{W}x{H}", "frames": NF, "gop": gop, "chroma": "4:2:0", "bits": list(BITS), "content": content, "what": key,
                         "kernel": names[key], "ring": rot, "us": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
                         "payload_bytes": int(NF * payload), "inter_share": round(inter, 4),
                         "rice_bytes_delta": round(coded_bytes + mapb * (NF - (NF + gop - 1) // gop) / NF), "rice_bytes_alone": round(alone_bytes),
                         "bytes_moved": round(moved[key]), "TBs": round(moved[key] / (med * 1e-6) / 1e12, 3),
                         "frac_of_8TBs": round(moved[key] / (med * 1e-6) / PEAK, 4), "times_copy": round(med / copy_us, 3)})
            print(json.dumps(rows[-1]), flush=True)
    torch.cuda.empty_cache()
    return rows


def size_rows():
    from test_delta_sequences import NFRAMES, SETS, sequences
    argb = read_png(os.path.join(ROOT, "tests", "golden", "inputs", "in512.png"))
    rgb = np.stack([(argb >> 16) & 0xFF, (argb >> 8) & 0xFF, argb & 0xFF], axis=-1).astype(np.uint8)
    out = []
    tmp = PREFIX + ".tmp.csic"
    for name, frames in sequences(rgb).items():
        for coding in ("groups", "rice"):
            row = {"sequence": name, "coding": coding, "ratios": [], "inter": []}
            for a, b, bits in SETS:
                with csic.Plan(csic.make_c_params(512, 512, a, b, *bits, 1, CSQ, out_format=N.FMT_PLANAR_BITS), 0) as pl:
                    px = np.stack([(np.uint32(0xFF000000) | (f[..., 0].astype(np.uint32) << 16) | (f[..., 1].astype(np.uint32) << 8) | f[..., 2]).reshape(-1)
                                   for f in frames])
                    bufs = pl.process_device(torch.from_numpy(px.reshape(-1).view(np.int32)).cuda(), None, NFRAMES).cpu().numpy().reshape(NFRAMES, -1)
                    csic.write_container(tmp, pl.c_params, bufs, coding=coding, gop=NFRAMES)
                    seq = int(csic.container_coded_sizes(tmp).sum())
                    inter = csic.container_inter_groups(tmp)[1:].sum() / ((NFRAMES - 1) * sum(pl.delta_layout.groups))
                    csic.write_container(tmp, pl.c_params, bufs, coding=coding)
                    row["ratios"].append(round(seq / int(csic.container_coded_sizes(tmp).sum()), 4))
                    row["inter"].append(round(float(inter), 4))
            out.append(row)
            print(json.dumps(row), flush=True)
    os.remove(tmp)
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/delta_rates.py measures on a GPU: no HIP device visible")
    tile = torch.from_numpy(read_png(os.path.join(ROOT, "tests", "golden", "inputs", "in512.png")).view(np.int32)).cuda()
    os.makedirs(os.path.dirname(PREFIX) or ".", exist_ok=True)
    rows = []
    for content in ("patch", "noise"):
        for gop in (16, 1):
            rows += speed_cell(content, gop, tile)
    sizes = size_rows()
    with open(PREFIX + ".jsonl", "w") as fh:
        for r in rows + sizes:
            fh.write(json.dumps(r) + "\n")
    with open(PREFIX + ".md", "w") as fh:
        fh.write(f"# csic_delta_device / csic_undelta_device on {NF} frames of {W} x {H}, 4:2:0 6/5/5, factor 1 (tools/delta_rates.py)\n\n"
                 f"One MI355X; per cell a ring of sequences in separate buffers larger than the Infinity Cache; median of {REPS} windows of {CALLS} calls "
                 f"of {NF} frames each, the four operations of a cell interleaved.  Bytes moved: delta and undelta = 2 x payload + maps, copy = 2 x payload, "
                 "rice_pack = 2 x payload + coded.  Nothing here is tuned: the figures say how far the unit is from the copy.\n\n"
                 "| content | gop | inter groups | Rice bytes, delta / alone | operation | us / 16 frames (min - max) | MiB moved | TB/s | of 8 TB/s | x copy |\n"
                 "|---|---:|---:|---:|---|---:|---:|---:|---:|---:|\n")
        for r in rows:
            fh.write(f"| {r['content']} | {r['gop']} | {r['inter_share']:.3f} | {r['rice_bytes_delta'] / r['rice_bytes_alone']:.3f} | {r['what']} `{r['kernel']}` | "
                     f"{r['us']:.1f} ({r['us_min']:.1f} - {r['us_max']:.1f}) | {r['bytes_moved'] / 2 ** 20:.1f} | {r['TBs']:.2f} | {100 * r['frac_of_8TBs']:.1f} % | "
                     f"{r['times_copy']:.2f} |\n")
        fh.write("\n## Sizes: 8 frames from in512.png at 512 x 512, one key frame and 7 delta frames over the same frames each coded alone\n\n"
                 "The sequences of tests/test_delta_sequences.py (A: static with a moving 96 x 96 patch, C: +-1 RGB noise per frame, D: the left half "
                 "scrolls 3 rows per frame, B: the whole frame pans 2 px per frame), from the library's own stored sizes.\n\n"
                 "| sequence | coding | 4:2:0 6/5/5 | 4:4:4 8/8/8 | 4:2:0 3/3/2 | groups taken inter |\n|---|---|---:|---:|---:|---:|\n")
        for r in sizes:
            fh.write(f"| {r['sequence']} | {r['coding']} | " + " | ".join(f"{x:.3f}" for x in r["ratios"]) + f" | {min(r['inter']):.2f} - {max(r['inter']):.2f} |\n")


if __name__ == "__main__":
    main()
