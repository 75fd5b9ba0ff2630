#!/usr/bin/env python3
"""tools/mc_rates.py [OUT_PREFIX] -- what csic_mc_delta_device and csic_mc_undelta_device cost on one MI355X next to csic_delta_device and
a copy, and what the motion-compensated layer saves.  Writes OUT_PREFIX.jsonl and OUT_PREFIX.md (default profiles/r18_mc_rates); the
JSON lines also go to stdout.

Speed: sequences of 16 frames of 3840 x 2160 at 4:2:0 6/5/5, factor 1 (order chroma, spatial, quant): tests/golden/inputs/in512.png tiled
over the frame and panned by (1, 2) pixels per frame, so that the search has something to find.  Method (tools/delta_rates.py's): the
library compresses the frames itself into a ring of ROT sequences in separate buffers, ROT chosen so that the ring exceeds 300 MiB (the
Infinity Cache holds 256 MiB); the operations take turns window by window after a warm-up round; a window is CALLS calls back to back
between two device events, the figure the median of REPS window means, with min and max.  Before anything is timed
mc_undelta(mc_delta(x)) is compared with x on every sequence of the ring.  The entry point does not expose its kernels one by one:
csic_mc_delta_device at range 0 launches no search (k_mc_table and k_mc_delta with a table of one entry), so the lines at range 2 and 4
less the line at range 0 are the search plus the pricing of the longer table.  Search and delta apart: `tools/mc_rates.py trace R` under
`rocprofv3 --kernel-trace --stats`, then `tools/mc_rates.py merge PREFIX 2=DIR 4=DIR` appends the per-kernel durations to OUT_PREFIX.md.

Sizes: sequences A, B, D of tests/test_delta_sequences.py and the diagonal pan of tests/test_mc_sequences.py (8 frames from in512.png at
512 x 512, three parameter sets, both codings, gop 8), host codecs: per frame the coded difference frame plus, for a delta frame, its
map, over the same frames each coded alone -- under csic_delta_* (what a version-5 file stores) and under csic_mc_*."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import csic_amd as csic  # noqa: E402
from delta_rates import read_png, timed_alternating  # noqa: E402

N = csic._native
PREFIX = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] not in ("trace", "merge") else os.path.join(ROOT, "profiles", "r18_mc_rates")
CSQ = (3, 1, 2)
W, H, BITS, NF = 3840, 2160, (6, 5, 5), 16
RING_BYTES = 300 << 20


def speed_rows(tile):
    L = N.lib()
    rows = []
    with csic.Plan(csic.make_c_params(W, H, 2, 0, *BITS, 1, CSQ, out_format=N.FMT_PLANAR_BITS), 0) as pl:
        lay, dl, ml = pl.planar_bits_layout, pl.delta_layout, pl.mc_layout
        fb, payload = lay.frame_bytes, lay.payload_bytes
        rot = max(2, -(-RING_BYTES // (NF * fb)))
        big = tile.repeat(-(-H // tile.shape[0]) + 1, -(-W // tile.shape[1]) + 1)
        src = []
        for s in range(rot):
            buf = torch.zeros((NF, fb), dtype=torch.uint8, device="cuda:0")
            for k in range(NF):
                pl.process_device(big[37 * s + k:37 * s + k + H, 53 * s + 2 * k:53 * s + 2 * k + W].contiguous().reshape(-1), buf[k])
            src.append(buf)
        mk = lambda shape: [torch.zeros(shape, dtype=torch.uint8, device="cuda:0") for _ in range(rot)]
        diff, back, maps, mmaps = mk((NF, fb)), mk((NF, fb)), mk((NF, dl.map_stride)), mk((NF, ml.map_stride))
        wsb = NF * ml.workspace_frame_bytes
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
        copy_px = NF * fb // 4
        copy_dst = torch.empty(copy_px, dtype=torch.int32, device="cuda:0")
        stream = pl._stream()
        p = lambda t: C.c_void_p(t.data_ptr())
        inter = {}

        def mc_delta(R, gop=NF):
            return lambda i: N.check(L.csic_mc_delta_device(pl._h, p(src[i]), NF, gop, R, p(diff[i]), p(mmaps[i]), p(ws), wsb, stream))

        def mc_undelta(gop):
            return lambda i: N.check(L.csic_mc_undelta_device(pl._h, p(diff[i]), p(mmaps[i]), NF, gop, p(back[i]), stream))

        for R in (0, 2, 4):
            for i in range(rot):
                mc_delta(R)(i)
                mc_undelta(NF)(i)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(src, back)), "mc_undelta(mc_delta(x)) != x"
            nib = np.concatenate([m.cpu().numpy()[1:, 192:ml.map_bytes].reshape(-1) for m in mmaps])
            inter[R] = (np.count_nonzero(nib & 15) + np.count_nonzero(nib >> 4)) / (rot * (NF - 1) * sum(ml.groups))
        fns = {"copy": lambda i: N.check(L.csic_copy_device(p(copy_dst), p(src[i]), copy_px, stream)),
               "delta gop 16": lambda i: N.check(L.csic_delta_device(pl._h, p(src[i]), NF, NF, p(diff[i]), p(maps[i]), stream)),
               "mc_delta R=0 gop 16": mc_delta(0), "mc_delta R=2 gop 16": mc_delta(2), "mc_delta R=4 gop 16": mc_delta(4)}
        t = timed_alternating(fns, rot)
        for i in range(rot):                                    # the maps of range 4 are in place again for the decoder
            mc_delta(4)(i)
        torch.cuda.synchronize()
        t.update(timed_alternating({"mc_undelta gop 16": mc_undelta(NF), "mc_undelta gop 1": mc_undelta(1),
                                    "copy (again)": fns["copy"]}, rot))
        copy_us = statistics.median(t["copy"])
        for key, us in t.items():
            med = statistics.median(us)
            R = int(key.split("R=")[1][0]) if "R=" in key else None
            rows.append({"shape": f"{W}x{H}", "frames": NF, "chroma": "4:2:0", "bits": list(BITS), "content": "tiled in512.png panned (1, 2) per frame",
                         "what": key, "kernel": pl.mc_kernel_name.replace("k_mc_delta", "k_mc_undelta") if key.startswith("mc_undelta") else pl.mc_kernel_name
                         if key.startswith("mc_") else pl.delta_kernel_name if key.startswith("delta") else "csic_copy_device",
                         "ring": rot, "us": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1), "payload_bytes": int(NF * payload),
                         "inter_share": None if R is None else round(inter[R], 4), "times_copy": round(med / copy_us, 2)})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def size_rows():
    from test_delta_sequences import NFRAMES, SETS, sequences
    argb = read_png(os.path.join(ROOT, "tests", "golden", "inputs", "in512.png"))
    rgb = np.stack([(argb >> 16) & 0xFF, (argb >> 8) & 0xFF, argb & 0xFF], axis=-1).astype(np.uint8)
    seqs = sequences(rgb)
    todo = [("B", seqs["B"], 2), ("D", seqs["D"], 4), ("P", [np.roll(np.roll(rgb, 3 * k, axis=0), -2 * k, axis=1) for k in range(NFRAMES)], 4), ("A", seqs["A"], 2)]
    coders = {"groups": csic.pack_frame_host, "rice": csic.rice_pack_host}
    out = []
    for name, frames, R in todo:
        for coding, coder in coders.items():
            row = {"sequence": name, "range": R, "coding": coding, "delta": [], "mc": []}
            for a, b, bits in SETS:
                with csic.Plan(csic.make_c_params(512, 512, a, b, *bits, 1, CSQ, out_format=N.FMT_PLANAR_BITS), 0) as pl:
                    px = np.stack([(np.uint32(0xFF000000) | (f[..., 0].astype(np.uint32) << 16) | (f[..., 1].astype(np.uint32) << 8) | f[..., 2]).reshape(-1)
                                   for f in frames])
                    bufs = pl.process_device(torch.from_numpy(px.reshape(-1).view(np.int32)).cuda(), None, NFRAMES).cpu().numpy().reshape(NFRAMES, -1)
                    cp = pl.c_params
                    alone = sum(len(coder(cp, f)) for f in bufs)
                    d5, _ = csic.delta_host(cp, bufs, NFRAMES)
                    d6, _ = csic.mc_delta_host(cp, bufs, NFRAMES, R)
                    row["delta"].append(round((sum(len(coder(cp, f)) for f in d5) + (NFRAMES - 1) * pl.delta_layout.map_bytes) / alone, 4))
                    row["mc"].append(round((sum(len(coder(cp, f)) for f in d6) + (NFRAMES - 1) * pl.mc_layout.map_bytes) / alone, 4))
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def trace_run(R):
    """`tools/mc_rates.py trace R`, to be run under `rocprofv3 --kernel-trace --stats` (nothing else traced): 8 calls of
    csic_mc_delta_device at range R and of csic_mc_undelta_device on the speed table's frames, so that the profiler's per-kernel
    durations tell the search from the delta kernel."""
    tile = torch.from_numpy(read_png(os.path.join(ROOT, "tests", "golden", "inputs", "in512.png")).view(np.int32)).cuda()
    with csic.Plan(csic.make_c_params(W, H, 2, 0, *BITS, 1, CSQ, out_format=N.FMT_PLANAR_BITS), 0) as pl:
        fb = pl.planar_bits_layout.frame_bytes
        rot = max(2, -(-RING_BYTES // (NF * fb)))
        big = tile.repeat(-(-H // tile.shape[0]) + 1, -(-W // tile.shape[1]) + 1)
        src = []
        for s in range(rot):
            buf = torch.zeros((NF, fb), dtype=torch.uint8, device="cuda:0")
            for k in range(NF):
                pl.process_device(big[37 * s + k:37 * s + k + H, 53 * s + 2 * k:53 * s + 2 * k + W].contiguous().reshape(-1), buf[k])
            src.append(buf)
        for i in range(8):
            diff, maps = pl.mc_delta_device(src[i % rot], NF, NF, R)
            pl.mc_undelta_device(diff, maps, NF, NF)
        torch.cuda.synchronize()


def merge_trace(prefix, dirs):
    """`tools/mc_rates.py merge PREFIX R=DIR ...`: the kernel_stats.csv of each traced run -> a table appended to PREFIX.md."""
    import csv
    import glob
    lines = ["\n## The kernels one by one (rocprofv3 --kernel-trace --stats of `tools/mc_rates.py trace R`, no other tracing)\n\n"
             "Per range 8 calls of csic_mc_delta_device and of csic_mc_undelta_device (gop 16) on the frames of the first table; us per call of 16 "
             "frames = the kernel's total time over the 8 calls (a call launches a kernel once per run of planes of equal width: Y, then Cb and Cr; the "
             "decoder 16 times that).  The profiler serialises less than the windows above, so the sums need not meet them.\n\n"
             "| range | kernel | launches | us / call of 16 frames |\n|---:|---|---:|---:|\n"]
    for item in dirs:
        R, d = item.split("=")
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if "k_mc_" in row["Name"]:
                    name = row["Name"].replace("void ", "").replace("csic::", "").split("(")[0]
                    lines.append(f"| {R} | `{name}` | {int(row['Calls'])} | {float(row['TotalDurationNs']) / 8 / 1e3:.1f} |\n")
    with open(prefix + ".md", "a") as fh:
        fh.writelines(lines)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "trace":
        return trace_run(int(sys.argv[2]))
    if len(sys.argv) > 3 and sys.argv[1] == "merge":
        return merge_trace(sys.argv[2], sys.argv[3:])
    if not torch.cuda.is_available():
        raise SystemExit("tools/mc_rates.py measures on a GPU: no HIP device visible")
    tile = torch.from_numpy(read_png(os.path.join(ROOT, "tests", "golden", "inputs", "in512.png")).view(np.int32)).cuda()
    os.makedirs(os.path.dirname(PREFIX) or ".", exist_ok=True)
    rows = speed_rows(tile)
    sizes = size_rows()
    with open(PREFIX + ".jsonl", "w") as fh:
        for r in rows + sizes:
            fh.write(json.dumps(r) + "\n")
    with open(PREFIX + ".md", "w") as fh:
        fh.write(f"# csic_mc_delta_device / csic_mc_undelta_device on {NF} frames of {W} x {H}, 4:2:0 6/5/5, factor 1 (tools/mc_rates.py)\n\n"
                 "One MI355X; a ring of sequences in separate buffers larger than the Infinity Cache; median of 5 windows of 4 calls of 16 frames each, "
                 "the operations of a table interleaved window by window.  The content is in512.png tiled and panned by (1, 2) pixels per frame.  "
                 "Range 0 launches no search: the lines at range 2 and 4 less that line are the search plus the pricing of a longer table.  "
                 "Nothing here is tuned: the figures say how far the unit is from the copy.\n\n"
                 "| operation | us / 16 frames (min - max) | x copy | groups taken inter |\n|---|---:|---:|---:|\n")
        for r in rows:
            share = "" if r["inter_share"] is None else f"{r['inter_share']:.3f}"
            fh.write(f"| {r['what']} `{r['kernel']}` | {r['us']:.1f} ({r['us_min']:.1f} - {r['us_max']:.1f}) | {r['times_copy']:.2f} | {share} |\n")
        fh.write("\n## Sizes: 8 frames from in512.png at 512 x 512, one key frame and 7 delta frames over the same frames each coded alone\n\n"
                 "B: the whole frame pans 2 px per frame; D: the left half scrolls 3 rows per frame; P: the whole frame pans (3, -2) per frame; A: static "
                 "with a moving 96 x 96 patch.  Host codecs; a delta frame's size includes its map.  Each cell: csic_delta_* -> csic_mc_*.\n\n"
                 "| sequence | range | coding | 4:2:0 6/5/5 | 4:4:4 8/8/8 | 4:2:0 3/3/2 |\n|---|---:|---|---:|---:|---:|\n")
        for r in sizes:
            fh.write(f"| {r['sequence']} | {r['range']} | {r['coding']} | " + " | ".join(f"{x:.3f} -> {y:.3f}" for x, y in zip(r["delta"], r["mc"])) + " |\n")


if __name__ == "__main__":
    main()
