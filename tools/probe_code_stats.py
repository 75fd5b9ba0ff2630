#!/usr/bin/env python3
"""tools/probe_code_stats.py [OUT_PREFIX] -- what csic_code_stats_device costs on one MI355X, and what same-bin LDS atomics cost it.
Writes OUT_PREFIX.jsonl and OUT_PREFIX.md (default profiles/r11_code_stats_probe); the JSON lines also go to stdout.

Matrix: 8192 x 8192, 4:2:0, factor 1 (order chroma, spatial, quant) at 8/8/8 and 6/5/5; source formats PLANAR and PLANAR_BITS; the
fast kernel (k_cstat_bytes / k_cstat_bits) beside the general one (k_cstat_gen, CSIC_TUNE_FORCE_GENERIC); three contents --
  noise    : csic_synth_frame_device frames (every bin about equally likely, neighbours independent),
  natural  : tests/golden/inputs/in512.png tiled 16 x 16 (many equal neighbours: many lanes of one LDS atomic on one bin),
  constant : one colour (every lane of every LDS atomic on one bin: the most contention there is).
Method: the frames are compressed on the device by the library itself; each call reads the next of ROT = 5 compressed frames in
separate buffers (340 - 480 MiB, more than the 256 MiB Infinity Cache), so no call finds its source cached.  A timed window is CALLS
calls back to back between two device events (launch latency is hidden behind the queue); the four kernels of one (bits, content)
cell take turns window by window after a warm-up round, and the figure is the median of REPS window means, with min and max.  A
call is the memset of the result plus the counting launch(es), through the C ABI.
Rate: payload bytes of the source (what the kernels read; the 12 KiB result is not counted) over time, as a fraction of 8 TB/s.  The
yardstick is the reads-only streaming figure of profiles/r04_ubench_mix.log, 84 % of 8 TB/s."""
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
PREFIX = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r11_code_stats_probe")
CSQ = (3, 1, 2)
W = H = 8192
REPS, CALLS, WARM, ROT = 7, 10, 1, 5
PEAK, YARDSTICK = 8.0e12, 0.84


def read_png(path):
    w, h = C.c_int32(), C.c_int32()
    N.check(N.lib().csic_png_info(path.encode(), C.byref(w), C.byref(h)))
    px = np.empty(w.value * h.value, dtype=np.uint32)
    N.check(N.lib().csic_png_read_argb(path.encode(), px.ctypes.data_as(C.c_void_p), px.size))
    return px.reshape(h.value, w.value)


def input_frame(content, k, tile):
    """Frame k of the ring for `content`: an int32 CUDA tensor of W * H ARGB pixels."""
    if content == "noise":
        d = torch.empty(W * H, dtype=torch.int32, device="cuda:0")
        N.check(N.lib().csic_synth_frame_device(C.c_void_p(d.data_ptr()), W * H, 0, 20250629 + k,
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return d
    if content == "natural":
        return torch.roll(tile.repeat(H // tile.shape[0], W // tile.shape[1]), 37 * k, dims=1).contiguous().reshape(-1)
    colour = 0xFF000000 | ((0x40 + 17 * k) << 16) | ((0x80 + 5 * k) << 8) | (0xC0 - 11 * k)
    return torch.full((W * H,), colour - (1 << 32), dtype=torch.int32, device="cuda:0")


def compressed_ring(bits, fmt, content, tile):
    """ROT compressed frames of `fmt` in separate buffers, made by the library itself."""
    with csic.Plan(csic.make_c_params(W, H, 2, 0, *bits, 1, CSQ, out_format=fmt), 0) as pl:
        ring = []
        for k in range(ROT):
            ring.append(pl.process_device(input_frame(content, k, tile)))
        torch.cuda.synchronize()
    return ring


def timed_alternating(fns):
    times = {k: [] for k in fns}
    for rep in range(WARM + REPS):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(CALLS):
                fn(i % ROT)
            b.record()
            b.synchronize()
            if rep >= WARM:
                times[k].append(a.elapsed_time(b) * 1e3 / CALLS)
    return times


def cell(bits, content, tile):
    """The four kernels of one (bits, content) cell, interleaved.  Returns the JSON rows."""
    rings = {fmt: compressed_ring(bits, fmt, content, tile) for fmt in (N.FMT_PLANAR, N.FMT_PLANAR_BITS)}
    cp = csic.make_c_params(W, H, 2, 0, *bits, 1, CSQ)
    plans, fns, meta = [], {}, {}
    L = N.lib()
    hist = torch.empty((N.STATS_KINDS, N.STATS_PLANES, N.STATS_BINS), dtype=torch.int64, device="cuda:0")
    checks = {}
    for fmt, fname in ((N.FMT_PLANAR, "planar"), (N.FMT_PLANAR_BITS, "bits")):
        for generic in (False, True):
            pl = csic.Plan(cp, 0)
            plans.append(pl)
            if generic:
                pl.tune(N.TUNE_FORCE_GENERIC, 1)
            lay = pl.planar_bits_layout if fmt == N.FMT_PLANAR_BITS else pl.planar_layout
            key = fname + ("_gen" if generic else "_fast")
            meta[key] = (pl.code_stats_kernel_name(fmt), int(lay.payload_bytes), fname)
            stream = pl._stream()
            fns[key] = (lambda i, pl=pl, fmt=fmt, ring=rings[fmt], stream=stream:
                        N.check(L.csic_code_stats_device(pl._h, C.c_void_p(ring[i].data_ptr()), fmt, 1, C.c_void_p(hist.data_ptr()), stream)))
            checks[key] = pl.code_stats_device(rings[fmt][0], fmt).cpu()
    # the four must agree before anything is timed
    ref = checks["planar_gen"]
    assert all(torch.equal(v, ref) for v in checks.values()), "the kernels disagree on frame 0"
    t = timed_alternating(fns)
    for pl in plans:
        pl.close()
    rows = []
    for key, us in t.items():
        kernel, nbytes, fname = meta[key]
        med = statistics.median(us)
        frac = nbytes / (med * 1e-6) / PEAK
        rows.append({"shape": f"{W}x{H}", "chroma": "4:2:0", "factor": 1, "bits": list(bits), "content": content, "source": fname,
                     "kernel": kernel, "us": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2), "bytes": nbytes,
                     "frac_of_8TBs": round(frac, 4), "of_streaming_yardstick": round(frac / YARDSTICK, 4)})
        print(json.dumps(rows[-1]), flush=True)
    del rings
    torch.cuda.empty_cache()
    return rows


def main():
    tile = torch.from_numpy(read_png(os.path.join(ROOT, "tests", "golden", "inputs", "in512.png")).view(np.int32)).cuda()
    rows = []
    for bits in ((8, 8, 8), (6, 5, 5)):
        for content in ("noise", "natural", "constant"):
            rows += cell(bits, content, tile)
    os.makedirs(os.path.dirname(PREFIX) or ".", exist_ok=True)
    with open(PREFIX + ".jsonl", "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
    with open(PREFIX + ".md", "w") as fh:
        fh.write("# csic_code_stats_device on 8192 x 8192, 4:2:0, factor 1 (tools/probe_code_stats.py)\n\n"
                 f"One MI355X; ring of {ROT} compressed frames in separate buffers (larger than the Infinity Cache); median of {REPS} windows "
                 f"of {CALLS} calls, the four kernels of a cell interleaved.  Rate = source payload bytes / time; the yardstick is the "
                 "reads-only streaming figure, 84 % of 8 TB/s (profiles/r04_ubench_mix.log).\n\n"
                 "| bits | content | source | kernel | us / frame (min - max) | MiB read | of 8 TB/s | of the yardstick |\n"
                 "|---|---|---|---|---:|---:|---:|---:|\n")
        for r in rows:
            fh.write(f"| {'/'.join(map(str, r['bits']))} | {r['content']} | {r['source']} | `{r['kernel']}` | {r['us']:.1f} ({r['us_min']:.1f} - "
                     f"{r['us_max']:.1f}) | {r['bytes'] / 2 ** 20:.1f} | {100 * r['frac_of_8TBs']:.1f} % | {100 * r['of_streaming_yardstick']:.1f} % |\n")
        fh.write("\nContention: time on a constant frame over time on noise, same kernel and bits (1 = same-bin LDS atomics cost nothing).\n\n"
                 "| bits | kernel | natural / noise | constant / noise |\n|---|---|---:|---:|\n")
        us = {(tuple(r["bits"]), r["kernel"], r["content"]): r["us"] for r in rows}
        for (bits, kernel, content), v in us.items():
            if content == "noise":
                fh.write(f"| {'/'.join(map(str, bits))} | `{kernel}` | {us[(bits, kernel, 'natural')] / v:.2f} | {us[(bits, kernel, 'constant')] / v:.2f} |\n")


if __name__ == "__main__":
    main()
