#!/usr/bin/env python3
"""tools/qsweep_rates.py [OUT_PREFIX] -- what the one-pass quantiser sweep costs next to the route it replaces, on one MI355X.
Writes OUT_PREFIX.md (default profiles/r22_qsweep_rates); the JSON lines behind it go to stdout.

Per shape (8192 x 8192 and 3840 x 2160), factor (1 and 2) and content (in512.png tiled and rolled per frame; one constant colour, the
worst case of the LDS atomics), at 4:2:0, order chroma, spatial, quant, four operations are timed in the same run, window by window
in turn (the method of tools/pack_rates.py: a ring of input frames in separate buffers larger than the Infinity Cache, windows of
CALLS calls between two device events, the median of REPS window means with min and max):
  sweep   csic_qsweep_device: the 24 sums and 24 histograms of one frame
  hist    csic_qsweep_hist_device on the 8/8/8 planar frame: the rate half of the sweep alone (the rest of `sweep` is the SSE kernel, the
          sum of its partials and the planar kernel)
  route   what it replaces: the 8/8/8 CSIC_FMT_PLANAR process, 8 x csic_distortion_device (one per width, each reading the input) and
          8 x csic_code_stats_device on that planar frame (one per width)
  copy    csic_copy_device of the input frame
Before anything is timed the sweep's table is compared with what the route gives, on the first frame of the ring."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import csic_amd as csic  # noqa: E402
from pack_rates import CSQ, RING_BYTES, read_png, REPS, CALLS, WARM  # noqa: E402

N = csic._native
PREFIX = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r22_qsweep_rates")
SHAPES = [(8192, 8192), (3840, 2160)]
WORDS = C.sizeof(N.CsicQsweepResult) // 8


def input_frame(content, k, tile, w, h):
    if content == "constant":
        return torch.full((w * h,), 0xFF4080C0 - (1 << 32), dtype=torch.int32, device="cuda:0")
    reps = (-(-h // tile.shape[0]), -(-w // tile.shape[1]))
    return torch.roll(tile.repeat(*reps)[:h, :w], (37 * k, 11 * k), dims=(1, 0)).contiguous().reshape(-1)


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


def cell(w, h, f, content, tile):
    L, P = N.lib(), C.c_void_p
    rows = []
    px = w * h
    rot = max(3, -(-RING_BYTES // (4 * px)))
    src = [input_frame(content, k, tile, w, h) for k in range(rot)]
    plans = [csic.Plan(csic.make_c_params(w, h, 2, 0, q, q, q, f, CSQ, out_format=N.FMT_PLANAR), 0) for q in range(1, 9)]
    try:
        pl = plans[7]
        stream = pl._stream()
        wsb = max(pl.qsweep_workspace_bytes(1), pl.distortion_workspace_bytes(1))
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
        res = torch.zeros(WORDS, dtype=torch.int64, device="cuda:0")
        res2 = torch.zeros(WORDS, dtype=torch.int64, device="cuda:0")
        planar = torch.zeros(pl.planar_layout.frame_bytes, dtype=torch.uint8, device="cuda:0")
        sse = torch.zeros((8, N.DIST_CHANNELS), dtype=torch.int64, device="cuda:0")
        hist = torch.zeros((8, N.STATS_KINDS, N.STATS_PLANES, N.STATS_BINS), dtype=torch.int64, device="cuda:0")
        copy_dst = torch.empty(px, dtype=torch.int32, device="cuda:0")

        def sweep(i):
            N.check(L.csic_qsweep_device(pl._h, P(src[i].data_ptr()), 1, P(res.data_ptr()), P(ws.data_ptr()), wsb, stream))

        def route(i):
            N.check(L.csic_process_device(pl._h, P(src[i].data_ptr()), P(planar.data_ptr()), stream))
            for q, pq in enumerate(plans):
                N.check(L.csic_distortion_device(pq._h, P(src[i].data_ptr()), 1, P(sse[q].data_ptr()), P(ws.data_ptr()), wsb, stream))
            for q, pq in enumerate(plans):
                N.check(L.csic_code_stats_device(pq._h, P(planar.data_ptr()), N.FMT_PLANAR, 1, P(hist[q].data_ptr()), stream))

        def hist_only(i):
            N.check(L.csic_qsweep_hist_device(pl._h, P(planar.data_ptr()), 1, P(res2.data_ptr()), stream))

        def copy(i):
            N.check(L.csic_copy_device(P(copy_dst.data_ptr()), P(src[i].data_ptr()), px, stream))

        sweep(0)
        route(0)
        torch.cuda.synchronize()
        r = res.cpu().numpy().view(np.uint64)
        assert np.array_equal(r[:24].reshape(3, 8), sse.cpu().numpy().view(np.uint64)[:, 3:].T), "the sweep's sums differ from csic_distortion_device"
        assert np.array_equal(r[24:].reshape(3, 8, 256), hist.cpu().numpy().view(np.uint64)[:, 1].transpose(1, 0, 2)), "the sweep's histograms differ"
        t = timed_alternating({"sweep": sweep, "hist": hist_only, "route": route, "copy": copy}, rot)
        for what, us in t.items():
            rows.append({"shape": f"{w}x{h}", "factor": f, "content": content, "what": what, "kernel": pl.qsweep_kernel_name if what == "sweep" else "",
                         "ring": rot, "us": round(statistics.median(us), 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1)})
            print(json.dumps(rows[-1]), flush=True)
    finally:
        for p in plans:
            p.close()
    del src
    torch.cuda.empty_cache()
    return rows


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/qsweep_rates.py measures on a GPU: no HIP device visible")
    tile = torch.from_numpy(read_png(os.path.join(ROOT, "tests", "golden", "inputs", "in512.png")).view(np.int32)).cuda()
    rows = []
    for w, h in SHAPES:
        for f in (1, 2):
            for content in ("natural", "constant"):
                rows += cell(w, h, f, content, tile)
    os.makedirs(os.path.dirname(PREFIX) or ".", exist_ok=True)
    us = {(r["shape"], r["factor"], r["content"], r["what"]): r for r in rows}
    with open(PREFIX + ".md", "w") as fh:
        fh.write("# csic_qsweep_device against the route it replaces (tools/qsweep_rates.py)\n\n"
                 f"One MI355X, one run; 4:2:0, order chroma, spatial, quant; a ring of input frames in separate buffers larger than the Infinity "
                 f"Cache; median of {REPS} windows of {CALLS} calls (min - max), the four operations interleaved window by window.  `route` is the "
                 "8/8/8 planar process + 8 x csic_distortion_device + 8 x csic_code_stats_device on the planar frame; `hist` is the sweep's rate "
                 "half alone (csic_qsweep_hist_device on that planar frame); `copy` is csic_copy_device of the input frame.  The sweep's table was compared with the route's results before timing.\n\n"
                 "| shape | factor | content | sweep kernel | sweep us | of which hist us | route us | copy us | route / sweep | sweep / copy |\n|---|---:|---|---|---:|---:|---:|---:|---:|---:|\n")
        for (shape, f, content, what), r in us.items():
            if what != "sweep":
                continue
            ro, co, hi = us[(shape, f, content, "route")], us[(shape, f, content, "copy")], us[(shape, f, content, "hist")]
            cellf = lambda x: f"{x['us']:.1f} ({x['us_min']:.1f} - {x['us_max']:.1f})"
            fh.write(f"| {shape} | {f} | {content} | `{r['kernel']}` | {cellf(r)} | {cellf(hi)} | {cellf(ro)} | {cellf(co)} | {ro['us'] / r['us']:.2f} | {r['us'] / co['us']:.2f} |\n")


if __name__ == "__main__":
    main()
