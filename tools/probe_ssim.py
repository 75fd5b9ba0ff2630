#!/usr/bin/env python3
"""tools/probe_ssim.py [OUT.jsonl] -- the SSIM kernels (csic_ssim_device) next to the distortion kernels (csic_distortion_device) on
the same frames, in one process, timed with device events (the JSON lines go to stdout, and to OUT.jsonl when it is given).
Each call takes the next of ROT input buffers holding different frames, 768 MiB at 8192 x 8192 -- three times the Infinity Cache --
so that no call finds its input cached.  A timed window is CALLS calls back to back between one pair of events (the queue stays
full: launch latency is not in the figure); the measurements take turns window by window, and the figure is the median of the
REPS window means (min and max are kept).  A call is the pixel kernel plus the reduction kernel, through the C ABI with
preallocated buffers.
Rate: the fraction of 8 TB/s on 4 * W * H bytes -- the input, read once; partials, sums and the map are < 1 % of it and not counted.
Cases: 8192 x 8192 4:2:0 at factor 1 and 2 (chroma first, HOLD: k_ssim_fast / k_dist_fast), the same with CSIC_TUNE_FORCE_GENERIC,
8192 x 8192 AVG 4:2:0 factor 2 and 1000 x 1000 spatial-first factor 8 (k_ssim_gen / k_dist_gen); at factor 1 also with the map
written, against d_map = NULL."""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import csic_amd as csic  # noqa: E402

N = csic._native
OUT = sys.argv[1] if len(sys.argv) > 1 else None
CSQ, SCQ = (3, 1, 2), (1, 3, 2)
REPS, CALLS, WARM, ROT = 9, 12, 1, 3
PEAK = 8.0e12


def synth(npix, seed):
    d = torch.empty(npix, dtype=torch.int32, device="cuda:0")
    N.check(N.lib().csic_synth_frame_device(C.c_void_p(d.data_ptr()), npix, 0, seed, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return d


def timed_alternating(fns):
    """fns: {name: fn(buffer index)} -> {name: [us per call of each timed window]}; the functions take turns window by window."""
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


def figure(us, nbytes, kernel):
    med = statistics.median(us)
    return {"kernel": kernel, "us": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2), "bytes": nbytes,
            "frac_of_8TBs": round(nbytes / (med * 1e-6) / PEAK, 4)}


def plan(W, H, a, b, f, op=CSQ, avg=False):
    return csic.Plan(csic.make_c_params(W, H, a, b, 6, 5, 5, f, op, sampling=1 if avg else 0), 0)


def case(name, bufs, W, H, a, b, f, op=CSQ, avg=False, generic=False, with_map=False, **kw):
    nbytes = 4 * W * H
    with plan(W, H, a, b, f, op, avg) as pl:
        if generic:
            pl.tune(N.TUNE_FORCE_GENERIC, 1)
        L, stream = N.lib(), pl._stream()
        sums = torch.empty((2, 6), dtype=torch.int64, device="cuda:0")
        ws = torch.empty(max(pl.distortion_workspace_bytes(1), pl.ssim_workspace_bytes(1)) // 8 + 1, dtype=torch.int64, device="cuda:0")
        qmap = torch.empty((6,) + pl.ssim_windows, dtype=torch.int32, device="cuda:0")
        ptr = lambda t: C.c_void_p(t.data_ptr())
        fns = {"dist": lambda i: N.check(L.csic_distortion_device(pl._h, ptr(bufs[i]), 1, ptr(sums[0]), ptr(ws), ws.numel() * 8, stream)),
               "ssim": lambda i: N.check(L.csic_ssim_device(pl._h, ptr(bufs[i]), 1, ptr(sums[1]), None, ptr(ws), ws.numel() * 8, stream))}
        if with_map:
            fns["ssim_map"] = lambda i: N.check(L.csic_ssim_device(pl._h, ptr(bufs[i]), 1, ptr(sums[1]), ptr(qmap), ptr(ws),
                                                                   ws.numel() * 8, stream))
        t = timed_alternating(fns)
        r = {"case": name, "shape": f"{W}x{H}", "factor": f, "chroma": f"4:{a}:{b}", "sampling": "AVG" if avg else "HOLD", **kw,
             "distortion": figure(t["dist"], nbytes, pl.distortion_kernel_name), "ssim": figure(t["ssim"], nbytes, pl.ssim_kernel_name)}
        r["ssim_over_distortion"] = round(r["ssim"]["us"] / r["distortion"]["us"], 3)
        if with_map:
            r["ssim_with_map"] = figure(t["ssim_map"], nbytes, pl.ssim_kernel_name)
            r["map_cost_us"] = round(r["ssim_with_map"]["us"] - r["ssim"]["us"], 2)
    print(json.dumps(r), flush=True)
    return r


def main():
    rows = []
    W = H = 8192
    bufs = [synth(W * H, 20250629 + k) for k in range(ROT)]
    rows.append(case("8k_420_f1", bufs, W, H, 2, 0, 1, order="C-first", with_map=True))
    rows.append(case("8k_420_f2", bufs, W, H, 2, 0, 2, order="C-first"))
    rows.append(case("8k_420_f1_force_generic", bufs, W, H, 2, 0, 1, order="C-first", generic=True))
    rows.append(case("8k_420_f2_force_generic", bufs, W, H, 2, 0, 2, order="C-first", generic=True))
    rows.append(case("8k_avg_420_f2", bufs, W, H, 2, 0, 2, order="C-first", avg=True))
    del bufs
    torch.cuda.empty_cache()
    W = H = 1000
    bufs = [synth(W * H, 7 + k) for k in range(ROT)]
    rows.append(case("1000_s_first_f8", bufs, W, H, 2, 0, 8, op=SCQ, order="S-first"))
    if OUT:
        os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
        with open(OUT, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
