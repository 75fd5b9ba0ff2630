#!/usr/bin/env python3
"""tools/probe_distortion.py [OUT.jsonl] -- the distortion kernels (csic_distortion_device) timed with device events in one process
(the JSON lines go to stdout, and to OUT.jsonl when it is given).  Rate: the fraction of 8 TB/s on 4 * W * H * nframes bytes -- the
input, which the fused measurement reads once; the partials and sums it writes are < 0.3 % of that and not counted.
Cases: 8192x8192 4:2:0 at factor 1 and 2 and 4:4:4 at factor 1 (chroma first, HOLD: k_dist_fast), 8192x8192 AVG 4:2:0 factor 2 and
1000x1000 spatial-first factor 8 (k_dist_gen), 1024 frames of 512x512 4:2:0 factor 2 in one call; the headline shapes also with
CSIC_TUNE_FORCE_GENERIC, and the headline (8192x8192 4:2:0 factor 2) next to the two-pass alternative: the packed ARGB and YCbCr
outputs written by process_device (two launches), then a second pass that compares the input with the ARGB output (torch elementwise
kernels: far from roofline-bound, so the two writes alone are the conservative figure)."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import csic_amd as csic  # noqa: E402

N = csic._native
OUT = sys.argv[1] if len(sys.argv) > 1 else None
CSQ, SCQ = (3, 1, 2), (1, 3, 2)
ITERS, WARM = 40, 5
PEAK = 8.0e12


def timed(fn):
    for _ in range(WARM):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / ITERS          # us per call


def synth(npix):
    d = torch.empty(npix, dtype=torch.int32, device="cuda:0")
    N.check(N.lib().csic_synth_frame_device(C.c_void_p(d.data_ptr()), npix, 0, 20250629, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return d


def plan(W, H, a, b, f, op=CSQ, avg=False, fmt=0):
    return csic.Plan(csic.make_c_params(W, H, a, b, 6, 5, 5, f, op, out_format=fmt, sampling=1 if avg else 0), 0)


def measure(pl, d_in, nframes, generic=False):
    if generic:
        pl.tune(N.TUNE_FORCE_GENERIC, 1)
    sse = torch.empty((nframes, 6), dtype=torch.int64, device="cuda:0")
    us = timed(lambda: pl.distortion_device(d_in, nframes, sse))
    nbytes = 4 * pl.width * pl.height * nframes
    r = {"kernel": pl.distortion_kernel_name, "us": round(us, 2), "bytes": nbytes, "frac_of_8TBs": round(nbytes / (us * 1e-6) / PEAK, 4)}
    if generic:
        pl.tune(N.TUNE_FORCE_GENERIC, 0)
    return r, sse


def compare_kernel(x, o_rgb, f):
    """The second pass over the input and the written ARGB output (torch elementwise kernels); only its time is used."""
    H, W = x.shape
    up = lambda o: o.repeat_interleave(f, 0).repeat_interleave(f, 1)[:H, :W]
    d = (x.view(torch.uint8).view(H, W, 4)[..., :3].to(torch.int32) - up(o_rgb).view(torch.uint8).view(H, W, 4)[..., :3].to(torch.int32))
    return (d * d).sum(dim=(0, 1))


def main():
    rows = []

    def emit(case, **kw):
        r = {"case": case, **kw}
        rows.append(r)
        print(json.dumps(r), flush=True)

    W = H = 8192
    d8k = synth(W * H)
    for name, a, b, f in (("8k_420_f1", 2, 0, 1), ("8k_420_f2", 2, 0, 2), ("8k_444_f1", 4, 4, 1)):
        with plan(W, H, a, b, f) as pl:
            fast, want = measure(pl, d8k, 1)
            gen, got = measure(pl, d8k, 1, generic=True)
            assert torch.equal(want, got)
            emit(name, shape=f"{W}x{H}", factor=f, chroma=f"4:{a}:{b}", order="C-first", sampling="HOLD", fused=fast, force_generic=gen)
    with plan(W, H, 2, 0, 2, avg=True) as pl:
        r, _ = measure(pl, d8k, 1)
        emit("8k_avg_420_f2", shape=f"{W}x{H}", factor=2, chroma="4:2:0", order="C-first", sampling="AVG", fused=r)

    # the headline against two passes: process_device to ARGB and to YCbCr (two launches writing 2 x 1 B/px of output at f = 2),
    # then a comparison pass that reads the input again (timed separately: with torch's elementwise kernels it is far from a
    # roofline-bound kernel, so the two writes alone are the conservative figure)
    with plan(W, H, 2, 0, 2) as pl, plan(W, H, 2, 0, 2, fmt=1) as py:
        o_rgb = torch.empty((pl.out_height, pl.out_width), dtype=torch.int32, device="cuda:0")
        o_ycc = torch.empty_like(o_rgb)
        fused, _ = measure(pl, d8k, 1)
        write_us = timed(lambda: (pl.process_device(d8k, o_rgb), py.process_device(d8k, o_ycc)))
        x2 = d8k.view(H, W)
        cmp_us = timed(lambda: compare_kernel(x2, o_rgb, 2))
        emit("headline_two_pass", shape=f"{W}x{H}", factor=2, chroma="4:2:0", fused=fused,
             two_pass={"process_device_argb_plus_ycc_us": round(write_us, 2), "torch_rgb_compare_us": round(cmp_us, 2),
                       "total_us": round(write_us + cmp_us, 2)},
             fused_faster_than_the_writes_alone=fused["us"] < write_us)
    del d8k
    torch.cuda.empty_cache()

    W = H = 1000
    d1k = synth(W * H)
    with plan(W, H, 2, 0, 8, op=SCQ) as pl:
        r, _ = measure(pl, d1k, 1)
        emit("1000_s_first_f8", shape=f"{W}x{H}", factor=8, chroma="4:2:0", order="S-first", sampling="HOLD", fused=r)
    W = H = 512
    nf = 1024
    dbat = synth(W * H * nf)
    with plan(W, H, 2, 0, 2) as pl:
        r, _ = measure(pl, dbat, nf)
        emit("batch_1024x512sq_420_f2", shape=f"{nf}x{W}x{H}", factor=2, chroma="4:2:0", order="C-first", sampling="HOLD", fused=r)
    if OUT:
        os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
        with open(OUT, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
