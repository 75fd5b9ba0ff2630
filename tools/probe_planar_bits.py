#!/usr/bin/env python3
"""tools/probe_planar_bits.py [OUT.jsonl] -- (the JSON lines go to stdout, and to OUT.jsonl when it is given) the bit-packed planar kernels (CSIC_FMT_PLANAR_BITS) timed with device events in one
process, each next to the kernel it is compared against on the same frame: k_pbits_f1 vs k_planar_flat (8192x8192 4:2:0, factor 1,
8/8/8, 6/5/5, 4/4/4, 3/3/2), k_pbits_strided vs k_planar_strided (cfg4: factor 2, 6/5/5), k_rbits vs k_recon, and the general
kernel (k_pbits_gen) on an AVG case and on a HOLD case.  Rates are fractions of 8 TB/s on the algorithmic bytes: input + payload
for the forward kernels (csic_algorithmic_bytes), payload + 4 bytes per output pixel for reconstruct."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import csic_amd as csic  # noqa: E402

N = csic._native
OUT = sys.argv[1] if len(sys.argv) > 1 else None
W = H = 8192
CSQ = (3, 1, 2)
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
    return a.elapsed_time(b) * 1e3 / ITERS          # us per launch


def plan(bits, f, fmt, avg=False, variant=0):
    pl = csic.Plan(csic.make_c_params(W, H, 2, 0, *bits, f, CSQ, out_format=fmt, sampling=1 if avg else 0), 0)
    if variant:
        pl.tune(N.TUNE_VARIANT, variant)
    return pl


def forward(pl, d_in):
    out = torch.empty(pl.frame_bytes, dtype=torch.uint8, device="cuda:0")
    us = timed(lambda: pl.process_device(d_in, out))
    return out, {"kernel": pl.kernel_name, "us": round(us, 2), "alg_bytes": pl.algorithmic_bytes,
                 "frac_of_8TBs": round(pl.algorithmic_bytes / (us * 1e-6) / PEAK, 4)}


def main():
    d_in = torch.empty(W * H, dtype=torch.int32, device="cuda:0")
    sh = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    N.check(N.lib().csic_synth_frame_device(C.c_void_p(d_in.data_ptr()), d_in.numel(), 0, 20250629, sh))
    rows = []

    def emit(case, bits, f, new, ref, **kw):
        r = {"case": case, "shape": f"{W}x{H}", "chroma": "4:2:0", "factor": f, "bits": list(bits), "bits_kernel": new, "compared_with": ref, **kw}
        rows.append(r)
        print(json.dumps(r), flush=True)

    for bits in ((8, 8, 8), (6, 5, 5), (4, 4, 4), (3, 3, 2)):
        with plan(bits, 1, csic.PixelFormat.PLANAR_BITS) as pb, plan(bits, 1, csic.PixelFormat.PLANAR) as pp:
            _, rb = forward(pb, d_in)
            _, rp = forward(pp, d_in)
            emit("forward_f1", bits, 1, rb, rp, bytes_per_pixel=round(pb.planar_bits_layout.payload_bytes / (W * H), 4))
    bits = (6, 5, 5)
    with plan(bits, 2, csic.PixelFormat.PLANAR_BITS) as pb, plan(bits, 2, csic.PixelFormat.PLANAR) as pp:
        _, rb = forward(pb, d_in)
        _, rp = forward(pp, d_in)
        emit("forward_cfg4", bits, 2, rb, rp)
    with plan(bits, 1, csic.PixelFormat.PLANAR_BITS) as pb, plan(bits, 1, csic.PixelFormat.PLANAR) as pp:
        fb, _ = forward(pb, d_in)
        fp, _ = forward(pp, d_in)
        out = torch.empty(W * H, dtype=torch.int32, device="cuda:0")
        res = []
        for pl, buf, rec, payload in ((pb, fb, pl_bits_rec, pb.planar_bits_layout.payload_bytes), (pp, fp, pl_rec, pp.planar_layout.payload_bytes)):
            us = timed(lambda: rec(pl, buf, out))
            alg = payload + 4 * W * H
            res.append({"kernel": "k_rbits" if pl is pb else "k_recon", "us": round(us, 2), "alg_bytes": alg,
                        "frac_of_8TBs": round(alg / (us * 1e-6) / PEAK, 4)})
        emit("reconstruct_f1_argb", bits, 1, res[0], res[1])
    with plan(bits, 1, csic.PixelFormat.PLANAR_BITS, avg=True) as pb, plan(bits, 1, csic.PixelFormat.PLANAR, avg=True) as pp:
        _, rb = forward(pb, d_in)
        _, rp = forward(pp, d_in)
        emit("forward_f1_avg_general", bits, 1, rb, rp, sampling="AVG")
    with plan(bits, 1, csic.PixelFormat.PLANAR_BITS, variant=9) as pb, plan(bits, 1, csic.PixelFormat.PLANAR) as pp:
        _, rb = forward(pb, d_in)
        _, rp = forward(pp, d_in)
        emit("forward_f1_hold_general_variant9", bits, 1, rb, rp)
    if OUT:
        os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
        with open(OUT, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


def pl_bits_rec(pl, buf, out):
    pl.reconstruct_bits_device(buf, out)


def pl_rec(pl, buf, out):
    pl.reconstruct_device(buf, out)


if __name__ == "__main__":
    main()
