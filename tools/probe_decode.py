#!/usr/bin/env python3
"""tools/probe_decode.py [OUT.jsonl] -- the full-resolution decode (csic_decode_device) timed with device events in one process, the
protocol of tools/probe_distortion.py (the JSON lines go to stdout, and to OUT.jsonl when it is given).
Shapes: 8192x8192 4:2:0 at factor 1, 2 and 4, and 64 frames of 3840x2160 at factor 4 in one call; each from PLANAR_BITS 6/5/5, from
PLANAR and from the packed YCbCr stream, to ARGB.  Rate: the fraction of 8 TB/s on 4 * W * H bytes written plus the source bytes
read (the planes' payload, or 4 bytes per source pixel), per frame.  Two reference points per shape, same process, same buffers:
csic_reconstruct_bits_device on the same plan (at factor 1 the identical work; at factor f it writes 1 / f^2 of the decode's bytes)
and csic_copy_device over W * H pixels (reads and writes 4 W H bytes: the streaming ceiling bench.py reports).  The bit-packed
source is also timed at every CSIC_TUNE_BLOCK_THREADS."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import csic_amd as csic  # noqa: E402

N = csic._native
OUT = sys.argv[1] if len(sys.argv) > 1 else None
CSQ = (3, 1, 2)
ITERS, WARM = 40, 5
PEAK = 8.0e12
BITS, PLANAR, YCC, ARGB = N.FMT_PLANAR_BITS, N.FMT_PLANAR, N.FMT_YCBCR888X, N.FMT_ARGB8888


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


def plan(W, H, f, fmt):
    return csic.Plan(csic.make_c_params(W, H, 2, 0, 6, 5, 5, f, CSQ, out_format=fmt), 0)


def rate(nbytes, us):
    return {"us": round(us, 2), "bytes": int(nbytes), "frac_of_8TBs": round(nbytes / (us * 1e-6) / PEAK, 4)}


def case(name, W, H, f, nf, emit):
    d_in = synth(W * H * nf)
    out_bytes = 4 * W * H * nf
    d_out = torch.empty((nf, H, W), dtype=torch.int32, device="cuda:0")
    row = {"shape": f"{nf}x{W}x{H}" if nf > 1 else f"{W}x{H}", "factor": f, "chroma": "4:2:0", "bits": "6/5/5", "nframes": nf}
    with plan(W, H, f, BITS) as pl:
        lay = pl.planar_bits_layout
        src_bytes = {BITS: lay.payload_bytes * nf, PLANAR: pl.planar_layout.payload_bytes * nf, YCC: 4 * pl.out_width * pl.out_height * nf}
        srcs = {}
        for fmt in (BITS, PLANAR, YCC):
            with plan(W, H, f, fmt) as pf:
                srcs[fmt] = pf.process_device(d_in, nframes=nf)
        del d_in
        want = None
        for fmt, label in ((BITS, "from_bits"), (PLANAR, "from_planar"), (YCC, "from_ycc")):
            us = timed(lambda: pl.decode_device(srcs[fmt], fmt, d_out, nframes=nf))
            row[label] = {"kernel": pl.decode_kernel_name(fmt, ARGB), **rate(out_bytes + src_bytes[fmt], us)}
            if want is None:
                want = d_out.clone()
            else:
                assert torch.equal(d_out, want), label
        del want
        for bt in (64, 128, 256):
            pl.tune(N.TUNE_BLOCK_THREADS, bt)
            us = timed(lambda: pl.decode_device(srcs[BITS], BITS, d_out, nframes=nf))
            row[f"from_bits_T{bt}"] = rate(out_bytes + src_bytes[BITS], us)
        pl.tune(N.TUNE_BLOCK_THREADS, 0)
        small = torch.empty((nf, pl.out_height, pl.out_width), dtype=torch.int32, device="cuda:0")
        us = timed(lambda: pl.reconstruct_bits_device(srcs[BITS], small, nframes=nf))
        row["reconstruct_bits"] = rate(4 * pl.out_width * pl.out_height * nf + src_bytes[BITS], us)
        del small, srcs
    d_src = torch.empty_like(d_out)
    d_src.copy_(d_out)
    sh = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    us = timed(lambda: N.check(N.lib().csic_copy_device(C.c_void_p(d_out.data_ptr()), C.c_void_p(d_src.data_ptr()), W * H * nf, sh)))
    row["copy_WH"] = rate(2 * out_bytes, us)
    emit(name, **row)
    del d_out, d_src
    torch.cuda.empty_cache()


def main():
    rows = []

    def emit(case_name, **kw):
        r = {"case": case_name, **kw}
        rows.append(r)
        print(json.dumps(r), flush=True)

    for f in (1, 2, 4):
        case(f"8k_420_f{f}", 8192, 8192, f, 1, emit)
    case("uhd_420_f4_x64", 3840, 2160, 4, 64, emit)
    if OUT:
        os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
        with open(OUT, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
