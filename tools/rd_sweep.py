#!/usr/bin/env python3
"""tools/rd_sweep.py [OUT_PREFIX] -- the rate-distortion table of the committed golden inputs (tests/golden/inputs/in128.png and
in512.png) on the GPU: chroma 4:4:4 / 4:2:2 / 4:2:0 / 4:1:1 x bits 8/8/8, 6/5/5, 4/4/4, 3/3/2 x factor 1, 2 x HOLD / AVG (order
chroma, spatial, quant).  Rate: bits per input pixel of the bit-packed planar frame, 8 * csic_planar_bits_layout_of(...).payload_bytes
/ (W * H).  Distortion: csic_distortion_host -> PSNR-RGB and PSNR-Y / Cb / Cr (dB, inf when lossless); csic_ssim_host -> the mean
8 x 8 block SSIM of Y, Cb, Cr and of R, G, B together.  What the samples really carry: csic_code_stats_host on the bit-packed frame
-> bits per input pixel of an ideal order-0 coder of the codes (H0), of their left-predicted residuals (H1), and of the cheapest of
raw, H0 and H1 per plane (best).  Writes OUT_PREFIX.jsonl and OUT_PREFIX.md (default profiles/r11_rd_sweep; profiles/r09_rd_sweep.* is
the table from before the entropy columns, profiles/r06_rd_sweep.* the one from before the SSIM columns)."""
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import csic_amd as csic  # noqa: E402

N = csic._native
PREFIX = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r11_rd_sweep")
CSQ = (3, 1, 2)
CHROMA = (("4:4:4", 4, 4), ("4:2:2", 2, 2), ("4:2:0", 2, 0), ("4:1:1", 1, 1))
BITS = ((8, 8, 8), (6, 5, 5), (4, 4, 4), (3, 3, 2))


def read_png(path):
    w, h = C.c_int32(), C.c_int32()
    N.check(N.lib().csic_png_info(path.encode(), C.byref(w), C.byref(h)))
    px = np.empty(w.value * h.value, dtype=np.uint32)
    N.check(N.lib().csic_png_read_argb(path.encode(), px.ctypes.data_as(C.c_void_p), px.size))
    return px.reshape(h.value, w.value)


def fmt_db(v):
    return "inf" if math.isinf(v) else f"{v:.2f}"


def main():
    rows = []
    for name in ("in128", "in512"):
        img = read_png(os.path.join(ROOT, "tests", "golden", "inputs", name + ".png"))
        H, W = img.shape
        for cname, a, b in CHROMA:
            for bits in BITS:
                for f in (1, 2):
                    for sampling in ("HOLD", "AVG"):
                        cp = csic.make_c_params(W, H, a, b, *bits, f, CSQ, sampling=1 if sampling == "AVG" else 0)
                        lay = N.CsicPlanarBitsLayout()
                        N.check(N.lib().csic_planar_bits_layout_of(C.byref(cp), C.byref(lay)))
                        with csic.Plan(cp, 0) as pl:
                            d = pl.distortion(img)
                            q = pl.ssim(img)
                            kernel, ssim_kernel = pl.distortion_kernel_name, pl.ssim_kernel_name
                        cpb = csic.make_c_params(W, H, a, b, *bits, f, CSQ, sampling=1 if sampling == "AVG" else 0, out_format=N.FMT_PLANAR_BITS)
                        with csic.Plan(cpb, 0) as plb:
                            st = plb.code_stats(plb.process_host(img))
                            stats_kernel = plb.code_stats_kernel_name()
                        r = {"image": name, "shape": f"{W}x{H}", "chroma": cname, "bits": list(bits), "factor": f, "sampling": sampling,
                             "bpp": round(8 * lay.payload_bytes / (W * H), 4), "psnr_rgb": round(d.psnr_rgb, 3),
                             "psnr_y": round(d.psnr("Y"), 3), "psnr_cb": round(d.psnr("Cb"), 3), "psnr_cr": round(d.psnr("Cr"), 3),
                             "sse": list(d.sse), "kernel": kernel, "ssim_rgb": round(q.mean_rgb, 5), "ssim_y": round(q.mean("Y"), 5),
                             "ssim_cb": round(q.mean("Cb"), 5), "ssim_cr": round(q.mean("Cr"), 5), "ssim_sums": list(q.sums),
                             "ssim_windows": q.windows, "ssim_kernel": ssim_kernel,
                             "h0_bpp": round(st.bits_per_pixel(0), 4), "h1_bpp": round(st.bits_per_pixel(1), 4),
                             "best_bpp": round(st.bits_per_pixel("best"), 4), "best_bytes": st.ideal_bytes("best"),
                             "entropy": [[round(st.entropy(k, p), 4) for p in range(3)] for k in range(2)], "stats_kernel": stats_kernel}
                        rows.append(r)
                        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(PREFIX) or ".", exist_ok=True)
    with open(PREFIX + ".jsonl", "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
    with open(PREFIX + ".md", "w") as fh:
        fh.write("# Rate-distortion of the golden inputs (tools/rd_sweep.py)\n\n"
                 "Order chroma, spatial, quant; floor rounding.  bpp = bits per input pixel of the bit-packed planar frame "
                 "(csic_planar_bits_layout_of payload); PSNR in dB against the input, every input pixel paired with its output "
                 "pixel by replication (csic_distortion_*); SSIM is the mean 8 x 8 block SSIM of the same pairing (csic_ssim_*), "
                 "SSIM-RGB the mean of the R, G and B means.  H0 / px, H1 / px and best / px are bits per input pixel after an ideal "
                 "order-0 entropy coder of the sample codes, of their left-predicted residuals, and of the cheapest of raw, H0 and H1 "
                 "per plane (csic_code_stats_*): what the bpp column could shrink to, not what any file here holds.\n\n")
        fh.write("| image | chroma | bits | f | sampling | bpp | H0 / px | H1 / px | best / px | PSNR-RGB | PSNR-Y | PSNR-Cb | PSNR-Cr | SSIM-RGB | SSIM-Y | SSIM-Cb | SSIM-Cr |\n"
                 "|---|---|---|---|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|\n")
        for r in rows:
            fh.write(f"| {r['image']} | {r['chroma']} | {'/'.join(map(str, r['bits']))} | {r['factor']} | {r['sampling']} | {r['bpp']:.3f} | "
                     f"{r['h0_bpp']:.3f} | {r['h1_bpp']:.3f} | {r['best_bpp']:.3f} | {fmt_db(r['psnr_rgb'])} | {fmt_db(r['psnr_y'])} | {fmt_db(r['psnr_cb'])} | {fmt_db(r['psnr_cr'])} | "
                     f"{r['ssim_rgb']:.4f} | {r['ssim_y']:.4f} | {r['ssim_cb']:.4f} | {r['ssim_cr']:.4f} |\n")


if __name__ == "__main__":
    main()
