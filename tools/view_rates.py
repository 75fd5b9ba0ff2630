#!/usr/bin/env python3
"""tools/view_rates.py [OUT_PREFIX] -- what csic_decode_view_device costs on one MI355X next to the route to the same pixels that the
library offered before it.  Writes OUT_PREFIX.jsonl and OUT_PREFIX.md (default profiles/r25_view_rates); the JSON lines also go to
stdout.

Frames of 8192 x 8192 at 4:2:0 6/5/5 (order chroma, spatial, quant), factor 1 and factor 2, from PLANAR_BITS to ARGB, four views:
  thumb8  : the whole frame at scale 8  (1024 x 1024 out)        thumb16 : the whole frame at scale 16 (512 x 512 out)
  uhd2    : a 3840 x 2160 output at scale 2 (7680 x 4320 source)  crop1   : a 1920 x 1080 window at scale 1, x0 = 1001, y0 = 777
Per view four operations take turns, window by window after a warm-up round (tools/rows_rates.py's method): a window is CALLS calls
back to back between two device events, the figure the median of REPS window means, with min and max --
  view        csic_decode_view_device
  decode      csic_decode_device of the whole frame (what had to run first before this entry point existed)
  decode+box  decode, then the crop and the integer box sum in torch: the earlier route to the same pixels, end to end
  copy        csic_copy_device of as many bytes as the view reads and writes
The sources are a ring of compressed frames larger than the Infinity Cache (256 MiB), call i reading buffer i % ring.  Before anything
is timed the view is compared with decode+box, pixel for pixel.
Bytes of a view: the share of the planes' payload under the source rectangle, read once, + 4 bytes per output pixel.  Nothing here is
tuned and no figure is a gate."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import csic_amd as csic  # noqa: E402

N = csic._native
PREFIX = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r25_view_rates")
CSQ = (3, 1, 2)
BITS = (6, 5, 5)
W = H = 8192
VIEWS = [("thumb8", csic.View(0, 0, 1024, 1024, 8)), ("thumb16", csic.View(0, 0, 512, 512, 16)), ("uhd2", csic.View(0, 0, 3840, 2160, 2)),
         ("crop1", csic.View(1001, 777, 1920, 1080, 1))]
REPS, CALLS, WARM = 5, 10, 1
RING_BYTES = 300 << 20
PEAK = 8.0e12


def box_in_torch(full, v):
    """The earlier route's second half: crop the decoded frame (H, W) int32 and reduce it by the box, byte by byte."""
    s = v.scale
    crop = full[v.y0:v.y0 + v.height * s, v.x0:v.x0 + v.width * s]
    if s == 1:
        return crop.contiguous()
    b = crop.contiguous().view(torch.uint8).reshape(v.height, s, v.width, s, 4).to(torch.int32).sum(dim=(1, 3))
    return ((b + ((s * s) >> 1)) >> (2 * (s.bit_length() - 1))).to(torch.uint8).view(torch.int32).reshape(v.height, v.width)


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


def cells(f):
    L = N.lib()
    rows = []
    with csic.Plan(csic.make_c_params(W, H, 2, 0, *BITS, f, CSQ, out_format=N.FMT_PLANAR_BITS), 0) as pl:
        lay = pl.planar_bits_layout
        rot = max(2, -(-RING_BYTES // lay.frame_bytes))
        src = []
        d_in = torch.empty(W * H, dtype=torch.int32, device="cuda:0")
        stream = pl._stream()
        for s in range(rot):
            N.check(L.csic_synth_frame_device(C.c_void_p(d_in.data_ptr()), W * H, 0, 20261021 + s, stream))
            src.append(pl.process_device(d_in))
        del d_in
        full = torch.empty((H, W), dtype=torch.int32, device="cuda:0")
        for label, v in VIEWS:
            out = torch.empty((v.height, v.width), dtype=torch.int32, device="cuda:0")
            share = (v.width * v.scale) * (v.height * v.scale) / (W * H)
            moved = int(lay.payload_bytes * share) + 4 * v.width * v.height
            copy_px = moved // 8
            copy_src = torch.empty(copy_px, dtype=torch.int32, device="cuda:0")
            copy_dst = torch.empty(copy_px, dtype=torch.int32, device="cuda:0")
            p = lambda t: C.c_void_p(t.data_ptr())

            def view(i):
                pl.decode_view_device(src[i], v, d_out=out)

            def decode(i):
                pl.decode_device(src[i], d_out=full)

            def decode_box(i):
                pl.decode_device(src[i], d_out=full)
                return box_in_torch(full, v)

            def copy(i):
                N.check(L.csic_copy_device(p(copy_dst), p(copy_src), copy_px, stream))

            for i in range(rot):
                view(i)
                assert torch.equal(out, decode_box(i)), (f, label, i)
            torch.cuda.synchronize()
            t = timed_alternating({"view": view, "decode": decode, "decode+box": decode_box, "copy": copy}, rot)
            names = {"view": pl.decode_view_kernel_name(N.FMT_PLANAR_BITS, v), "decode": pl.decode_kernel_name(N.FMT_PLANAR_BITS),
                     "decode+box": pl.decode_kernel_name(N.FMT_PLANAR_BITS) + " + torch", "copy": "csic_copy_device"}
            decode_bytes = lay.payload_bytes + 4 * W * H
            view_us = statistics.median(t["view"])
            for key, us in t.items():
                med = statistics.median(us)
                b = moved if key in ("view", "copy") else decode_bytes
                rows.append({"factor": f, "view": label, "x0": v.x0, "y0": v.y0, "out": f"{v.width}x{v.height}", "scale": v.scale, "what": key,
                             "kernel": names[key], "ring": rot, "us": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
                             "bytes_moved": int(b), "TBs": round(b / (med * 1e-6) / 1e12, 3), "frac_of_8TBs": round(b / (med * 1e-6) / PEAK, 4),
                             "times_view": round(med / view_us, 2)})
                print(json.dumps(rows[-1]), flush=True)
            del out, copy_src, copy_dst
    torch.cuda.empty_cache()
    return rows


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/view_rates.py measures on a GPU: no HIP device visible")
    os.makedirs(os.path.dirname(PREFIX) or ".", exist_ok=True)
    rows = cells(1) + cells(2)
    with open(PREFIX + ".jsonl", "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
    with open(PREFIX + ".md", "w") as fh:
        fh.write("# csic_decode_view_device on 8192 x 8192, 4:2:0 6/5/5, PLANAR_BITS -> ARGB (tools/view_rates.py)\n\n"
                 f"One MI355X; the sources are a ring of compressed frames larger than the Infinity Cache; median of {REPS} windows of {CALLS} calls, the "
                 "four operations of a view interleaved.  Bytes moved: view and copy = the planes' payload under the source rectangle + the output; decode "
                 "and decode+box = the whole payload + the 256 MiB frame (the torch half's traffic is not counted: its row is a time, not a rate).  "
                 "Nothing here is tuned and no figure is a gate.\n\n"
                 "| factor | view | out | scale | operation | us / call (min - max) | MiB moved | TB/s | of 8 TB/s | x view |\n"
                 "|---:|---|---|---:|---|---:|---:|---:|---:|---:|\n")
        for r in rows:
            fh.write(f"| {r['factor']} | {r['view']} | {r['out']} | {r['scale']} | {r['what']} `{r['kernel']}` | {r['us']:.1f} ({r['us_min']:.1f} - {r['us_max']:.1f}) | "
                     f"{r['bytes_moved'] / 2 ** 20:.1f} | {r['TBs']:.2f} | {100 * r['frac_of_8TBs']:.1f} % | {r['times_view']:.2f} |\n")


if __name__ == "__main__":
    main()
