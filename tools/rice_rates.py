#!/usr/bin/env python3
"""tools/rice_rates.py [OUT_PREFIX] -- what the Rice coding saves and what it costs next to the group coding, on one MI355X.
Writes OUT_PREFIX.md (default profiles/r13_rice_rates); the JSON lines behind it go to stdout.

1. Sizes: tests/golden/inputs/in512.png at the README's four parameter sets (factor 1, order chroma, spatial, quant) compressed on the
   device, then coded by csic_pack_device and csic_rice_pack_device: RAW (payload_bytes) / GROUPS / RICE bytes beside the ideal_bytes
   of the code statistics of the same frame (order-0, left-predicted, best per plane).  Each coded frame is unpacked and compared.
2. Times: 8192 x 8192, 4:2:0, 6/5/5, factor 1, on noise and on in512.png tiled 16 x 16 and rolled per frame -- pack and unpack of both
   codings in the same run, window by window in turn, with the method of tools/pack_rates.py: a ring of PLANAR_BITS frames in separate
   buffers larger than the Infinity Cache, windows of CALLS calls between two device events, the median of REPS window means with min
   and max, unpack(pack(x)) == x on every frame of the ring before anything is timed."""
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
from pack_rates import CSQ, H, W, RING_BYTES, input_frame, read_png, timed_alternating, REPS, CALLS  # noqa: E402

N = csic._native
PREFIX = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r13_rice_rates")
SETS = [(4, 4, (8, 8, 8)), (2, 0, (6, 5, 5)), (2, 0, (4, 4, 4)), (2, 0, (3, 3, 2))]


def sizes(png):
    rows = []
    h, w = png.shape
    d_in = torch.from_numpy(png.reshape(-1).view(np.int32)).cuda()
    for a, b, bits in SETS:
        with csic.Plan(csic.make_c_params(w, h, a, b, *bits, 1, CSQ, out_format=N.FMT_PLANAR_BITS), 0) as pl:
            src = pl.process_device(d_in, torch.zeros(pl.frame_bytes, dtype=torch.uint8, device="cuda:0"))
            g, gs = pl.pack_device(src)
            r, rs = pl.rice_pack_device(src)
            assert torch.equal(pl.unpack_device(g), src) and torch.equal(pl.rice_unpack_device(r), src)
            st = pl.code_stats(src, N.FMT_PLANAR_BITS)
            rows.append({"table": "sizes", "chroma": f"4:{a}:{b}", "bits": list(bits), "raw": int(pl.planar_bits_layout.payload_bytes),
                         "groups": int(gs[0]), "rice": int(rs[0]), "ideal_order0": int(st.ideal_bytes(0)), "ideal_left": int(st.ideal_bytes(1)),
                         "ideal_best": int(st.ideal_bytes("best"))})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def times(content, tile, bits=(6, 5, 5)):
    L = N.lib()
    rows = []
    with csic.Plan(csic.make_c_params(W, H, 2, 0, *bits, 1, CSQ, out_format=N.FMT_PLANAR_BITS), 0) as pl:
        lay = pl.planar_bits_layout
        fb, payload = lay.frame_bytes, lay.payload_bytes
        gbound, rbound = pl.pack_layout.bound_bytes, pl.rice_layout.bound_bytes
        rot = max(5, -(-RING_BYTES // fb))
        src = [pl.process_device(input_frame(content, k, tile), torch.zeros(fb, dtype=torch.uint8, device="cuda:0")) for k in range(rot)]
        gcoded = [torch.empty(gbound, dtype=torch.uint8, device="cuda:0") for _ in range(rot)]
        rcoded = [torch.empty(rbound, dtype=torch.uint8, device="cuda:0") for _ in range(rot)]
        back = [torch.zeros(fb, dtype=torch.uint8, device="cuda:0") for _ in range(rot)]
        gsizes, rsizes = (torch.zeros(rot, dtype=torch.int64, device="cuda:0") for _ in range(2))
        wsb = max(pl.pack_workspace_bytes(1), pl.rice_workspace_bytes(1))
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
        stream = pl._stream()
        P = C.c_void_p

        def gpack(i):
            N.check(L.csic_pack_device(pl._h, P(src[i].data_ptr()), 1, P(gcoded[i].data_ptr()), P(gsizes.data_ptr() + 8 * i), P(ws.data_ptr()), wsb, stream))

        def gunpack(i):
            N.check(L.csic_unpack_device(pl._h, P(gcoded[i].data_ptr()), 1, P(back[i].data_ptr()), P(ws.data_ptr()), wsb, stream))

        def rpack(i):
            N.check(L.csic_rice_pack_device(pl._h, P(src[i].data_ptr()), 1, P(rcoded[i].data_ptr()), P(rsizes.data_ptr() + 8 * i), P(ws.data_ptr()), wsb, stream))

        def runpack(i):
            N.check(L.csic_rice_unpack_device(pl._h, P(rcoded[i].data_ptr()), 1, P(back[i].data_ptr()), stream))

        for pack, unpack in ((gpack, gunpack), (rpack, runpack)):     # lossless on every frame of the ring before anything is timed
            for b in back:
                b.zero_()
            for i in range(rot):
                pack(i)
                unpack(i)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(src, back)), "unpack(pack(x)) != x"
        coded = {"groups": float(gsizes.double().mean()), "rice": float(rsizes.double().mean())}
        t = timed_alternating({"groups pack": gpack, "rice pack": rpack, "groups unpack": gunpack, "rice unpack": runpack}, rot)
        for key, us in t.items():
            coding, what = key.split()
            rows.append({"table": "times", "shape": f"{W}x{H}", "bits": list(bits), "content": content, "coding": coding, "what": what,
                         "kernel": pl.pack_kernel_name if coding == "groups" else pl.rice_kernel_name, "ring": rot, "us": round(statistics.median(us), 1),
                         "us_min": round(min(us), 1), "us_max": round(max(us), 1), "payload_bytes": int(payload), "coded_bytes": round(coded[coding]),
                         "ratio": round(coded[coding] / payload, 4)})
            print(json.dumps(rows[-1]), flush=True)
    torch.cuda.empty_cache()
    return rows


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/rice_rates.py measures on a GPU: no HIP device visible")
    png = read_png(os.path.join(ROOT, "tests", "golden", "inputs", "in512.png"))
    tile = torch.from_numpy(png.view(np.int32)).cuda()
    srows = sizes(png)
    trows = times("noise", tile) + times("natural", tile)
    os.makedirs(os.path.dirname(PREFIX) or ".", exist_ok=True)
    with open(PREFIX + ".md", "w") as fh:
        fh.write("# The Rice coding next to the group coding (tools/rice_rates.py)\n\n"
                 "## Coded sizes of in512.png, factor 1, bytes (fraction of RAW)\n\n"
                 "`ideal` is `ideal_bytes` of the code statistics of the same frame: what an ideal zero-order coder of the left-predicted residuals "
                 "(`left`) or of the better of codes and residuals per plane (`best`) would need.\n\n"
                 "| chroma | bits | RAW | GROUPS | RICE | ideal left | ideal best |\n|---|---|---:|---:|---:|---:|---:|\n")
        for r in srows:
            frac = lambda k: f"{r[k]} ({r[k] / r['raw']:.3f})"
            fh.write(f"| {r['chroma']} | {'/'.join(map(str, r['bits']))} | {r['raw']} | {frac('groups')} | {frac('rice')} | {frac('ideal_left')} | {frac('ideal_best')} |\n")
        fh.write(f"\n## Pack and unpack on 8192 x 8192, 4:2:0, 6/5/5, factor 1\n\nOne MI355X, one run; a ring of PLANAR_BITS frames in separate buffers "
                 f"larger than the Infinity Cache; median of {REPS} windows of {CALLS} calls, the four operations interleaved window by window.\n\n"
                 "| content | coding | coded / raw | operation | us / frame (min - max) | RICE / GROUPS |\n|---|---|---:|---|---:|---:|\n")
        us = {(r["content"], r["coding"], r["what"]): r["us"] for r in trows}
        for r in trows:
            ratio = f"{r['us'] / us[(r['content'], 'groups', r['what'])]:.2f}" if r["coding"] == "rice" else ""
            fh.write(f"| {r['content']} | {r['coding']} `{r['kernel']}` | {r['ratio']:.3f} | {r['what']} | {r['us']:.1f} ({r['us_min']:.1f} - {r['us_max']:.1f}) | {ratio} |\n")


if __name__ == "__main__":
    main()
