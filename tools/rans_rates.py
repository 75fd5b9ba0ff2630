#!/usr/bin/env python3
"""tools/rans_rates.py [OUT_PREFIX] -- what the rANS coding saves and what it costs next to the Rice coding, on one MI355X.
Writes OUT_PREFIX.md (default profiles/r21_rans_rates); the JSON lines behind it go to stdout.

1. Sizes: tests/golden/inputs/in512.png at the README's four parameter sets (factor 1, order chroma, spatial, quant) compressed on the
   device, then coded by csic_pack_device, csic_rice_pack_device and csic_rans_pack_device: RAW / GROUPS / RICE / RANS bytes beside the
   ideal_bytes of the code statistics of the same frame, and how many blocks went out raw.  Each coded frame is unpacked and compared.
2. Times: 8192 x 8192, 4:2:0, factor 1 at 8/8/8, 6/5/5 and 3/3/2, on noise and on in512.png tiled 16 x 16 and rolled per frame -- rANS
   pack and unpack, Rice pack and unpack and csic_copy_device of the payload in the same run, window by window in turn, with the method
   of tools/pack_rates.py: a ring of PLANAR_BITS frames in separate buffers larger than the Infinity Cache, windows of CALLS calls
   between two device events, the median of REPS window means with min and max, unpack(pack(x)) == x on every frame of the ring first.
3. Sequences: the 16-frame 3840 x 2160 sequences of tools/delta_rates.py at 6/5/5 through csic_delta_device (gop 16), the difference
   frames coded by both coders: bytes of delta + rANS against delta + Rice."""
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
import delta_rates  # noqa: E402
from pack_rates import CSQ, H, W, RING_BYTES, input_frame, read_png, timed_alternating, REPS, CALLS  # noqa: E402

N = csic._native
PREFIX = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r21_rans_rates")
SETS = [(4, 4, (8, 8, 8)), (2, 0, (6, 5, 5)), (2, 0, (4, 4, 4)), (2, 0, (3, 3, 2))]


def raw_blocks(pl, coded):
    rl = pl.rans_layout
    d = coded.reshape(-1)[rl.directory_offset:rl.directory_offset + 4 * sum(rl.blocks)].cpu().numpy().view("<u4")
    return int(np.count_nonzero(d >> 31)), int(sum(rl.blocks))


def sizes(png):
    rows = []
    h, w = png.shape
    d_in = torch.from_numpy(png.reshape(-1).view(np.int32)).cuda()
    for a, b, bits in SETS:
        with csic.Plan(csic.make_c_params(w, h, a, b, *bits, 1, CSQ, out_format=N.FMT_PLANAR_BITS), 0) as pl:
            src = pl.process_device(d_in, torch.zeros(pl.frame_bytes, dtype=torch.uint8, device="cuda:0"))
            g, gs = pl.pack_device(src)
            r, rs = pl.rice_pack_device(src)
            x, xs = pl.rans_pack_device(src)
            assert torch.equal(pl.unpack_device(g), src) and torch.equal(pl.rice_unpack_device(r), src) and torch.equal(pl.rans_unpack_device(x), src)
            st = pl.code_stats(src, N.FMT_PLANAR_BITS)
            raw, nb = raw_blocks(pl, x)
            rows.append({"table": "sizes", "chroma": f"4:{a}:{b}", "bits": list(bits), "raw": int(pl.planar_bits_layout.payload_bytes),
                         "groups": int(gs[0]), "rice": int(rs[0]), "rans": int(xs[0]), "raw_blocks": raw, "blocks": nb,
                         "ideal_left": int(st.ideal_bytes(1)), "ideal_best": int(st.ideal_bytes("best"))})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def times(content, tile, bits):
    L = N.lib()
    rows = []
    with csic.Plan(csic.make_c_params(W, H, 2, 0, *bits, 1, CSQ, out_format=N.FMT_PLANAR_BITS), 0) as pl:
        lay = pl.planar_bits_layout
        fb, payload = lay.frame_bytes, lay.payload_bytes
        rbound, xbound = pl.rice_layout.bound_bytes, pl.rans_layout.bound_bytes
        rot = max(5, -(-RING_BYTES // fb))
        src = [pl.process_device(input_frame(content, k, tile), torch.zeros(fb, dtype=torch.uint8, device="cuda:0")) for k in range(rot)]
        rcoded = [torch.empty(rbound, dtype=torch.uint8, device="cuda:0") for _ in range(rot)]
        xcoded = [torch.empty(xbound, dtype=torch.uint8, device="cuda:0") for _ in range(rot)]
        back = [torch.zeros(fb, dtype=torch.uint8, device="cuda:0") for _ in range(rot)]
        rsizes, xsizes = (torch.zeros(rot, dtype=torch.int64, device="cuda:0") for _ in range(2))
        wsb = max(pl.rice_workspace_bytes(1), pl.rans_workspace_bytes(1))
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
        copy_px = payload // 4
        copy_dst = torch.empty(4 * copy_px, dtype=torch.uint8, device="cuda:0")
        stream = pl._stream()
        P = C.c_void_p

        def rpack(i):
            N.check(L.csic_rice_pack_device(pl._h, P(src[i].data_ptr()), 1, P(rcoded[i].data_ptr()), P(rsizes.data_ptr() + 8 * i), P(ws.data_ptr()), wsb, stream))

        def runpack(i):
            N.check(L.csic_rice_unpack_device(pl._h, P(rcoded[i].data_ptr()), 1, P(back[i].data_ptr()), stream))

        def xpack(i):
            N.check(L.csic_rans_pack_device(pl._h, P(src[i].data_ptr()), 1, P(xcoded[i].data_ptr()), P(xsizes.data_ptr() + 8 * i), P(ws.data_ptr()), wsb, stream))

        def xunpack(i):
            N.check(L.csic_rans_unpack_device(pl._h, P(xcoded[i].data_ptr()), 1, P(back[i].data_ptr()), stream))

        def copy(i):
            N.check(L.csic_copy_device(P(copy_dst.data_ptr()), P(src[i].data_ptr()), copy_px, stream))

        for pack, unpack in ((rpack, runpack), (xpack, xunpack)):     # lossless on every frame of the ring before anything is timed
            for b in back:
                b.zero_()
            for i in range(rot):
                pack(i)
                unpack(i)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(src, back)), "unpack(pack(x)) != x"
        coded = {"rice": float(rsizes.double().mean()), "rans": float(xsizes.double().mean()), "copy": float(payload)}
        raw, nb = raw_blocks(pl, xcoded[0])
        t = timed_alternating({"rice pack": rpack, "rans pack": xpack, "rice unpack": runpack, "rans unpack": xunpack, "copy payload": copy}, rot)
        names = {"rice": pl.rice_kernel_name, "rans": pl.rans_kernel_name, "copy": "csic_copy_device"}
        for key, us in t.items():
            coding, what = key.split()
            rows.append({"table": "times", "shape": f"{W}x{H}", "bits": list(bits), "content": content, "coding": coding, "what": what,
                         "kernel": names[coding], "ring": rot, "us": round(statistics.median(us), 1), "us_min": round(min(us), 1),
                         "us_max": round(max(us), 1), "payload_bytes": int(payload), "coded_bytes": round(coded[coding]),
                         "ratio": round(coded[coding] / payload, 4), "raw_blocks": raw if coding == "rans" else None, "blocks": nb})
            print(json.dumps(rows[-1]), flush=True)
    torch.cuda.empty_cache()
    return rows


def sequences(tile):
    """delta + rANS against delta + Rice on the sequences of tools/delta_rates.py: bytes of 16 difference frames at gop 16."""
    rows = []
    w, h, bits, nf = delta_rates.W, delta_rates.H, delta_rates.BITS, delta_rates.NF
    with csic.Plan(csic.make_c_params(w, h, 2, 0, *bits, 1, CSQ, out_format=N.FMT_PLANAR_BITS), 0) as pl:
        for content in ("noise", "natural"):                  # noise: unrelated frames; natural: in512.png tiled, a 96 x 96 patch moves
            for seq in (0, 1):
                frames = torch.stack([pl.process_device(delta_rates.input_frame(content, seq, k, tile),
                                                        torch.zeros(pl.frame_bytes, dtype=torch.uint8, device="cuda:0")) for k in range(nf)])
                diff, _ = pl.delta_device(frames, nf, nf)
                _, rs = pl.rice_pack_device(diff, nf)
                x, xs = pl.rans_pack_device(diff, nf)
                lo = pl.rans_unpack_device(x, nf, torch.zeros_like(diff)).reshape(-1)       # only the payload ranges are written: the bytes that
                hi = pl.rans_unpack_device(x, nf, torch.full_like(diff, 255)).reshape(-1)   # come out the same over 0x00 and over 0xff
                wrote = lo == hi
                assert int(wrote.sum()) >= nf * pl.planar_bits_layout.payload_bytes * 0.99 and torch.equal(lo[wrote], diff.reshape(-1)[wrote])
                rows.append({"table": "sequences", "shape": f"{w}x{h}", "bits": list(bits), "content": content, "sequence": seq, "frames": nf,
                             "raw": int(nf * pl.planar_bits_layout.payload_bytes), "delta_rice": int(rs.sum()), "delta_rans": int(xs.sum())})
                print(json.dumps(rows[-1]), flush=True)
    torch.cuda.empty_cache()
    return rows


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/rans_rates.py measures on a GPU: no HIP device visible")
    png = read_png(os.path.join(ROOT, "tests", "golden", "inputs", "in512.png"))
    tile = torch.from_numpy(png.view(np.int32)).cuda()
    srows = sizes(png)
    trows = []
    for bits in ((8, 8, 8), (6, 5, 5), (3, 3, 2)):
        trows += times("noise", tile, bits) + times("natural", tile, bits)
    qrows = sequences(tile)
    os.makedirs(os.path.dirname(PREFIX) or ".", exist_ok=True)
    with open(PREFIX + ".md", "w") as fh:
        fh.write("# The rANS coding next to the Rice coding (tools/rans_rates.py)\n\n"
                 "## Coded sizes of in512.png, factor 1, bytes (fraction of RAW)\n\n"
                 "`ideal` is `ideal_bytes` of the code statistics of the same frame: what an ideal zero-order coder of the left-predicted residuals "
                 "(`left`) or of the better of codes and residuals per plane (`best`) would need.\n\n"
                 "| chroma | bits | RAW | GROUPS | RICE | RANS | RANS / RICE | raw blocks | ideal left | ideal best |\n|---|---|---:|---:|---:|---:|---:|---:|---:|---:|\n")
        for r in srows:
            frac = lambda k: f"{r[k]} ({r[k] / r['raw']:.3f})"
            fh.write(f"| {r['chroma']} | {'/'.join(map(str, r['bits']))} | {r['raw']} | {frac('groups')} | {frac('rice')} | {frac('rans')} | "
                     f"{r['rans'] / r['rice']:.3f} | {r['raw_blocks']} of {r['blocks']} | {frac('ideal_left')} | {frac('ideal_best')} |\n")
        fh.write(f"\n## Pack and unpack on 8192 x 8192, 4:2:0, factor 1\n\nOne MI355X, one run; a ring of PLANAR_BITS frames in separate buffers "
                 f"larger than the Infinity Cache; median of {REPS} windows of {CALLS} calls, the five operations interleaved window by window.  "
                 "A block of the rANS coding goes out raw wherever that is strictly smaller (`raw blocks`, of the frame the ring begins with).\n\n"
                 "| bits | content | coding | coded / raw | raw blocks | operation | us / frame (min - max) | RANS / RICE |\n|---|---|---|---:|---:|---|---:|---:|\n")
        us = {(tuple(r["bits"]), r["content"], r["coding"], r["what"]): r["us"] for r in trows}
        for r in trows:
            ratio = f"{r['us'] / us[(tuple(r['bits']), r['content'], 'rice', r['what'])]:.2f}" if r["coding"] == "rans" else ""
            blocks = f"{r['raw_blocks']} of {r['blocks']}" if r["coding"] == "rans" else ""
            fh.write(f"| {'/'.join(map(str, r['bits']))} | {r['content']} | {r['coding']} `{r['kernel']}` | {r['ratio']:.3f} | {blocks} | {r['what']} | "
                     f"{r['us']:.1f} ({r['us_min']:.1f} - {r['us_max']:.1f}) | {ratio} |\n")
        fh.write("\n## Difference frames of 16-frame 3840 x 2160 sequences at 6/5/5, gop 16 (csic_delta_device), bytes\n\n"
                 "| content | sequence | RAW | delta + RICE | delta + RANS | RANS / RICE |\n|---|---|---:|---:|---:|---:|\n")
        for r in qrows:
            fh.write(f"| {r['content']} | {r['sequence']} | {r['raw']} | {r['delta_rice']} | {r['delta_rans']} | {r['delta_rans'] / r['delta_rice']:.3f} |\n")


if __name__ == "__main__":
    main()
