"""csic_decode_* on the GPU (csic_decode.hip): a compressed frame back to width x height pixels, decode(r, c) = o(r / f, c / f).
Expected frames come from numpy -- the oracle's packed output indexed by (row // f, column // f) -- for the four sources
(PLANAR_BITS, PLANAR, packed YCbCr, packed ARGB) and both outputs, on random shapes, on the fast kernel's shapes, in batches, from
misaligned buffers, on the reference's goldens, at full size, under graph capture and through the host path; the sums of squared
differences between an input and its decode must equal csic_distortion_*; compress / decompress go through files.  Every
comparison is exact."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_png_rgb

pytestmark = pytest.mark.gpu

ORDERS = list(itertools.permutations((1, 2, 3)))
CSQ = (3, 1, 2)
MODES = [(4, 4), (2, 2), (2, 0), (1, 1), (4, 0), (1, 0)]
CANARY = -286331154                      # 0xEEEEEEEE as int32
BITS, PLANAR, YCC, ARGB = 3, 2, 1, 0
PAIRS = [(s, o) for s in (BITS, PLANAR, YCC, ARGB) for o in (ARGB, YCC) if (s, o) != (ARGB, YCC)]

with open(os.path.join(GOLDEN, "manifest.json")) as _fh:
    _GOLDENS = json.load(_fh)["goldens"]


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    assert csic_amd._native.lib().csic_device_count() >= 1
    return csic_amd


def _plan(csic, W, H, a, b, bits, f, op, rounding=0, fmt=0, avg=False):
    cp = csic.make_c_params(W, H, a, b, *bits, f, op, rounding=rounding, out_format=fmt,
                            sampling=csic.Sampling.AVG if avg else csic.Sampling.HOLD_DECIMATE)
    return csic.Plan(cp, 0)


def _op(orc, W, H, a, b, bits, f, op, rounding=0, fmt=0):
    return orc.OracleParams(width=W, height=H, chroma_a=a, chroma_b=b, y_bits=bits[0], cb_bits=bits[1], cr_bits=bits[2],
                            factor=f, op=op, rounding=rounding, out_format=fmt)


def _expected(oracle, W, H, a, b, bits, f, op, rounding, avg, argb, fmt):
    """The decode by its definition: the oracle's packed output in `fmt`, replicated."""
    o = oracle.process(_op(oracle, W, H, a, b, bits, f, op, rounding, fmt), argb, form="avg" if avg else "stream")
    Ho, Wo = -(-H // f), -(-W // f)
    return o.reshape(Ho, Wo)[np.arange(H)[:, None] // f, np.arange(W)[None, :] // f]


def _sources(csic, W, H, a, b, bits, f, op, rounding, avg, d_in, nframes=1):
    """{src_format: device tensor} -- each source produced by the forward path of the same parameters."""
    out = {}
    for fmt in (BITS, PLANAR, YCC, ARGB):
        with _plan(csic, W, H, a, b, bits, f, op, rounding, fmt, avg) as pl:
            out[fmt] = pl.process_device(d_in, nframes=nframes)
    return out


def _decode_checked(pl, src, s, o, W, H, nframes=1):
    """decode_device into a buffer with a canary tail; returns the frames as uint32 (nframes, H, W)."""
    import torch
    n = nframes * W * H
    buf = torch.full((n + 64,), CANARY, dtype=torch.int32, device="cuda:0")
    pl.decode_device(src, s, buf[:n], nframes=nframes, out_format=o)
    host = buf.cpu().numpy()
    assert (host[n:] == CANARY).all(), "the canary behind the output was overwritten"
    return host[:n].view(np.uint32).reshape(nframes, H, W)


def _check_all_pairs(csic, oracle, W, H, a, b, bits, f, op, rounding, avg, argb, variants=(0, 9)):
    import torch
    N = csic._native
    d_in = torch.from_numpy(argb.view(np.int32)).cuda()
    srcs = _sources(csic, W, H, a, b, bits, f, op, rounding, avg, d_in)
    want = {o: _expected(oracle, W, H, a, b, bits, f, op, rounding, avg, argb, o) for o in (ARGB, YCC)}
    names = set()
    with _plan(csic, W, H, a, b, bits, f, op, rounding, ARGB, avg) as pl:
        for variant in variants:
            pl.tune(N.TUNE_VARIANT, variant)
            for s, o in PAIRS:
                name = pl.decode_kernel_name(s, o)
                names.add(name.split("<")[0] + ("*" if variant == 9 else ""))
                got = _decode_checked(pl, srcs[s], s, o, W, H)[0]
                assert np.array_equal(got, want[o]), (name, W, H, a, b, bits, f, op, rounding, avg, variant, s, o)
        assert pl.decode_kernel_name(ARGB, YCC) == ""
    return names


@pytest.mark.parametrize("seed", range(3))
def test_decode_random_shapes_vs_oracle(csic, oracle, seed):
    """W 1..96, H 1..40, every chroma mode, factor, order and rounding, independent bits per channel; four sources x two outputs minus
    the refused pair; the default kernels and the general one (variant 9)."""
    rng = np.random.default_rng(9100 + seed)
    seen = set()
    for _ in range(100):
        W, H = int(rng.integers(1, 97)), int(rng.integers(1, 41))
        a, b = MODES[int(rng.integers(0, 6))]
        bits = tuple(int(x) for x in rng.integers(1, 9, 3))
        f = int(rng.choice([1, 2, 4, 8]))
        op = ORDERS[int(rng.integers(0, 6))]
        rounding = int(rng.integers(0, 2))
        argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        seen |= _check_all_pairs(csic, oracle, W, H, a, b, bits, f, op, rounding, False, argb)
    assert {"k_decode_gen", "k_decode_gen*"} <= seen, seen


def test_decode_avg_random_shapes_vs_oracle(csic, oracle):
    rng = np.random.default_rng(9200)
    for _ in range(80):
        W, H = int(rng.integers(1, 97)), int(rng.integers(1, 41))
        a, b = MODES[int(rng.integers(0, 6))]
        bits = tuple(int(x) for x in rng.integers(1, 9, 3))
        f = int(rng.choice([1, 2, 4, 8]))
        argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        _check_all_pairs(csic, oracle, W, H, a, b, bits, f, CSQ, int(rng.integers(0, 2)), True, argb)


@pytest.mark.parametrize("W", [128, 256, 1024])
def test_decode_fast_kernel_shapes(csic, oracle, W):
    """Every chroma mode x factor x one order of each class on widths the fast kernel takes (any width that is a multiple of 4), at
    heights that leave a ragged last source row and a ragged last block; a width that is not falls to the general kernel."""
    rng = np.random.default_rng(9300 + W)
    seen = set()
    for (a, b), f, op in itertools.product(MODES, (1, 2, 4, 8), (CSQ, (1, 3, 2))):
        H = 5 if f == 1 else 3 * f + int(rng.integers(0, f))
        bits = tuple(int(x) for x in rng.integers(1, 9, 3))
        argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        seen |= _check_all_pairs(csic, oracle, W, H, a, b, bits, f, op, int(rng.integers(0, 2)), False, argb)
    assert "k_decode_gen" not in seen, seen
    for f in (2, 4, 8):                       # widths of 4 k pixels that are not multiples of the factor, and one that is no multiple of 4
        argb = rng.integers(0, 1 << 32, (W + 4) * 9, dtype=np.uint32)
        assert "k_decode" in _check_all_pairs(csic, oracle, W + 4, 9, 2, 0, (6, 5, 5), f, CSQ, 0, False, argb)
    argb = rng.integers(0, 1 << 32, (W + 2) * 9, dtype=np.uint32)
    seen |= _check_all_pairs(csic, oracle, W + 2, 9, 2, 0, (6, 5, 5), 2, CSQ, 0, False, argb)
    assert {"k_decode", "k_decode_gen", "k_decode_gen*", "k_rbits", "k_recon"} <= seen, seen


def test_decode_headline_shape_names_the_fast_kernel(csic):
    with _plan(csic, 8192, 8192, 2, 0, (6, 5, 5), 2, CSQ) as pl:
        for s in (BITS, PLANAR, YCC):
            for o in (ARGB, YCC):
                assert pl.decode_kernel_name(s, o).startswith("k_decode<"), (s, o, pl.decode_kernel_name(s, o))
        assert pl.decode_kernel_name(ARGB, ARGB).startswith("k_decode<")
    with _plan(csic, 8192, 8192, 2, 0, (6, 5, 5), 1, CSQ) as pl:
        assert pl.decode_kernel_name(BITS).startswith("k_rbits<") and pl.decode_kernel_name(PLANAR).startswith("k_recon<")
        assert pl.decode_kernel_name(YCC).startswith("k_decode<")


@pytest.mark.parametrize("f", [1, 2])
def test_decode_batches_of_odd_frames(csic, oracle, f):
    """nframes = 3 on 201 x 27, order spatial, chroma, quant: W * H is odd, so frames 1 and 2 start at addresses that are only
    4-byte aligned -- in the output always, in the packed sources at factor 1."""
    import torch
    W, H, a, b, bits, op, nf = 201, 27, 2, 0, (5, 7, 3), (1, 3, 2), 3
    argb = oracle.synth_frame(nf * W * H, 23)
    d_in = torch.from_numpy(argb.view(np.int32)).cuda()
    srcs = _sources(csic, W, H, a, b, bits, f, op, 0, False, d_in, nframes=nf)
    with _plan(csic, W, H, a, b, bits, f, op) as pl:
        for s, o in PAIRS:
            got = _decode_checked(pl, srcs[s], s, o, W, H, nframes=nf)
            for k in range(nf):
                want = _expected(oracle, W, H, a, b, bits, f, op, 0, False, argb[k * W * H:(k + 1) * W * H], o)
                assert np.array_equal(got[k], want), (f, s, o, k)


def test_decode_batches_on_the_fast_kernel(csic, oracle):
    import torch
    W, H, a, b, bits, f, nf = 256, 12, 2, 0, (6, 5, 5), 4, 5
    argb = oracle.synth_frame(nf * W * H, 29)
    d_in = torch.from_numpy(argb.view(np.int32)).cuda()
    srcs = _sources(csic, W, H, a, b, bits, f, CSQ, 0, False, d_in, nframes=nf)
    with _plan(csic, W, H, a, b, bits, f, CSQ) as pl:
        for s, o in PAIRS:
            assert pl.decode_kernel_name(s, o).startswith("k_decode<")
            got = _decode_checked(pl, srcs[s], s, o, W, H, nframes=nf)
            for k in range(nf):
                want = _expected(oracle, W, H, a, b, bits, f, CSQ, 0, False, argb[k * W * H:(k + 1) * W * H], o)
                assert np.array_equal(got[k], want), (s, o, k)


def test_decode_misaligned_buffers(csic, oracle):
    """A packed source and an output that are only 4-byte aligned: correct result, through the 4-byte kernel."""
    import torch
    rng = np.random.default_rng(9400)
    for (W, H, f) in ((256, 8, 2), (128, 6, 1), (77, 13, 4)):
        a, b, bits = 2, 0, (6, 5, 5)
        argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        d_in = torch.from_numpy(argb.view(np.int32)).cuda()
        srcs = _sources(csic, W, H, a, b, bits, f, CSQ, 0, False, d_in)
        with _plan(csic, W, H, a, b, bits, f, CSQ) as pl:
            for s, o in ((YCC, ARGB), (YCC, YCC), (ARGB, ARGB)):
                want = _expected(oracle, W, H, a, b, bits, f, CSQ, 0, False, argb, o)
                n_src = srcs[s].numel()
                shifted = torch.full((n_src + 1,), CANARY, dtype=torch.int32, device="cuda:0")
                shifted[1:] = srcs[s].reshape(-1).view(torch.int32)
                for src_off, out_off in ((1, 0), (0, 1), (1, 1)):
                    src = shifted[1:] if src_off else srcs[s].reshape(-1)
                    assert src.data_ptr() % 16 == (4 if src_off else 0)
                    buf = torch.full((W * H + 65,), CANARY, dtype=torch.int32, device="cuda:0")
                    out = buf[out_off:out_off + W * H]
                    pl.decode_device(src, s, out, out_format=o)
                    host = buf.cpu().numpy()
                    assert np.array_equal(host[out_off:out_off + W * H].view(np.uint32).reshape(H, W), want), (W, H, f, s, o, src_off, out_off)
                    assert (host[:out_off] == CANARY).all() and (host[out_off + W * H:] == CANARY).all()
            # a planar source must be 256-byte aligned, whatever the output's alignment
            lay = pl.planar_bits_layout
            raw = torch.zeros(lay.frame_bytes + 256, dtype=torch.uint8, device="cuda:0")
            out = torch.empty(W * H, dtype=torch.int32, device="cuda:0")
            N = csic._native
            st = N.lib().csic_decode_device(pl._h, C.c_void_p(raw.data_ptr() + 16), BITS, C.c_void_p(out.data_ptr()), ARGB, 1, None)
            assert st == N.EINVAL_SIZE


@pytest.mark.parametrize("e", _GOLDENS, ids=[g["name"] for g in _GOLDENS])
def test_decode_reproduces_the_goldens(csic, oracle, input_images, e):
    """decode(bits(input PNG)) equals the golden PNG replicated by its factor and cropped to the input size -- at factor 1 the golden
    itself.  model_copy_16 (rounding IDENTITY) is the reference's readImage -> writeImage round trip: no parameter set produces it,
    so there the input is compressed at 4:4:4, 8/8/8, factor 1 and the decode must equal the plain reconstruct of the same bits."""
    import torch
    N = csic._native
    rgb = input_images[e["input"]]
    h, w = rgb.shape[:2]
    f = e["factor"]
    rounding = 1 if e["rounding"] == "TRUNC_SW" else 0
    d_in = torch.from_numpy(oracle.rgb_to_argb(rgb).view(np.int32)).cuda()
    with _plan(csic, w, h, e["chroma_a"], e["chroma_b"], tuple(e["bits"]), f, tuple(e["op"]), rounding, BITS) as pl:
        bits = pl.process_device(d_in)
        if e["rounding"] == "IDENTITY":
            want = oracle.argb_to_rgb(pl.reconstruct_bits_device(bits).cpu().numpy().view(np.uint32))
        else:
            golden = load_png_rgb(os.path.join(GOLDEN, e["file"]))
            want = golden[np.arange(h)[:, None] // f, np.arange(w)[None, :] // f]
        assert want.shape == (h, w, 3)
        for variant in (0, 9):
            pl.tune(N.TUNE_VARIANT, variant)
            got = oracle.argb_to_rgb(_decode_checked(pl, bits, BITS, ARGB, w, h)[0])
            assert np.array_equal(got, want), (e["name"], variant)


# ---- closing the loop: SSE(x, decode(compress(x))) == distortion(x) -------------------------------------------------------------
def _div256(x, trunc):
    return np.where(x < 0, -((-x) // 256), x // 256) if trunc else x // 256


def forward(argb, rounding):
    """(Y, Cb, Cr) int64 arrays of ARGB pixels: RGB2YCbCr under `rounding` (0 floor, 1 trunc); as in tests/test_distortion_host.py."""
    a = np.asarray(argb, dtype=np.uint32).astype(np.int64)
    r, g, b = (a >> 16) & 255, (a >> 8) & 255, a & 255
    t = rounding == 1
    y = np.clip(_div256(77 * r + 150 * g + 29 * b + 128, t), 0, 255)
    cb = np.clip(_div256(-43 * r - 85 * g + 128 * b + 128, t) + 128, 0, 255)
    cr = np.clip(_div256(128 * r - 107 * g - 21 * b + 128, t) + 128, 0, 255)
    return y, cb, cr


def _bytes3(px):
    a = np.asarray(px, dtype=np.uint32).astype(np.int64)
    return (a >> 16) & 255, (a >> 8) & 255, a & 255          # R, G, B of an ARGB pixel; Cr, Cb, Y of a YCbCr pixel


def test_decode_closes_the_loop_with_distortion(csic):
    """No oracle here: the decoded frames themselves, compared in numpy with the input, must give the six sums the fused distortion
    kernel reports for the same parameters."""
    import torch
    rng = np.random.default_rng(9500)
    for k in range(50):
        W, H = int(rng.integers(1, 97)), int(rng.integers(1, 41))
        if k % 5 == 0:
            f = int(rng.choice([2, 4]))
            W = 4 * int(rng.integers(1, 25))                                         # the fast kernel's shapes
        else:
            f = int(rng.choice([1, 2, 4, 8]))
        a, b = MODES[int(rng.integers(0, 6))]
        bits = tuple(int(x) for x in rng.integers(1, 9, 3))
        avg = k % 4 == 3
        op = CSQ if avg else ORDERS[int(rng.integers(0, 6))]
        rounding = int(rng.integers(0, 2))
        frame = rng.integers(0, 1 << 32, (H, W), dtype=np.uint32)
        d_in = torch.from_numpy(frame.view(np.int32)).cuda()
        with _plan(csic, W, H, a, b, bits, f, op, rounding, BITS, avg) as pl:
            buf = pl.process_device(d_in)
            d_rgb = _decode_checked(pl, buf, BITS, ARGB, W, H)[0]
            d_ycc = _decode_checked(pl, buf, BITS, YCC, W, H)[0]
            dist = pl.distortion(d_in.reshape(H, W))
        sums = [int(((x - y) ** 2).sum()) for x, y in zip(_bytes3(frame), _bytes3(d_rgb))]
        dcr, dcb, dy = _bytes3(d_ycc)
        sums += [int(((x - y) ** 2).sum()) for x, y in zip(forward(frame, rounding), (dy, dcb, dcr))]
        assert tuple(sums) == dist.sse, (W, H, a, b, bits, f, op, rounding, avg)


def test_decode_full_size_equals_the_replicated_reconstruct(csic):
    """8192 x 8192, BASELINE cfg 4 (4:2:0, factor 2, chroma, spatial, quant) at 6/5/5, from bits, from planar and from the packed
    YCbCr stream: equal to reconstruct_bits_device's output repeated along both axes."""
    import torch
    N = csic._native
    W = H = 8192
    sh = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_in = torch.empty(W * H, dtype=torch.int32, device="cuda:0")
    N.check(N.lib().csic_synth_frame_device(C.c_void_p(d_in.data_ptr()), d_in.numel(), 0, 20250629, sh))
    with _plan(csic, W, H, 2, 0, (6, 5, 5), 2, CSQ, 0, BITS) as pl, _plan(csic, W, H, 2, 0, (6, 5, 5), 2, CSQ, 0, PLANAR) as pp, \
            _plan(csic, W, H, 2, 0, (6, 5, 5), 2, CSQ, 0, YCC) as py:
        bits = pl.process_device(d_in)
        for o in (ARGB, YCC):
            small = pl.reconstruct_bits_device(bits, out_format=o)
            want = small.repeat_interleave(2, dim=0).repeat_interleave(2, dim=1)
            assert want.shape == (H, W)
            assert pl.decode_kernel_name(BITS, o).startswith("k_decode<")
            got = pl.decode_device(bits, out_format=o)
            assert torch.equal(got, want), ("bits", o)
            del got
            got = pl.decode_device(pp.process_device(d_in), PLANAR, out_format=o)
            assert torch.equal(got, want), ("planar", o)
            del got
            got = pl.decode_device(py.process_device(d_in), YCC, out_format=o)
            assert torch.equal(got, want), ("ycc", o)
            del got, want, small


def test_decode_graph_capture_and_replay(csic, oracle):
    import torch
    W, H, a, b, bits, f = 512, 16, 2, 0, (6, 5, 5), 2
    rng = np.random.default_rng(9600)
    frames = [rng.integers(0, 1 << 32, W * H, dtype=np.uint32) for _ in range(2)]
    with _plan(csic, W, H, a, b, bits, f, CSQ, 0, BITS) as pl:
        d_in = torch.from_numpy(frames[0].view(np.int32)).cuda()
        d_bits = pl.process_device(d_in)
        d_out = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            pl.decode_device(d_bits, d_out=d_out)             # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            pl.process_device(d_in, d_bits)
            pl.decode_device(d_bits, d_out=d_out)
        for fr in frames[::-1]:
            d_in.copy_(torch.from_numpy(fr.view(np.int32)))
            d_out.zero_()
            g.replay()
            torch.cuda.synchronize()
            want = _expected(oracle, W, H, a, b, bits, f, CSQ, 0, False, fr, ARGB)
            assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want)


def test_decode_host_path(csic, oracle):
    rng = np.random.default_rng(9700)
    for (W, H, a, b, bits, f, op, avg, nf) in ((96, 30, 2, 0, (6, 5, 5), 2, CSQ, False, 1), (201, 27, 1, 1, (3, 3, 2), 1, (1, 3, 2), False, 2),
                                                 (256, 16, 2, 2, (5, 4, 3), 4, CSQ, True, 3)):
        argb = rng.integers(0, 1 << 32, nf * W * H, dtype=np.uint32)
        with _plan(csic, W, H, a, b, bits, f, op, 0, BITS, avg) as pl, _plan(csic, W, H, a, b, bits, f, op, 0, YCC, avg) as py:
            import torch
            d_in = torch.from_numpy(argb.view(np.int32)).cuda()
            h_bits = pl.process_device(d_in, nframes=nf).cpu().numpy()
            h_ycc = py.process_device(d_in, nframes=nf).cpu().numpy()
            for o in (ARGB, YCC):
                want = np.stack([_expected(oracle, W, H, a, b, bits, f, op, 0, avg, argb[k * W * H:(k + 1) * W * H], o) for k in range(nf)])
                got = pl.decode_host(h_bits, nframes=nf, out_format=o).reshape(nf, H, W)
                assert got.dtype == np.uint32 and np.array_equal(got, want), (W, H, o)
                got = pl.decode_host(h_ycc, YCC, nframes=nf, out_format=o).reshape(nf, H, W)
                assert np.array_equal(got, want), (W, H, o, "ycc")
            # sizes that do not match the plan
            N = csic._native
            with pytest.raises(csic.IllegalArgumentException) as ei:
                pl.decode_host(h_bits.reshape(-1)[:-1], nframes=nf)
            assert ei.value.status == N.EINVAL_SIZE
    top = csic.ImageCompressorTop(96, 30, 2, 0, 6, 5, 5, 2, *[csic.ProcessingStep(x) for x in CSQ])
    frame = rng.integers(0, 1 << 32, (30, 96), dtype=np.uint32)
    got = top.decode(top.processPlanarBits(frame))
    assert np.array_equal(got, _expected(oracle, 96, 30, 2, 0, (6, 5, 5), 2, CSQ, 0, False, frame.reshape(-1), ARGB))
    top.close()


def test_decode_refusals(csic):
    import torch
    N = csic._native
    lib = N.lib()
    W, H = 64, 8
    with _plan(csic, W, H, 2, 0, (6, 5, 5), 2, CSQ, 0, BITS) as pl:
        lay = pl.planar_bits_layout
        src = torch.zeros(lay.frame_bytes, dtype=torch.uint8, device="cuda:0")
        packed = torch.zeros(pl.out_width * pl.out_height, dtype=torch.int32, device="cuda:0")
        out = torch.zeros(W * H, dtype=torch.int32, device="cuda:0")
        ps, pp, po = C.c_void_p(src.data_ptr()), C.c_void_p(packed.data_ptr()), C.c_void_p(out.data_ptr())
        assert lib.csic_decode_device(None, ps, BITS, po, ARGB, 1, None) == N.EINVAL_NULL
        assert lib.csic_decode_device(pl._h, None, BITS, po, ARGB, 1, None) == N.EINVAL_NULL
        assert lib.csic_decode_device(pl._h, ps, BITS, None, ARGB, 1, None) == N.EINVAL_NULL
        for nf in (0, -3):
            assert lib.csic_decode_device(pl._h, ps, BITS, po, ARGB, nf, None) == N.EINVAL_SIZE
        assert lib.csic_decode_device(pl._h, pp, ARGB, po, YCC, 1, None) == N.EINVAL_FORMAT
        assert "inverse" in lib.csic_last_error().decode()
        for bad in (4, -1):
            assert lib.csic_decode_device(pl._h, ps, bad, po, ARGB, 1, None) == N.EINVAL_FORMAT
        for bad in (PLANAR, BITS, 7):
            assert lib.csic_decode_device(pl._h, ps, BITS, po, bad, 1, None) == N.EINVAL_FORMAT
        for s in (BITS, PLANAR):
            assert lib.csic_decode_device(pl._h, C.c_void_p(src.data_ptr() + 128), s, po, ARGB, 1, None) == N.EINVAL_SIZE
        assert lib.csic_decode_device(pl._h, C.c_void_p(packed.data_ptr() + 2), YCC, po, ARGB, 1, None) == N.EINVAL_SIZE
        assert lib.csic_decode_device(pl._h, pp, YCC, C.c_void_p(out.data_ptr() + 2), ARGB, 1, None) == N.EINVAL_SIZE
        assert lib.csic_decode_device(pl._h, ps, BITS, po, ARGB, 1, None) == N.OK
        torch.cuda.synchronize()
        hs, ho = np.zeros(lay.frame_bytes, dtype=np.uint8), np.zeros(W * H, dtype=np.uint32)
        phs, pho = hs.ctypes.data_as(C.c_void_p), ho.ctypes.data_as(C.c_void_p)
        assert lib.csic_decode_host(None, phs, hs.size, BITS, pho, ho.size, ARGB, 1) == N.EINVAL_NULL
        assert lib.csic_decode_host(pl._h, None, hs.size, BITS, pho, ho.size, ARGB, 1) == N.EINVAL_NULL
        assert lib.csic_decode_host(pl._h, phs, hs.size, BITS, None, ho.size, ARGB, 1) == N.EINVAL_NULL
        assert lib.csic_decode_host(pl._h, phs, hs.size, BITS, pho, ho.size, ARGB, 0) == N.EINVAL_SIZE
        assert lib.csic_decode_host(pl._h, phs, hs.size - 1, BITS, pho, ho.size, ARGB, 1) == N.EINVAL_SIZE
        assert lib.csic_decode_host(pl._h, phs, hs.size, BITS, pho, ho.size + 1, ARGB, 1) == N.EINVAL_SIZE
        assert lib.csic_decode_host(pl._h, phs, hs.size, ARGB, pho, ho.size, YCC, 1) == N.EINVAL_FORMAT
        # the Python layer
        with pytest.raises(csic.IllegalArgumentException):
            pl.decode_device(src[:-1])
        with pytest.raises(csic.IllegalArgumentException):
            pl.decode_device(src, d_out=out[:-1])
        with pytest.raises(csic.IllegalArgumentException) as ei:
            pl.decode_device(packed, ARGB, out_format=YCC)
        assert ei.value.status == N.EINVAL_FORMAT


def test_decode_tuning_knobs(csic, oracle):
    """NO_VECTOR and FORCE_GENERIC select the general kernel; NONTEMPORAL 0 and every BLOCK_THREADS give the same pixels."""
    import torch
    N = csic._native
    W, H, a, b, bits, f = 256, 8, 2, 0, (6, 5, 5), 2
    argb = np.random.default_rng(9800).integers(0, 1 << 32, W * H, dtype=np.uint32)
    d_in = torch.from_numpy(argb.view(np.int32)).cuda()
    srcs = _sources(csic, W, H, a, b, bits, f, CSQ, 0, False, d_in)
    want = _expected(oracle, W, H, a, b, bits, f, CSQ, 0, False, argb, ARGB)
    for knob, value, family in ((N.TUNE_NO_VECTOR, 1, "k_decode_gen<"), (N.TUNE_FORCE_GENERIC, 1, "k_decode_gen<"), (N.TUNE_NONTEMPORAL, 0, "k_decode<"),
                                (N.TUNE_BLOCK_THREADS, 64, "k_decode<"), (N.TUNE_BLOCK_THREADS, 128, "k_decode<"), (N.TUNE_BLOCK_THREADS, 256, "k_decode<")):
        with _plan(csic, W, H, a, b, bits, f, CSQ) as pl:
            pl.tune(knob, value)
            for s in (BITS, PLANAR, YCC):
                name = pl.decode_kernel_name(s, ARGB)
                assert name.startswith(family), (knob, value, name)
                if family == "k_decode<":
                    assert ("cached" in name) == (knob == N.TUNE_NONTEMPORAL), name
                assert np.array_equal(_decode_checked(pl, srcs[s], s, ARGB, W, H)[0], want), (knob, value, s)


def test_compress_and_decompress_files(csic, oracle, input_images, tmp_path):
    """main(["compress", ...]) on in512.png at 4:2:0, 6/5/5, factor 2 writes exactly 80 + payload_bytes bytes -- fewer than the input
    PNG -- and main(["decompress", ...]) a 512 x 512 PNG equal to the numpy expectation."""
    from csic_amd.app import main
    src = os.path.join(GOLDEN, "inputs", "in512.png")
    packed, back = str(tmp_path / "in512.csic"), str(tmp_path / "back" / "in512.png")
    assert main(["compress", "--input", src, "--output", packed, "--a", "2", "--b", "0", "--yq", "6", "--cbq", "5", "--crq", "5", "--sf", "2",
                 "--op1", "chroma", "--op2", "spatial", "--op3", "color"]) == 0
    info = csic.container_info(packed)
    cp = info.params
    assert (cp.width, cp.height, cp.chroma_a, cp.chroma_b, cp.y_bits, cp.cb_bits, cp.cr_bits, cp.factor, tuple(cp.op)) == \
        (512, 512, 2, 0, 6, 5, 5, 2, CSQ)
    lay = csic._native.CsicPlanarBitsLayout()
    csic._native.check(csic._native.lib().csic_planar_bits_layout_of(C.byref(cp), C.byref(lay)))
    assert os.path.getsize(packed) == 80 + lay.payload_bytes == info.file_bytes
    assert os.path.getsize(packed) < os.path.getsize(src)
    assert main(["decompress", "--input", packed, "--output", back]) == 0
    got = load_png_rgb(back)
    rgb = input_images["in512"]
    want = _expected(oracle, 512, 512, 2, 0, (6, 5, 5), 2, CSQ, 0, False, oracle.rgb_to_argb(rgb).reshape(-1), ARGB)
    assert got.shape == (512, 512, 3) and np.array_equal(got, oracle.argb_to_rgb(want))
    # the API under the verbs, with the AVG extension
    size = csic.ImageCompressionApp.compressImage(src, str(tmp_path / "avg.csic"), 2, 0, 6, 5, 5, 4, *[csic.ProcessingStep(x) for x in CSQ],
                                                  sampling=csic.Sampling.AVG)
    assert size == os.path.getsize(tmp_path / "avg.csic")
    csic.ImageCompressionApp.decompressImage(str(tmp_path / "avg.csic"), str(tmp_path / "avg.png"))
    want = _expected(oracle, 512, 512, 2, 0, (6, 5, 5), 4, CSQ, 0, True, oracle.rgb_to_argb(rgb).reshape(-1), ARGB)
    assert np.array_equal(load_png_rgb(str(tmp_path / "avg.png")), oracle.argb_to_rgb(want))
    # a missing input is reported, not raised; anything but a verb in front leaves the verb-less CLI in charge
    assert main(["decompress", "--input", str(tmp_path / "none.csic"), "--output", back]) == 1
