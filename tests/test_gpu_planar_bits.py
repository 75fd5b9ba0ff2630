"""out_format = CSIC_FMT_PLANAR_BITS on the GPU (csic_planar_bits.hip): every plane byte for byte against the oracle's planar form
packed at the plan's bit widths, a canary in every byte the format does not own, csic_reconstruct_bits_device against the packed
oracle output, the reference's golden images through bits -> reconstruct, and the refusals.  Every comparison is exact."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_png_rgb
from plane_frames import pack_codes

pytestmark = pytest.mark.gpu

ORDERS = list(itertools.permutations((1, 2, 3)))
CSQ = (3, 1, 2)
MODES = [(4, 4), (2, 2), (2, 0), (1, 1), (4, 0), (1, 0)]
CANARY = 0xEE

with open(os.path.join(GOLDEN, "manifest.json")) as _fh:
    _GOLDENS = json.load(_fh)["goldens"]


def test_packer_matches_the_worked_vectors():
    assert pack_codes(np.array([1, 2, 3, 4, 5, 6, 7, 0]) << 5, 3).tobytes().hex() == "d1581f"
    assert pack_codes(np.array([0x1F, 0, 0x15]) << 3, 5).tobytes().hex() == "1f54"


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    assert csic_amd._native.lib().csic_device_count() >= 1
    return csic_amd


def _plan(csic, W, H, a, b, bits, f, op, rounding=0, fmt=3, avg=False):
    cp = csic.make_c_params(W, H, a, b, *bits, f, op, rounding=rounding, out_format=fmt,
                            sampling=csic.Sampling.AVG if avg else csic.Sampling.HOLD_DECIMATE)
    return csic.Plan(cp, 0)


def _op(orc, W, H, a, b, bits, f, op, rounding=0, fmt=0):
    return orc.OracleParams(width=W, height=H, chroma_a=a, chroma_b=b, y_bits=bits[0], cb_bits=bits[1], cr_bits=bits[2],
                            factor=f, op=op, rounding=rounding, out_format=fmt)


def _expected_frame(lay, y, cb, cr):
    """The whole frame buffer the format defines, with CANARY in every byte it does not own."""
    want = np.full(lay.frame_bytes, CANARY, dtype=np.uint8)
    for off, nb, vals, q in ((lay.y_offset, lay.y_bytes, y, lay.y_bits), (lay.cb_offset, lay.cb_bytes, cb, lay.cb_bits),
                             (lay.cr_offset, lay.cr_bytes, cr, lay.cr_bits)):
        p = pack_codes(vals, q)
        assert p.size == nb
        want[off:off + nb] = p
    return want


def _check_one(csic, oracle, W, H, a, b, bits, f, op, rounding, avg, argb, variants=(0, 9)):
    import torch
    N = csic._native
    form = "avg" if avg else "stream"
    _, y_o, cb_o, cr_o = oracle.planar(_op(oracle, W, H, a, b, bits, f, op, rounding), argb, avg=avg)
    want_argb = oracle.process(_op(oracle, W, H, a, b, bits, f, op, rounding, 0), argb, form=form)
    want_ycc = oracle.process(_op(oracle, W, H, a, b, bits, f, op, rounding, 1), argb, form=form)
    d_in = torch.from_numpy(argb.view(np.int32)).cuda()
    names = set()
    with _plan(csic, W, H, a, b, bits, f, op, rounding, avg=avg) as pl:
        lay = pl.planar_bits_layout
        want = _expected_frame(lay, y_o, cb_o, cr_o)
        for variant in variants:
            pl.tune(N.TUNE_VARIANT, variant)
            names.add(pl.kernel_name.split("<")[0] + ("*" if variant == 9 else ""))
            buf = torch.full((lay.frame_bytes,), CANARY, dtype=torch.uint8, device="cuda:0")
            pl.process_device(d_in, buf)
            host = buf.cpu().numpy()
            tag = (pl.kernel_name, W, H, a, b, bits, f, op, rounding, avg, variant)
            assert np.array_equal(host, want), tag
            y, cb, cr = pl.unpack_planar_bits(host)
            assert np.array_equal(y, y_o) and np.array_equal(cb, cb_o) and np.array_equal(cr, cr_o), tag
            for fmt, w in ((N.FMT_ARGB8888, want_argb), (N.FMT_YCBCR888X, want_ycc)):
                got = pl.reconstruct_bits_device(buf, out_format=fmt).cpu().numpy().view(np.uint32)
                assert np.array_equal(got, w), tag + (fmt,)
        pl.tune(N.TUNE_VARIANT, 0)
    return names


@pytest.mark.parametrize("seed", range(3))
def test_bits_random_shapes_vs_oracle(csic, oracle, seed):
    """W 1..96, H 1..40, every chroma mode, factor and order, both roundings, independent bits per channel, the default kernel and
    the general one (variant 9) on the same shapes."""
    rng = np.random.default_rng(7100 + seed)
    seen = set()
    for _ in range(100):
        W, H = int(rng.integers(1, 97)), int(rng.integers(1, 41))
        a, b = MODES[int(rng.integers(0, 6))]
        bits = tuple(int(x) for x in rng.integers(1, 9, 3))
        f = int(rng.choice([1, 2, 4, 8]))
        op = ORDERS[int(rng.integers(0, 6))]
        rounding = int(rng.integers(0, 2))
        argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        seen |= _check_one(csic, oracle, W, H, a, b, bits, f, op, rounding, False, argb)
    assert {"k_pbits_gen", "k_pbits_gen*"} <= seen, seen


def test_bits_avg_random_shapes_vs_oracle(csic, oracle):
    rng = np.random.default_rng(7200)
    for _ in range(80):
        W, H = int(rng.integers(1, 97)), int(rng.integers(1, 41))
        a, b = MODES[int(rng.integers(0, 6))]
        bits = tuple(int(x) for x in rng.integers(1, 9, 3))
        f = int(rng.choice([1, 2, 4, 8]))
        argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        _check_one(csic, oracle, W, H, a, b, bits, f, CSQ, int(rng.integers(0, 2)), True, argb)


@pytest.mark.parametrize("f", [1, 2, 4, 8])
def test_bits_fast_kernels_every_mode_and_bit_count(csic, oracle, f):
    """Shapes whose module width is a multiple of 128 (the fast kernels: k_pbits_f1 at factor 1, k_pbits_strided with the chroma
    stage before the decimator), every chroma mode, every bit count 1..8 on some channel, both orders classes, odd heights."""
    rng = np.random.default_rng(7300 + f)
    seen = set()
    shapes = [(128 * f, 5 * f + 1), (384 * f, 3 * f), (256 * f, 2 * f + 1)]
    for (W, H), (a, b) in itertools.product(shapes, MODES):
        argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        for k in range(3):
            bits = tuple(int(x) for x in rng.integers(1, 9, 3))
            op = (CSQ, (3, 2, 1), (1, 3, 2))[k]
            seen |= _check_one(csic, oracle, W, H, a, b, bits, f, op, int(rng.integers(0, 2)), False, argb)
    for q in range(1, 9):
        W, H = 128 * f, 4 * f
        argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        seen |= _check_one(csic, oracle, W, H, 2, 0, (q, q, 9 - q), f, CSQ, 0, False, argb)
    assert ("k_pbits_f1" if f == 1 else "k_pbits_strided") in seen and "k_pbits_gen*" in seen, seen


def test_bits_888_frame_is_the_planar_frame(csic, oracle):
    import torch
    rng = np.random.default_rng(7400)
    for (W, H, a, b, f, op, avg) in ((256, 17, 2, 0, 1, CSQ, False), (512, 8, 1, 0, 2, CSQ, False), (77, 13, 2, 2, 2, (1, 3, 2), False),
                                     (64, 16, 2, 0, 2, CSQ, True), (128, 9, 4, 4, 1, (2, 3, 1), False)):
        argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        d_in = torch.from_numpy(argb.view(np.int32)).cuda()
        with _plan(csic, W, H, a, b, (8, 8, 8), f, op, avg=avg) as pb, _plan(csic, W, H, a, b, (8, 8, 8), f, op, fmt=2, avg=avg) as pp:
            assert pb.planar_bits_layout.frame_bytes == pp.planar_layout.frame_bytes
            fb = pp.planar_layout.frame_bytes
            b1 = torch.full((fb,), CANARY, dtype=torch.uint8, device="cuda:0")
            b2 = torch.full((fb,), CANARY, dtype=torch.uint8, device="cuda:0")
            pb.process_device(d_in, b1)
            pp.process_device(d_in, b2)
            assert torch.equal(b1, b2), (W, H, a, b, f, op, avg, pb.kernel_name)


def test_bits_reproduce_the_goldens(csic, oracle, input_images):
    """Every golden except IDENTITY through bits -> reconstruct_bits: the quantiser goldens (6/5/5, 3/3/2, 8/4/4, 4/4/4, 1/1/1), the
    chroma goldens, app_420_q8_sf1_128 and the factor-2 goldens, default and general kernels."""
    import torch
    N = csic._native
    n = 0
    for e in _GOLDENS:
        if e["rounding"] == "IDENTITY":
            continue
        rgb = input_images[e["input"]]
        h, w = rgb.shape[:2]
        rounding = 1 if e["rounding"] == "TRUNC_SW" else 0
        want = load_png_rgb(os.path.join(GOLDEN, e["file"]))
        with _plan(csic, w, h, e["chroma_a"], e["chroma_b"], tuple(e["bits"]), e["factor"], tuple(e["op"]), rounding) as pl:
            d_in = torch.from_numpy(oracle.rgb_to_argb(rgb).view(np.int32)).cuda()
            for variant in (0, 9):
                pl.tune(N.TUNE_VARIANT, variant)
                buf = pl.process_device(d_in)
                got = oracle.argb_to_rgb(pl.reconstruct_bits_device(buf).cpu().numpy().view(np.uint32))
                assert np.array_equal(got, want), (e["name"], variant)
        n += 1
    assert n >= 25


def test_bits_batches_host_path_and_mid_byte_plane_ends(csic, oracle):
    """nframes 1..5 (frame k at k * frame_bytes) with bit counts that end planes mid-byte, and csic_process_host."""
    import torch
    W, H = 203, 27
    argb = oracle.synth_frame(5 * W * H, 11)
    d_in = torch.from_numpy(argb.view(np.int32)).cuda()
    for (a, b, bits, f, op, avg) in ((2, 0, (3, 3, 2), 1, CSQ, False), (2, 0, (5, 7, 3), 2, (1, 3, 2), False), (1, 1, (1, 5, 7), 2, CSQ, False),
                                     (2, 0, (6, 5, 5), 1, CSQ, True), (2, 2, (7, 3, 1), 4, CSQ, True)):
        with _plan(csic, W, H, a, b, bits, f, op, avg=avg) as pl:
            lay = pl.planar_bits_layout
            assert any((s * q) % 8 for s, q in ((lay.geometry.y_width * lay.geometry.y_height, bits[0]),
                                                (lay.geometry.chroma_samples, bits[1]), (lay.geometry.chroma_samples, bits[2])))
            for nf in range(1, 6):
                buf = torch.full((nf, lay.frame_bytes), CANARY, dtype=torch.uint8, device="cuda:0")
                pl.process_device(d_in[:nf * W * H], buf, nframes=nf)
                host = buf.cpu().numpy().reshape(nf, -1)
                out = pl.reconstruct_bits_device(buf, nframes=nf).cpu().numpy().view(np.uint32).reshape(nf, -1)
                for k in range(nf):
                    fr = argb[k * W * H:(k + 1) * W * H]
                    _, y_o, cb_o, cr_o = oracle.planar(_op(oracle, W, H, a, b, bits, f, op), fr, avg=avg)
                    assert np.array_equal(host[k], _expected_frame(lay, y_o, cb_o, cr_o)), (nf, k, a, b, bits, f, avg)
                    want = oracle.process(_op(oracle, W, H, a, b, bits, f, op), fr, form="avg" if avg else "stream")
                    assert np.array_equal(out[k], want.reshape(-1)), (nf, k, a, b, bits, f, avg)
            got = pl.process_host(argb[:W * H])
            assert got.dtype == np.uint8 and got.size == lay.frame_bytes
            y, cb, cr = pl.unpack_planar_bits(got)
            _, y_o, cb_o, cr_o = oracle.planar(_op(oracle, W, H, a, b, bits, f, op), argb[:W * H], avg=avg)
            assert np.array_equal(y, y_o) and np.array_equal(cb, cb_o) and np.array_equal(cr, cr_o)


@pytest.mark.parametrize("zero_copy", [True, False])
def test_bits_through_the_host_frame_pipeline(csic, oracle, zero_copy):
    rng = np.random.default_rng(7500)
    for (W, H, a, b, bits, f, order, avg) in ((128, 16, 2, 0, (6, 5, 5), 1, CSQ, False), (250, 37, 2, 0, (3, 3, 2), 2, CSQ, False),
                                              (512, 20, 2, 2, (4, 4, 4), 2, CSQ, False), (128, 32, 2, 0, (5, 4, 3), 2, CSQ, True)):
        frames = [rng.integers(0, 1 << 32, (H, W), dtype=np.uint32) for _ in range(5)]
        op_ = _op(oracle, W, H, a, b, bits, f, order)
        with _plan(csic, W, H, a, b, bits, f, order, avg=avg) as pl, csic.FramePipeline(pl, depth=2, zero_copy=zero_copy) as pipe:
            outs = list(pipe.run(frames))
            assert len(outs) == len(frames)
            lay = pl.planar_bits_layout
            for fr, got in zip(frames, outs):
                assert got.dtype == np.uint8 and got.size == lay.frame_bytes
                _, y_o, cb_o, cr_o = oracle.planar(op_, fr.reshape(-1), avg=avg)
                y, cb, cr = pl.unpack_planar_bits(got)
                assert np.array_equal(y, y_o) and np.array_equal(cb, cb_o) and np.array_equal(cr, cr_o), (W, H, a, b, f, order, avg)


def test_bits_processPlanarBits(csic, oracle):
    rng = np.random.default_rng(7600)
    W, H = 96, 30
    argb = rng.integers(0, 1 << 32, (H, W), dtype=np.uint32)
    top = csic.ImageCompressorTop(W, H, 2, 0, 6, 5, 5, 2, *[csic.ProcessingStep(x) for x in CSQ])
    got = top.processPlanarBits(argb)
    pl = top.plan(csic.PixelFormat.PLANAR_BITS)
    _, y_o, cb_o, cr_o = oracle.planar(_op(oracle, W, H, 2, 0, (6, 5, 5), 2, CSQ), argb.reshape(-1))
    y, cb, cr = pl.unpack_planar_bits(got)
    assert np.array_equal(y, y_o) and np.array_equal(cb, cb_o) and np.array_equal(cr, cr_o)
    top.close()


def test_bits_full_size_vs_oracle(csic, oracle):
    """8192 x 8192 4:2:0 at factor 1, 6/5/5 (k_pbits_f1), and BASELINE cfg4 (factor 2) at 3/3/2 (k_pbits_strided), against the oracle,
    and the round trip through k_rbits against the packed kernels on the device."""
    import torch
    N = csic._native
    W = H = 8192
    sh = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_in = torch.empty(W * H, dtype=torch.int32, device="cuda:0")
    N.check(N.lib().csic_synth_frame_device(C.c_void_p(d_in.data_ptr()), d_in.numel(), 0, 20250629, sh))
    argb = d_in.cpu().numpy().view(np.uint32)
    for bits, f, family in (((6, 5, 5), 1, "k_pbits_f1"), ((3, 3, 2), 2, "k_pbits_strided")):
        with _plan(csic, W, H, 2, 0, bits, f, CSQ) as pl, _plan(csic, W, H, 2, 0, bits, f, CSQ, fmt=0) as packed:
            assert pl.kernel_name.startswith(family), pl.kernel_name
            lay = pl.planar_bits_layout
            buf = torch.full((lay.frame_bytes,), CANARY, dtype=torch.uint8, device="cuda:0")
            pl.process_device(d_in, buf)
            _, y_o, cb_o, cr_o = oracle.planar(_op(oracle, W, H, 2, 0, bits, f, CSQ), argb)
            assert np.array_equal(buf.cpu().numpy(), _expected_frame(lay, y_o, cb_o, cr_o)), (bits, f)
            back = pl.reconstruct_bits_device(buf)
            want = packed.process_device(d_in)
            assert torch.equal(back.reshape(-1), want.reshape(-1)), (bits, f)
            del buf, back, want


def test_bits_is_refused_where_it_is_not_supported(csic, oracle, tmp_path):
    """Row pitches, every frame-graph backend (FUSED and AUTO included), the file pools, csic_multi_* and the stream model return
    CSIC_EINVAL_FORMAT for a CSIC_FMT_PLANAR_BITS plan; reconstruct_bits takes packed output formats only."""
    import torch
    N = csic._native
    lib = N.lib()
    W, H = 256, 16
    with _plan(csic, W, H, 2, 0, (6, 5, 5), 1, CSQ) as pl:
        lay = pl.planar_bits_layout
        d_in = torch.zeros(W * H, dtype=torch.int32, device="cuda:0")
        d_out = torch.zeros(lay.frame_bytes, dtype=torch.uint8, device="cuda:0")
        assert lib.csic_process_pitched_device(pl._h, C.c_void_p(d_in.data_ptr()), W, C.c_void_p(d_out.data_ptr()), W, 1, None) == N.EINVAL_FORMAT
        pin = (C.c_void_p * 1)(C.c_void_p(d_in.data_ptr()))
        pout = (C.c_void_p * 1)(C.c_void_p(d_out.data_ptr()))
        for backend in (N.FRAME_GRAPH_HIP, N.FRAME_GRAPH_DIRECT, N.FRAME_GRAPH_FUSED, N.FRAME_GRAPH_AUTO):
            h = C.c_void_p()
            assert lib.csic_frame_graph_create_ex(pl._h, pin, pout, 1, 0, backend, C.byref(h)) == N.EINVAL_FORMAT, backend
            assert "PLANAR_BITS" in lib.csic_last_error().decode()
            assert not h.value
        h = C.c_void_p()
        assert lib.csic_frame_graph_create(pl._h, pin, pout, 1, 0, C.byref(h)) == N.EINVAL_FORMAT
        ins = (C.c_char_p * 1)(str(tmp_path / "in.png").encode())
        outs = (C.c_char_p * 1)(str(tmp_path / "out.png").encode())
        assert lib.csic_process_png_files(pl._h, ins, outs, 1, 1, 1, 1, 0, 0, None) == N.EINVAL_FORMAT
        assert "PLANAR_BITS" in lib.csic_last_error().decode()
        assert lib.csic_reconstruct_bits_device(pl._h, C.c_void_p(d_out.data_ptr()), C.c_void_p(d_in.data_ptr()), 1, N.FMT_PLANAR_BITS, None) == N.EINVAL_FORMAT
        assert lib.csic_process_device(pl._h, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr() + 4), None) == N.EINVAL_SIZE
        devs = (C.c_int32 * 1)(0)
        m = C.c_void_p()
        assert lib.csic_multi_create(C.byref(pl.c_params), devs, 1, C.byref(m)) == N.EINVAL_FORMAT
        assert "PLANAR_BITS" in lib.csic_last_error().decode()
        s = C.c_void_p()
        assert lib.csic_stream_create(C.byref(pl.c_params), N.STREAM_TOP, C.byref(s)) == N.EINVAL_FORMAT
