"""Distortion measurement without a GPU: a numpy statement of the definition in include/csic.h (csic_distortion_*), checked on
a hand-worked frame and against a per-pixel evaluation through the oracle's own transforms; the PSNR helpers of the Python and
the refusals of the four C entry points that need no device.  tests/test_gpu_distortion.py holds the GPU against this."""
import ctypes as C
import math

import numpy as np
import pytest

import csic_amd as csic

N = csic._native
CSQ = (3, 1, 2)


# ---- the definition, in numpy ------------------------------------------------------------------
def _div256(x, trunc):
    return np.where(x < 0, -((-x) // 256), x // 256) if trunc else x // 256


def forward(argb, rounding):
    """(Y, Cb, Cr) int64 arrays of ARGB pixels: RGB2YCbCr under `rounding` (0 floor, 1 trunc)."""
    a = np.asarray(argb, dtype=np.uint32).astype(np.int64)
    r, g, b = (a >> 16) & 255, (a >> 8) & 255, a & 255
    t = rounding == 1
    y = np.clip(_div256(77 * r + 150 * g + 29 * b + 128, t), 0, 255)
    cb = np.clip(_div256(-43 * r - 85 * g + 128 * b + 128, t) + 128, 0, 255)
    cr = np.clip(_div256(128 * r - 107 * g - 21 * b + 128, t) + 128, 0, 255)
    return y, cb, cr


def inverse(y, cb, cr):
    """(R, G, B) int64 arrays: YCbCrUtils.ycbcr2rgb."""
    y, d, e = (np.asarray(v, dtype=np.int64) for v in (y, cb, cr))
    d, e = d - 128, e - 128
    return (np.clip((298 * y + 409 * e + 128) >> 8, 0, 255), np.clip((298 * y - 100 * d - 208 * e + 128) >> 8, 0, 255),
            np.clip((298 * y + 516 * d + 128) >> 8, 0, 255))


def unpack(px):
    a = np.asarray(px, dtype=np.uint32).astype(np.int64)
    return (a >> 16) & 255, (a >> 8) & 255, a & 255          # R, G, B  (or Cr, Cb, Y of a YCbCr pixel)


def sse_numpy(frame, o_rgb, o_ycc, f, rounding=0, in_format=0):
    """The six sums (R, G, B, Y, Cb, Cr) of one input frame (H, W) against its packed outputs (Ho, Wo), paired by replication."""
    frame = np.asarray(frame, dtype=np.uint32)
    H, W = frame.shape
    rows, cols = np.arange(H) // f, np.arange(W) // f
    up_rgb = np.asarray(o_rgb, dtype=np.uint32)[rows[:, None], cols[None, :]]
    up_ycc = np.asarray(o_ycc, dtype=np.uint32)[rows[:, None], cols[None, :]]
    if in_format == N.FMT_YCBCR888X:
        cr, cb, y = unpack(frame)
        ref_rgb = inverse(y, cb, cr)
        ref_ycc = (y, cb, cr)
    else:
        ref_rgb = unpack(frame)
        ref_ycc = forward(frame, rounding)
    ocr, ocb, oy = unpack(up_ycc)
    sums = [int(((ref - out) ** 2).sum()) for ref, out in zip(ref_rgb, unpack(up_rgb))]
    sums += [int(((ref - out) ** 2).sum()) for ref, out in zip(ref_ycc, (oy, ocb, ocr))]
    return sums


def oracle_params(orc, W, H, a=4, b=4, bits=(8, 8, 8), f=1, op=CSQ, rounding=0, fmt=0, in_format=0):
    return orc.OracleParams(width=W, height=H, chroma_a=a, chroma_b=b, y_bits=bits[0], cb_bits=bits[1], cr_bits=bits[2],
                            factor=f, op=op, rounding=rounding, out_format=fmt, in_format=in_format)


def oracle_sse(orc, frame, W, H, a=4, b=4, bits=(8, 8, 8), f=1, op=CSQ, rounding=0, avg=False, in_format=0):
    """sse_numpy against the oracle's packed outputs of these parameters (form "avg" for the AVG extension)."""
    form = "avg" if avg else "stream"
    outs = [orc.process(oracle_params(orc, W, H, a, b, bits, f, op, rounding, fmt, in_format), frame, form=form)
            for fmt in (orc.FMT_ARGB, orc.FMT_YCC)]
    return sse_numpy(np.asarray(frame, dtype=np.uint32).reshape(H, W), outs[0], outs[1], f, rounding, in_format)


# ---- the numpy statement itself ----------------------------------------------------------------
def _gray(v):
    return 0xFF000000 | (v * 0x010101)


def test_hand_worked_4x2_factor_2(oracle):
    """4:4:4, 8/8/8, chroma-spatial-quant, floor, factor 2: outputs (0, 0) <- input (0, 0), (0, 1) <- input (0, 2).
    Input: gray 0, RED, 20, 30 / gray 40, 50, 60, 70.
      output 0: Y 0, Cb = Cr = 128 -> RGB (0, 0, 0);  output 1: Y 20 -> RGB ((298 * 20 + 128) >> 8) = 23 for all three.
      red (255, 0, 0) has Y 77, Cb 85, Cr 255 (clamped from 256).
      R: 255^2 + 40^2 + 50^2 = 69125, plus (20-23)^2 + (30-23)^2 + (60-23)^2 + (70-23)^2 = 3636        -> 72761
      G = B: 0 + 40^2 + 50^2 = 4100, plus 3636                                                             -> 7736
      Y: 77^2 + 40^2 + 50^2 = 10029, plus 0 + 10^2 + 40^2 + 50^2 = 4200                                  -> 14229
      Cb: (85 - 128)^2 = 1849;  Cr: (255 - 128)^2 = 16129."""
    frame = np.array([[_gray(0), 0xFFFF0000, _gray(20), _gray(30)],
                      [_gray(40), _gray(50), _gray(60), _gray(70)]], dtype=np.uint32)
    o_rgb = np.array([[0xFF000000, _gray(23)]], dtype=np.uint32)
    o_ycc = np.array([[0 | 128 << 8 | 128 << 16, 20 | 128 << 8 | 128 << 16]], dtype=np.uint32)
    want = [72761, 7736, 7736, 14229, 1849, 16129]
    assert sse_numpy(frame, o_rgb, o_ycc, 2) == want
    # the outputs above are the oracle's
    assert oracle_sse(oracle, frame, 4, 2, f=2) == want


def test_numpy_transforms_match_the_oracle(oracle):
    rng = np.random.default_rng(7)
    px = rng.integers(0, 1 << 32, 400, dtype=np.uint32)
    for rounding in (0, 1):
        y, cb, cr = forward(px, rounding)
        for k in range(0, 400, 7):
            v = int(px[k])
            assert (y[k], cb[k], cr[k]) == oracle.rgb2ycbcr((v >> 16) & 255, (v >> 8) & 255, v & 255, rounding)
    r, g, b = inverse(*(rng.integers(0, 256, 300) for _ in range(3)))
    ycc = rng.integers(0, 256, (3, 300))
    r, g, b = inverse(*ycc)
    for k in range(0, 300, 5):
        assert (r[k], g[k], b[k]) == oracle.ycbcr2rgb(*(int(v) for v in ycc[:, k]))


def _loop_sse(orc, frame, W, H, f, rounding, in_format, o_rgb, o_ycc):
    """The definition pixel by pixel through the oracle's scalar transforms (independent of the numpy vectorisation)."""
    s = [0] * 6
    for r in range(H):
        for c in range(W):
            v = int(frame[r * W + c])
            if in_format == 1:
                ry, rcb, rcr = v & 255, (v >> 8) & 255, (v >> 16) & 255
                rgb = orc.ycbcr2rgb(ry, rcb, rcr)
            else:
                rgb = ((v >> 16) & 255, (v >> 8) & 255, v & 255)
                ry, rcb, rcr = orc.rgb2ycbcr(*rgb, rounding)
            o = int(o_rgb[r // f, c // f])
            q = int(o_ycc[r // f, c // f])
            out = ((o >> 16) & 255, (o >> 8) & 255, o & 255, q & 255, (q >> 8) & 255, (q >> 16) & 255)
            for k, ref in enumerate(rgb + (ry, rcb, rcr)):
                s[k] += (ref - out[k]) ** 2
    return s


@pytest.mark.parametrize("case", [
    dict(W=5, H=3, a=2, b=0, bits=(6, 5, 5), f=2, op=(3, 1, 2)),
    dict(W=7, H=3, a=1, b=1, bits=(3, 3, 2), f=8, op=(1, 3, 2)),
    dict(W=6, H=5, a=4, b=0, bits=(8, 8, 8), f=4, op=(2, 1, 3), rounding=1),
    dict(W=9, H=4, a=2, b=2, bits=(5, 4, 4), f=1, op=(1, 2, 3), in_format=1),
    dict(W=8, H=6, a=2, b=0, bits=(6, 5, 5), f=2, avg=True),
    dict(W=7, H=5, a=1, b=0, bits=(4, 4, 4), f=4, avg=True, rounding=1),
    dict(W=1, H=1, a=4, b=4, bits=(1, 1, 1), f=8),
])
def test_numpy_sse_matches_a_per_pixel_evaluation_of_oracle_outputs(oracle, case):
    case = dict(case)
    W, H, f = case["W"], case["H"], case["f"]
    rounding, in_format, avg = case.pop("rounding", 0), case.pop("in_format", 0), case.pop("avg", False)
    rng = np.random.default_rng(W * 100 + H)
    frame = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
    kw = dict(a=case["a"], b=case["b"], bits=case["bits"], f=f, op=case.get("op", CSQ), rounding=rounding)
    outs = [oracle.process(oracle_params(oracle, W, H, fmt=fmt, in_format=in_format, **kw), frame, form="avg" if avg else "stream")
            for fmt in (oracle.FMT_ARGB, oracle.FMT_YCC)]
    got = oracle_sse(oracle, frame, W, H, avg=avg, in_format=in_format, **kw)
    assert got == _loop_sse(oracle, frame, W, H, f, rounding, in_format, outs[0], outs[1])
    assert any(got)


# ---- PSNR helpers ------------------------------------------------------------------------------
def test_distortion_psnr_helpers():
    d = csic.Distortion([0, 0, 0, 0, 0, 0], 100)
    assert d.psnr("R") == math.inf and d.psnr(5) == math.inf and d.psnr_rgb == math.inf and d.mse("Y") == 0.0
    d = csic.Distortion([65025, 65025, 65025, 6502500, 650, 0], 100)
    assert d.mse("R") == 650.25 and d.psnr("R") == pytest.approx(20.0, abs=1e-12)
    assert d.psnr_rgb == pytest.approx(20.0, abs=1e-12)
    assert d.psnr("Y") == pytest.approx(0.0, abs=1e-12)                  # mse 255^2
    assert d.psnr(4) == pytest.approx(10 * math.log10(65025 * 100 / 650))
    assert d.psnr("Cr") == math.inf
    d = csic.Distortion([100, 200, 300, 1, 1, 1], 10)
    assert d.psnr_rgb == pytest.approx(10 * math.log10(65025 * 30 / 600))
    with pytest.raises(ValueError):
        csic.Distortion([1, 2, 3], 10)


# ---- refusals that need no device --------------------------------------------------------------
def test_null_arguments_are_refused_without_a_device():
    L = N.lib()
    b = C.c_size_t()
    assert L.csic_distortion_workspace_bytes(None, 1, C.byref(b)) == N.EINVAL_NULL
    buf = C.create_string_buffer(64)
    sse = (C.c_uint64 * 6)()
    assert L.csic_distortion_device(None, buf, 1, buf, buf, 64, None) == N.EINVAL_NULL
    assert L.csic_distortion_host(None, buf, 16, 1, sse) == N.EINVAL_NULL
    assert L.csic_distortion_kernel_name(None) == b""
    assert N.DIST_CHANNELS == 6
