"""Structural similarity without a GPU: a numpy statement of the definition in include/csic.h (csic_ssim_*), checked on a
hand-worked window, against a per-window evaluation in plain Python through the oracle's outputs and against the floating-point
SSIM it stands for; the Ssim helpers of the Python and the refusals of the four C entry points that need no device.
tests/test_gpu_ssim.py holds the GPU against this."""
import ctypes as C
import itertools

import numpy as np
import pytest

import csic_amd as csic
from test_distortion_host import forward, inverse, oracle_params, unpack

N = csic._native
CSQ = (3, 1, 2)
C1, C2 = 416, 235963
ONE = 65536


# ---- the definition, in numpy ------------------------------------------------------------------
def window_q(x, y):
    """q of windows: x, y integer arrays (..., 64) of reference and output values -> int64 array (...)."""
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    s1, s2 = x.sum(-1), y.sum(-1)
    ss, s12 = (x * x).sum(-1) + (y * y).sum(-1), (x * y).sum(-1)
    var, covar = 64 * ss - s1 * s1 - s2 * s2, 64 * s12 - s1 * s2
    n = (2 * s1 * s2 + C1) * (2 * covar + C2)
    d = (s1 * s1 + s2 * s2 + C1) * (var + C2)
    return np.sign(n) * ((64 * np.abs(n)) // (d // 1024))


def _windows(ch):
    """(H, W) -> (H / 8, W / 8, 64): the whole 8 x 8 windows, row-major inside."""
    H, W = ch.shape
    ny, nx = H // 8, W // 8
    return ch[:ny * 8, :nx * 8].reshape(ny, 8, nx, 8).transpose(0, 2, 1, 3).reshape(ny, nx, 64)


def _channels(frame, o_rgb, o_ycc, f, rounding, in_format):
    """Six (reference, output) pairs of (H, W) int64 arrays: the pairing of sse_numpy."""
    frame = np.asarray(frame, dtype=np.uint32)
    H, W = frame.shape
    rows, cols = np.arange(H) // f, np.arange(W) // f
    up_rgb = np.asarray(o_rgb, dtype=np.uint32)[rows[:, None], cols[None, :]]
    up_ycc = np.asarray(o_ycc, dtype=np.uint32)[rows[:, None], cols[None, :]]
    if in_format == N.FMT_YCBCR888X:
        cr, cb, y = unpack(frame)
        ref = list(inverse(y, cb, cr)) + [y, cb, cr]
    else:
        ref = list(unpack(frame)) + list(forward(frame, rounding))
    ocr, ocb, oy = unpack(up_ycc)
    return list(zip(ref, list(unpack(up_rgb)) + [oy, ocb, ocr]))


def ssim_numpy(frame, o_rgb, o_ycc, f, rounding=0, in_format=0):
    """(sums[6], map[6, H / 8, W / 8]) of one input frame (H, W) against its packed outputs (Ho, Wo), paired by replication."""
    qmap = np.stack([window_q(_windows(ref), _windows(out)) for ref, out in _channels(frame, o_rgb, o_ycc, f, rounding, in_format)])
    return [int(v) for v in qmap.sum(axis=(1, 2))], qmap.astype(np.int32)


def oracle_outputs(orc, frame, W, H, a=4, b=4, bits=(8, 8, 8), f=1, op=CSQ, rounding=0, avg=False, in_format=0):
    form = "avg" if avg else "stream"
    return [orc.process(oracle_params(orc, W, H, a, b, bits, f, op, rounding, fmt, in_format), frame, form=form)
            for fmt in (orc.FMT_ARGB, orc.FMT_YCC)]


def oracle_ssim(orc, frame, W, H, a=4, b=4, bits=(8, 8, 8), f=1, op=CSQ, rounding=0, avg=False, in_format=0):
    """ssim_numpy against the oracle's packed outputs of these parameters (form "avg" for the AVG extension)."""
    outs = oracle_outputs(orc, frame, W, H, a, b, bits, f, op, rounding, avg, in_format)
    return ssim_numpy(np.asarray(frame, dtype=np.uint32).reshape(H, W), outs[0], outs[1], f, rounding, in_format)


def float_ssim(x, y):
    """The SSIM the integers stand for, N / D in floating point from exact Python integers."""
    x, y = [int(v) for v in x], [int(v) for v in y]
    s1, s2 = sum(x), sum(y)
    ss, s12 = sum(v * v for v in x) + sum(v * v for v in y), sum(p * q for p, q in zip(x, y))
    n = (2 * s1 * s2 + C1) * (2 * (64 * s12 - s1 * s2) + C2)
    d = (s1 * s1 + s2 * s2 + C1) * (64 * ss - s1 * s1 - s2 * s2 + C2)
    return n, d


# ---- the numpy statement itself ----------------------------------------------------------------
def _gray(v):
    return (0xFF000000 | (v.astype(np.uint32) * 0x010101)).astype(np.uint32)


def test_hand_worked_window():
    """x(i, j) = 10 j + 3 i (row i, column j), y = x & 0xF0 (a 4-bit quantiser):
      row sums of x: 280 + 24 i -> s1 = 8 * 280 + 24 * 28 = 2912;   y takes 0, 16, ..., 80 -> s2 = 2432
      sum x^2 = 169 120, sum y^2 = 129 024 -> ss = 298 144;   s12 = 146 592
      vars  = 64 * 298144 - 2912^2 - 2432^2 = 19 081 216 - 8 479 744 - 5 914 624 = 4 686 848
      covar = 64 * 146592 - 2912 * 2432 = 9 381 888 - 7 081 984 = 2 299 904
      N = (2 * 7081984 + 416) * (2 * 2299904 + 235963) = 14 164 384 * 4 835 771 = 68 495 717 380 064
      D = (8479744 + 5914624 + 416) * (4686848 + 235963) = 14 394 784 * 4 922 811 = 70 862 801 017 824
      q = floor(64 * N / floor(D / 1024)) = floor(4 383 725 912 324 096 / 69 201 954 118) = 63 346   (N / D = 0.96660)."""
    i, j = np.mgrid[0:8, 0:8]
    x = 10 * j + 3 * i
    y = x & 0xF0
    assert (int(x.sum()), int(y.sum())) == (2912, 2432)
    assert int((x * x).sum() + (y * y).sum()) == 298144 and int((x * y).sum()) == 146592
    n, d = float_ssim(x.ravel(), y.ravel())
    assert (n, d) == (68495717380064, 70862801017824) and d // 1024 == 69201954118
    assert int(window_q(x.reshape(64), y.reshape(64))) == 63346
    # as a frame: gray pixels carry x in R, G and B, the ARGB output carries y
    sums, qmap = ssim_numpy(_gray(x), _gray(y), np.zeros((8, 8), dtype=np.uint32), 1)
    assert sums[:3] == [63346] * 3 and qmap.shape == (6, 1, 1) and qmap[:3, 0, 0].tolist() == [63346] * 3
    # and a negative one: the ramp 32 j against its complement, covar = -22 020 096
    x = (32 * j).reshape(64)
    assert int(window_q(x, 255 - x)) == -62948


def _loop_ssim(orc, frame, W, H, f, rounding, in_format, o_rgb, o_ycc):
    """The definition window by window in plain Python integers, through the oracle's scalar transforms."""
    ny, nx = H // 8, W // 8
    sums, qmap = [0] * 6, np.zeros((6, ny, nx), dtype=np.int32)
    for wy in range(ny):
        for wx in range(nx):
            xs, ys = [[] for _ in range(6)], [[] for _ in range(6)]
            for r in range(8 * wy, 8 * wy + 8):
                for c in range(8 * wx, 8 * wx + 8):
                    v = int(frame[r * W + c])
                    if in_format == 1:
                        ycc = (v & 255, (v >> 8) & 255, (v >> 16) & 255)
                        rgb = tuple(orc.ycbcr2rgb(*ycc))
                    else:
                        rgb = ((v >> 16) & 255, (v >> 8) & 255, v & 255)
                        ycc = tuple(orc.rgb2ycbcr(*rgb, rounding))
                    o, q = int(o_rgb[r // f, c // f]), int(o_ycc[r // f, c // f])
                    out = ((o >> 16) & 255, (o >> 8) & 255, o & 255, q & 255, (q >> 8) & 255, (q >> 16) & 255)
                    for k, ref in enumerate(rgb + ycc):
                        xs[k].append(int(ref))
                        ys[k].append(out[k])
            for k in range(6):
                n, d = float_ssim(xs[k], ys[k])
                q = (64 * abs(n)) // (d // 1024)
                q = -q if n < 0 else q
                sums[k] += q
                qmap[k, wy, wx] = q
    return sums, qmap


ORDERS = list(itertools.permutations((1, 2, 3)))
CHROMA = [(4, 4), (2, 2), (2, 0), (1, 1), (4, 0), (1, 0)]


def test_numpy_ssim_matches_a_per_window_evaluation_of_oracle_outputs(oracle):
    rng = np.random.default_rng(4242)
    seen_negative = False
    for i in range(30):
        W, H = int(rng.integers(8, 41)), int(rng.integers(8, 25))
        f = int(rng.choice([1, 2, 4, 8]))
        a, b = CHROMA[int(rng.integers(0, 6))]
        bits = tuple(int(v) for v in rng.integers(1, 9, 3))
        avg = rng.random() < 0.3
        op = CSQ if avg else ORDERS[int(rng.integers(0, 6))]
        rounding, in_format = int(rng.integers(0, 2)), int(rng.random() < 0.25)
        frame = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        if in_format == 1:
            frame &= np.uint32(0x00FFFFFF)
        outs = oracle_outputs(oracle, frame, W, H, a, b, bits, f, op, rounding, avg, in_format)
        sums, qmap = oracle_ssim(oracle, frame, W, H, a, b, bits, f, op, rounding, avg, in_format)
        want_sums, want_map = _loop_ssim(oracle, frame, W, H, f, rounding, in_format, outs[0], outs[1])
        assert sums == want_sums and np.array_equal(qmap, want_map), (W, H, a, b, bits, f, op, rounding, avg, in_format)
        assert qmap.shape == (6, H // 8, W // 8)
        seen_negative |= bool((qmap < 0).any())
    assert seen_negative                      # noise against a coarse decimation: some windows anticorrelate


def _extreme_windows():
    z, w = np.zeros(64, dtype=np.int64), np.full(64, 255, dtype=np.int64)
    half = np.concatenate([np.zeros(32, dtype=np.int64), np.full(32, 255, dtype=np.int64)])
    checker = (np.indices((8, 8)).sum(0) & 1).reshape(64) * 255
    return [(z, z), (w, w), (z, w), (w, z), (half, half), (half, 255 - half), (checker, checker), (checker, 255 - checker),
            (half, z), (half, w), (checker, half)]


def test_identity_is_one_and_the_quotient_is_bounded():
    rng = np.random.default_rng(17)
    x = rng.integers(0, 256, (4000, 64))
    assert (window_q(x, x) == ONE).all()
    for lo, hi in ((0, 256), (0, 2), (250, 256), (100, 140)):
        x, y = rng.integers(lo, hi, (4000, 64)), rng.integers(lo, hi, (4000, 64))
        assert (np.abs(window_q(x, y)) <= ONE).all()
    for x, y in _extreme_windows():
        q = int(window_q(x, y))
        assert abs(q) <= ONE and (q == ONE) == bool((x == y).all())


def test_the_fixed_point_quotient_is_within_2_6e_5_of_the_float_ssim():
    rng = np.random.default_rng(23)
    cases = list(_extreme_windows())
    for lo, hi in ((0, 256), (0, 4), (252, 256), (120, 136)):
        cases += [(rng.integers(lo, hi, 64), rng.integers(lo, hi, 64)) for _ in range(250)]
    x = rng.integers(0, 256, (250, 64))
    cases += [(v, np.clip(v + rng.integers(-6, 7, 64), 0, 255)) for v in x]          # nearly equal: SSIM close to 1
    cases += [(v, 255 - v) for v in x[:50]]
    worst = 0.0
    for x, y in cases:
        n, d = float_ssim(x, y)
        assert 64 * abs(n) < 2 ** 63 and abs(n) <= d and 98160608 <= d
        err = abs(int(window_q(x, y)) / ONE - n / d)
        worst = max(worst, err)
        assert err < 2.6e-5
    assert worst > 0


# ---- Ssim helpers ------------------------------------------------------------------------------
def test_ssim_helpers():
    s = csic.Ssim([ONE * 10, ONE * 5, 0, -ONE * 10, 32768 * 10, 1], 10)
    assert s.mean("R") == 1.0 and s.mean(1) == 0.5 and s.mean("B") == 0.0 and s.mean("Y") == -1.0 and s.mean("Cb") == 0.5
    assert s.mean("Cr") == 1 / (ONE * 10)
    assert s.mean_rgb == pytest.approx(0.5, abs=1e-15)
    assert s.sums == (ONE * 10, ONE * 5, 0, -ONE * 10, 327680, 1) and s.windows == 10
    assert s == csic.Ssim(list(s.sums), 10) and s != csic.Ssim(list(s.sums), 11) and s != csic.Distortion([0] * 6, 10)
    assert repr(s) == f"Ssim(sums={s.sums}, windows=10)"
    assert csic.Ssim.CHANNELS == csic.Distortion.CHANNELS
    with pytest.raises(ValueError):
        csic.Ssim([1, 2, 3], 10)


# ---- refusals that need no device --------------------------------------------------------------
def test_null_arguments_are_refused_without_a_device():
    L = N.lib()
    b = C.c_size_t()
    assert L.csic_ssim_workspace_bytes(None, 1, C.byref(b)) == N.EINVAL_NULL
    buf = C.create_string_buffer(64)
    sums = (C.c_int64 * 6)()
    assert L.csic_ssim_device(None, buf, 1, buf, None, buf, 64, None) == N.EINVAL_NULL
    assert L.csic_ssim_host(None, buf, 16, 1, sums, None) == N.EINVAL_NULL
    assert L.csic_ssim_kernel_name(None) == b""
    assert (N.SSIM_WINDOW, N.SSIM_ONE) == (8, ONE)
