"""The quantiser sweep without a GPU (csic_qsweep_*; definition in include/csic.h): csic_qsweep_rank against a numpy ranker on synthetic
tables, the exact raw sizes, the refusals of every entry point that come before any device is touched, what a machine without a device
answers, and the refusals of `compress --target-bytes`.  tests/test_gpu_qsweep.py holds the kernels against csic_distortion_* and
csic_code_stats_*."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN

import csic_amd as csic
from test_container import _c_params

N = csic._native
CSQ = (3, 1, 2)
WORDS = C.sizeof(N.CsicQsweepResult) // 8
CODINGS = {"raw": 0, "groups": 1, "rice": 3, "rans": 5}


# ---- the ranking, in numpy ---------------------------------------------------------------------
def entropy_bits(h):
    """N H of one histogram in bits (float64): 0 for an empty or single-valued one."""
    h = np.asarray(h, dtype=np.float64)
    n = h.sum()
    if n == 0:
        return 0.0
    p = h[h > 0] / n
    return max(0.0, float(-(p * np.log2(p)).sum())) * n


def rank_numpy(sse, hist, weights=(1, 1, 1), max_bits=(8, 8, 8), raw_bytes=None):
    """sse (nframes, 3, 8), hist (nframes, 3, 8, 256) -> [(D, est, (y, cb, cr))] in rank order; Python integers for D.  raw_bytes:
    a function of (y, cb, cr) for the raw coding, None for the coded estimate."""
    sse = np.asarray(sse, dtype=np.uint64).reshape(-1, 3, 8)
    hist = np.asarray(hist, dtype=np.uint64).reshape(-1, 3, 8, 256)
    tot = [[sum(int(v) for v in sse[:, p, q]) for q in range(8)] for p in range(3)]
    hs = hist.astype(object).sum(axis=0)
    plane_bytes = [[math.ceil(min(float(int(hs[p, q].sum())) * (q + 1), entropy_bits(hs[p, q].astype(np.float64))) / 8.0) for q in range(8)]
                   for p in range(3)]
    out = []
    for y in range(1, max_bits[0] + 1):
        for cb in range(1, max_bits[1] + 1):
            for cr in range(1, max_bits[2] + 1):
                d = weights[0] * tot[0][y - 1] + weights[1] * tot[1][cb - 1] + weights[2] * tot[2][cr - 1]
                est = raw_bytes((y, cb, cr)) if raw_bytes else 80 + plane_bytes[0][y - 1] + plane_bytes[1][cb - 1] + plane_bytes[2][cr - 1]
                out.append((d, est, (y, cb, cr)))
    return sorted(out)


def rank_c(c_params, table, nframes, coding, weights=(1, 1, 1), max_bits=(8, 8, 8), capacity=512):
    table = np.ascontiguousarray(table, dtype=np.uint64).reshape(nframes, WORDS)
    out = (N.CsicQsweepCandidate * max(capacity, 1))()
    n = C.c_int32(capacity)
    st = N.lib().csic_qsweep_rank(C.byref(c_params), table.ctypes.data_as(C.c_void_p), nframes, coding,
                                  (C.c_uint8 * 3)(*weights) if weights is not None else None,
                                  (C.c_uint8 * 3)(*max_bits) if max_bits is not None else None, out, C.byref(n))
    return st, [(c.distortion, c.est_bytes, (c.y_bits, c.cb_bits, c.cr_bits)) for c in out[:n.value]] if st == N.OK else []


def synthetic_table(rng, nframes, n_y, n_c):
    """Tables as a sweep gives them: the totals of every histogram of a plane agree, bins >= 2^q are empty, the sums fall with q."""
    table = np.zeros((nframes, WORDS), dtype=np.uint64)
    sse = table[:, :24].reshape(nframes, 3, 8)
    hist = table[:, 24:].reshape(nframes, 3, 8, 256)
    for f in range(nframes):
        for p, n in enumerate((n_y, n_c, n_c)):
            steps = rng.integers(1, 1 << 40, 8, dtype=np.uint64)
            sse[f, p] = np.cumsum(steps)[::-1]
            sse[f, p, 7] = 0 if rng.random() < 0.5 else sse[f, p, 7]
            for q in range(1, 9):
                conc = rng.choice([0.02, 0.3, 5.0])                      # peaked ... flat: entropies from near 0 to near q
                w = rng.dirichlet(np.full(1 << q, conc))
                hist[f, p, q - 1, :1 << q] = rng.multinomial(n, w)
    return table


@pytest.mark.parametrize("seed", range(4))
def test_rank_against_numpy_on_synthetic_tables(seed):
    rng = np.random.default_rng(4200 + seed)
    nframes = (1, 1, 3, 2)[seed]
    W, H = ((64, 48), (100, 36), (32, 32), (252, 4))[seed]
    cp = _c_params(W, H, 2, 0, (6, 5, 5), 1, CSQ)
    table = synthetic_table(rng, nframes, W * H, W * H // 4)
    weights = ((1, 1, 1), (3, 1, 2), (255, 1, 1), (1, 7, 7))[seed]
    max_bits = ((8, 8, 8), (8, 8, 8), (6, 5, 5), (8, 3, 8))[seed]
    sse, hist = table[:, :24], table[:, 24:]
    for coding in ("rans", "rice", "groups"):
        want = rank_numpy(sse, hist, weights, max_bits)
        # no two candidates of equal distortion have estimates within 2 bytes: the order cannot hinge on one rounding
        for (d0, e0, _), (d1, e1, _) in zip(want, want[1:]):
            assert d0 < d1 or abs(e0 - e1) > 2
        st, got = rank_c(cp, table, nframes, CODINGS[coding], weights, max_bits)
        assert st == N.OK and len(got) == max_bits[0] * max_bits[1] * max_bits[2] == len(want)
        assert [(d, b) for d, _, b in got] == [(d, b) for d, _, b in want]
        assert all(abs(g[1] - w[1]) <= 1 for g, w in zip(got, want))
    # NULL weights and max_bits: 1, 1, 1 and 8, 8, 8
    assert rank_c(cp, table, nframes, 5, None, None)[1] == rank_c(cp, table, nframes, 5)[1]


def test_rank_breaks_ties_by_estimate_then_widths():
    """Equal sums at widths 7 and 8 of Y: the cheaper estimate comes first; all sums and all histograms equal: the widths decide."""
    cp = _c_params(16, 16, 4, 4, (8, 8, 8), 1, CSQ)
    table = np.zeros((1, WORDS), dtype=np.uint64)
    sse, hist = table[:, :24].reshape(3, 8), table[:, 24:].reshape(3, 8, 256)
    hist[:, :, 0] = 256                                         # single-valued: 0 bytes at every width
    st, got = rank_c(cp, table, 1, 5)
    assert st == N.OK and [b for _, _, b in got] == sorted(b for _, _, b in got) and {(d, e) for d, e, _ in got} == {(0, 80)}
    hist[0, 7, :] = 1                                           # Y at 8 bits: flat over 256 bins, 256 bytes; at 7 bits still free
    st, got = rank_c(cp, table, 1, 5, max_bits=(8, 1, 1))
    assert [(e, b) for _, e, b in got][-2:] == [(80, (7, 1, 1)), (80 + 256, (8, 1, 1))]
    sse[0, 7] = 0
    sse[0, :7] = 5
    st, got = rank_c(cp, table, 1, 5, max_bits=(8, 1, 1))
    assert got[0] == (0, 80 + 256, (8, 1, 1)) and got[1] == (5, 80, (1, 1, 1))
    # the estimate never exceeds the raw size of the plane: a flat histogram costs q bits per sample, not more
    hist[0, 2, :8] = 32
    assert {b: e for _, e, b in rank_c(cp, table, 1, 5, max_bits=(3, 1, 1))[1]}[(3, 1, 1)] == 80 + 256 * 3 // 8


def test_raw_estimates_are_the_exact_file_sizes():
    rng = np.random.default_rng(808)
    empty = np.zeros((3, WORDS), dtype=np.uint64)
    for i in range(40):
        W, H = int(rng.integers(1, 300)), int(rng.integers(1, 200))
        a, b = [(4, 4), (2, 2), (2, 0), (1, 1), (4, 0), (1, 0)][i % 6]
        f = int(rng.choice([1, 2, 4, 8]))
        op = [(3, 1, 2), (1, 3, 2), (1, 2, 3), (2, 1, 3), (2, 3, 1), (3, 2, 1)][int(rng.integers(0, 6))]
        nframes = int(rng.integers(1, 4))
        max_bits = tuple(int(v) for v in rng.integers(1, 9, 3))
        cp = _c_params(W, H, a, b, (3, 3, 2), f, op)
        st, got = rank_c(cp, empty[:nframes], nframes, CODINGS["raw"], (1, 1, 1), max_bits)
        assert st == N.OK and len(got) == max_bits[0] * max_bits[1] * max_bits[2]
        for d, est, bits in got:
            lay = N.CsicPlanarBitsLayout()
            assert N.lib().csic_planar_bits_layout_of(C.byref(_c_params(W, H, a, b, bits, f, op)), C.byref(lay)) == N.OK
            assert d == 0 and est == 80 + nframes * lay.payload_bytes
        # equal distortion everywhere: ascending size, then widths
        assert [(e, b) for _, e, b in got] == sorted((e, b) for _, e, b in got)


def test_rank_refusals():
    cp = _c_params(16, 16, 2, 0, (6, 5, 5), 1, CSQ)
    table = np.zeros((1, WORDS), dtype=np.uint64)
    L = N.lib()
    out = (N.CsicQsweepCandidate * 512)()
    n = C.c_int32(512)
    tp = table.ctypes.data_as(C.c_void_p)
    assert L.csic_qsweep_rank(None, tp, 1, 5, None, None, out, C.byref(n)) == N.EINVAL_NULL
    assert L.csic_qsweep_rank(C.byref(cp), None, 1, 5, None, None, out, C.byref(n)) == N.EINVAL_NULL
    assert L.csic_qsweep_rank(C.byref(cp), tp, 1, 5, None, None, None, C.byref(n)) == N.EINVAL_NULL
    assert L.csic_qsweep_rank(C.byref(cp), tp, 1, 5, None, None, out, None) == N.EINVAL_NULL
    for nframes in (0, -1, 65536):
        assert L.csic_qsweep_rank(C.byref(cp), tp, nframes, 5, None, None, out, C.byref(n)) == N.EINVAL_SIZE
    for coding in (2, 4, 6, -1):
        assert rank_c(cp, table, 1, coding)[0] == N.EINVAL_FORMAT
    ycc = _c_params(16, 16, 2, 0, (6, 5, 5), 1, CSQ)
    ycc.in_format = N.FMT_YCBCR888X
    assert rank_c(ycc, table, 1, 5)[0] == N.EINVAL_FORMAT
    for w in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert rank_c(cp, table, 1, 5, weights=w)[0] == N.EINVAL_SIZE
    for mb in ((0, 8, 8), (8, 9, 8), (8, 8, 255)):
        assert rank_c(cp, table, 1, 5, max_bits=mb)[0] == N.EINVAL_BITS
    assert rank_c(cp, table, 1, 5, capacity=511)[0] == N.EINVAL_SIZE
    assert rank_c(cp, table, 1, 5, max_bits=(2, 2, 2), capacity=8)[0] == N.OK
    bad = _c_params(16, 16, 3, 0, (6, 5, 5), 1, CSQ)
    assert rank_c(bad, table, 1, 5)[0] == N.EINVAL_CHROMA_A
    # sums that leave 64 bits are refused, not wrapped
    table[0, 0] = np.uint64(1 << 63)
    assert rank_c(cp, table, 1, 5, weights=(2, 1, 1))[0] == N.EINVAL_SIZE
    big = np.concatenate([table, table])
    assert rank_c(cp, big, 2, 5)[0] == N.EINVAL_SIZE


def test_qsweep_python_helpers():
    cp = _c_params(16, 16, 4, 4, (6, 5, 5), 1, CSQ)
    table = np.zeros((1, WORDS), dtype=np.uint64)
    table[0, :24] = np.tile(np.array([16 * 16 * 255 * 255, 4000, 1000, 250, 60, 15, 4, 0], dtype=np.uint64), 3)
    table[:, 24:].reshape(3, 8, 256)[:, :, 0] = 256
    s = csic.QSweep(table, cp)
    assert s.nframes == 1 and s.sse.shape == (3, 8) and s.hist.shape == (3, 8, 256) and s.pixels == 256
    assert s.psnr("Y", 8) == math.inf and s.psnr(1, 1) == 0.0 and s.psnr("Cr", 7) == pytest.approx(10 * math.log10(65025 * 256 / 4))
    r = s.rank()
    assert len(r) == 512 and r[0] == (0, 80, (8, 8, 8)) and r[-1][2] == (1, 1, 1)
    assert s.rank("raw", max_bits=(2, 2, 2))[0] == (3 * 1000 * 0 + 3 * 4000, 80 + 3 * 64, (2, 2, 2))
    assert s.est_bytes((6, 5, 5), "raw") == 80 + 32 * 6 + 32 * 5 + 32 * 5 and s.est_bytes((6, 5, 5)) == 80
    with pytest.raises(csic.IllegalArgumentException):
        s.rank(weights=(0, 1, 1))
    two = csic.QSweep(np.concatenate([table, table]), cp)
    assert two.nframes == 2 and two.sse.shape == (2, 3, 8) and two.psnr("Cr", 7) == s.psnr("Cr", 7)
    assert two.rank()[1][0] == 2 * s.rank()[1][0]


# ---- refusals that need no device --------------------------------------------------------------
def test_arguments_are_checked_before_any_device_is_touched():
    """`standin` is zeroed memory in a plan's place (ARGB input): a refused call never looks further."""
    L = N.lib()
    standin = C.create_string_buffer(4096)
    raw = C.create_string_buffer(4096 + 256)
    base = (C.addressof(raw) + 255) & ~255
    buf, res, ws = C.c_void_p(base), C.c_void_p(base + 512), C.c_void_p(base + 1024)
    assert L.csic_qsweep_device(None, buf, 1, res, ws, 4096, None) == N.EINVAL_NULL
    assert L.csic_qsweep_device(standin, None, 1, res, ws, 4096, None) == N.EINVAL_NULL
    assert L.csic_qsweep_device(standin, buf, 1, None, ws, 4096, None) == N.EINVAL_NULL
    assert L.csic_qsweep_device(standin, buf, 1, res, None, 4096, None) == N.EINVAL_NULL
    assert L.csic_qsweep_hist_device(None, buf, 1, res, None) == N.EINVAL_NULL
    assert L.csic_qsweep_hist_device(standin, None, 1, res, None) == N.EINVAL_NULL
    assert L.csic_qsweep_hist_device(standin, buf, 1, None, None) == N.EINVAL_NULL
    assert L.csic_qsweep_host(None, buf, 256, 1, res) == N.EINVAL_NULL
    assert L.csic_qsweep_host(standin, None, 256, 1, res) == N.EINVAL_NULL
    assert L.csic_qsweep_host(standin, buf, 256, 1, None) == N.EINVAL_NULL
    assert L.csic_qsweep_workspace_bytes(None, 1, C.byref(C.c_size_t())) == N.EINVAL_NULL
    assert L.csic_qsweep_workspace_bytes(standin, 1, None) == N.EINVAL_NULL
    for nframes in (0, -3, 65536):
        assert L.csic_qsweep_device(standin, buf, nframes, res, ws, 4096, None) == N.EINVAL_SIZE
        assert L.csic_qsweep_hist_device(standin, buf, nframes, res, None) == N.EINVAL_SIZE
        assert L.csic_qsweep_host(standin, buf, 256, nframes, res) == N.EINVAL_SIZE
        assert L.csic_qsweep_workspace_bytes(standin, nframes, C.byref(C.c_size_t())) == N.EINVAL_SIZE
    assert L.csic_qsweep_device(standin, C.c_void_p(base + 2), 1, res, ws, 4096, None) == N.EINVAL_SIZE
    assert L.csic_qsweep_device(standin, buf, 1, C.c_void_p(base + 512 + 4), ws, 4096, None) == N.EINVAL_SIZE
    assert L.csic_qsweep_device(standin, buf, 1, res, C.c_void_p(base + 1024 + 128), 4096, None) == N.EINVAL_SIZE
    assert L.csic_qsweep_hist_device(standin, C.c_void_p(base + 128), 1, res, None) == N.EINVAL_SIZE
    assert L.csic_qsweep_hist_device(standin, buf, 1, C.c_void_p(base + 512 + 4), None) == N.EINVAL_SIZE
    assert b"aligned" in L.csic_last_error()
    # a YCbCr input: the plan begins with its csic_params
    C.cast(standin, C.POINTER(N.CsicParams)).contents.in_format = N.FMT_YCBCR888X
    assert L.csic_qsweep_device(standin, buf, 1, res, ws, 4096, None) == N.EINVAL_FORMAT
    assert L.csic_qsweep_hist_device(standin, buf, 1, res, None) == N.EINVAL_FORMAT
    assert L.csic_qsweep_host(standin, buf, 256, 1, res) == N.EINVAL_FORMAT
    assert L.csic_qsweep_workspace_bytes(standin, 1, C.byref(C.c_size_t())) == N.EINVAL_FORMAT
    C.cast(standin, C.POINTER(N.CsicParams)).contents.in_format = N.FMT_ARGB8888
    # the two questions that need no device
    b = C.c_int64()
    assert L.csic_qsweep_block_samples(None, C.byref(b)) == N.EINVAL_NULL and L.csic_qsweep_block_samples(standin, None) == N.EINVAL_NULL
    assert L.csic_qsweep_block_samples(standin, C.byref(b)) == N.OK and b.value > 0 and b.value % (16 * 64) == 0 and b.value < 2 ** 32
    assert L.csic_qsweep_kernel_name(None) == b""
    assert (N.QSWEEP_WIDTHS, N.QSWEEP_MAX_CANDIDATES, N.QSWEEP_MAX_TRIES) == (8, 512, 4)
    assert C.sizeof(N.CsicQsweepResult) == 8 * (24 + 24 * 256) and C.sizeof(N.CsicQsweepCandidate) == 32
    assert N.CsicQsweepResult.hist.offset == 192
    # without a device every entry point that would launch says so, after its argument checks
    if L.csic_device_count() < 1:
        assert L.csic_qsweep_device(standin, buf, 1, res, ws, 4096, None) == N.ENODEVICE
        assert L.csic_qsweep_hist_device(standin, buf, 1, res, None) == N.ENODEVICE
        assert L.csic_qsweep_host(standin, buf, 256, 1, res) == N.ENODEVICE
        h = C.c_void_p()
        assert L.csic_plan_create(C.byref(_c_params(16, 16, 2, 0, (6, 5, 5), 1, CSQ)), 0, C.byref(h)) == N.ENODEVICE


# ---- the command line --------------------------------------------------------------------------
def test_cli_refusals(tmp_path, capsys):
    png = os.path.join(GOLDEN, "inputs", "in16.png")
    out = str(tmp_path / "x.csic")
    assert csic.app.main(["compress", "--inputs", f"{png},{png}", "--gop", "2", "--output", out, "--target-bytes", "5000"]) == 2
    assert "--target-bytes" in capsys.readouterr().out and not os.path.exists(out)
    for n in ("79", "0", "-5"):
        assert csic.app.main(["compress", "--input", png, "--output", out, "--sf", "1", "--target-bytes", n]) == 2
        assert "at least the 80 bytes" in capsys.readouterr().out and not os.path.exists(out)
    assert csic.app.main(["compress", "--input", png, "--output", out, "--target-bytes", "many"]) == 2
    assert csic.app.main(["compress", "--input", png, "--output", out, "--target-bytes", "5000", "--coding", "zip"]) == 2
    assert not os.path.exists(out)
    with pytest.raises(csic.IllegalArgumentException):
        csic.ImageCompressionApp.compressImageToSize(png, out, 2, 0, 8, 8, 8, 1, csic.ProcessingStep.ChromaSubsampling,
                                                     csic.ProcessingStep.SpatialSampling, csic.ProcessingStep.ColorQuantization, targetBytes=79)
    with pytest.raises(csic.IllegalArgumentException):
        csic.ImageCompressionApp.compressImageToSize(png, out, 2, 0, 8, 8, 8, 1, csic.ProcessingStep.ChromaSubsampling,
                                                     csic.ProcessingStep.SpatialSampling, csic.ProcessingStep.ColorQuantization, targetBytes=5000, coding="zip")
