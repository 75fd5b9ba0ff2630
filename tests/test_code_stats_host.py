"""Code statistics without a GPU: a numpy statement of the definition in include/csic.h (csic_code_stats_*), checked on the worked
vectors and on its own invariants; the CodeStats arithmetic on hand-made counts; what a natural image's planes carry; the refusals of
the C entry points that come before any device is touched; and the `inspect` subcommand on a container written on the CPU.
tests/test_gpu_code_stats.py holds the GPU against code_stats_numpy."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_png_rgb

import csic_amd as csic
from test_container import _c_params, _frame_buffer, _layout, pack_codes

N = csic._native
CSQ = (3, 1, 2)
KINDS, PLANES, BINS = 2, 3, 256


# ---- the definition, in numpy ------------------------------------------------------------------
def plane_hists(codes, q):
    """(h0, h1) of one plane: codes in storage order, q bits each -> two uint64 arrays of 256 counts."""
    c = np.asarray(codes, dtype=np.int64).reshape(-1)
    h0 = np.bincount(c, minlength=BINS).astype(np.uint64)
    if c.size == 0:
        return h0, h0.copy()
    e = np.concatenate([c[:1], np.diff(c) % (1 << q)])
    return h0, np.bincount(e, minlength=BINS).astype(np.uint64)


def code_stats_numpy(y, cb, cr, bits):
    """The planes' 8-bit values (what oracle.planar and Plan.split_planar give) -> uint64 [2][3][256]: code = value >> (8 - q)."""
    out = np.zeros((KINDS, PLANES, BINS), dtype=np.uint64)
    for p, (v, q) in enumerate(zip((y, cb, cr), bits)):
        out[0, p], out[1, p] = plane_hists(np.asarray(v, dtype=np.uint8).reshape(-1) >> (8 - q), q)
    return out


def oracle_planes(orc, frame, W, H, a=4, b=4, bits=(8, 8, 8), f=1, op=CSQ, rounding=0, avg=False):
    p = orc.OracleParams(width=W, height=H, chroma_a=a, chroma_b=b, y_bits=bits[0], cb_bits=bits[1], cr_bits=bits[2], factor=f,
                         op=op, rounding=rounding)
    _, y, cb, cr = orc.planar(p, np.asarray(frame, dtype=np.uint32).reshape(-1), avg=avg)
    return y, cb, cr


def oracle_code_stats(orc, frame, W, H, a=4, b=4, bits=(8, 8, 8), f=1, op=CSQ, rounding=0, avg=False):
    return code_stats_numpy(*oracle_planes(orc, frame, W, H, a, b, bits, f, op, rounding, avg), bits)


# ---- the numpy statement itself ----------------------------------------------------------------
def test_worked_vectors():
    h0, h1 = plane_hists([1, 2, 3, 4, 5, 6, 7, 0], 3)
    assert h1[1] == 8 and h1.sum() == 8 and h0[:8].tolist() == [1] * 8
    h0, h1 = plane_hists([0x1F, 0, 0x15], 5)
    assert h1[0x1F] == 1 and h1[1] == 1 and h1[0x15] == 1 and h1.sum() == 3
    assert h0[0x1F] == 1 and h0[0] == 1 and h0[0x15] == 1
    # the same through the bytes the bit layout stores them in (csic.h: d1 58 1f and 1f 54)
    assert pack_codes(np.array([1, 2, 3, 4, 5, 6, 7, 0]) << 5, 3).tobytes().hex() == "d1581f"
    assert pack_codes(np.array([0x1F, 0, 0x15]) << 3, 5).tobytes().hex() == "1f54"


def test_invariants_of_the_numpy_statement():
    rng = np.random.default_rng(7700)
    for _ in range(40):
        q = int(rng.integers(1, 9))
        n = int(rng.integers(0, 400))
        codes = rng.integers(0, 1 << q, n)
        h0, h1 = plane_hists(codes, q)
        assert int(h0.sum()) == n and int(h1.sum()) == n
        assert not h0[1 << q:].any() and not h1[1 << q:].any()
        assert np.array_equal(h0, np.bincount(codes, minlength=BINS))
        # the codes can be rebuilt from the residuals, so h0 can: a running sum mod 2^q
        if n:
            e = np.concatenate([codes[:1], np.diff(codes) % (1 << q)])
            assert np.array_equal(np.cumsum(e) % (1 << q), codes)
    # the low bits of a PLANAR byte are ignored
    a = code_stats_numpy([0xA7, 0xA0], [0x17], [0xFF], (4, 3, 1))
    assert a[0, 0, 0xA] == 2 and a[1, 0, 0xA] == 1 and a[1, 0, 0] == 1 and a[0, 1, 0] == 1 and a[0, 2, 1] == 1


# ---- CodeStats arithmetic ----------------------------------------------------------------------
def _stats(h0s, h1s, bits, pixels):
    hist = np.zeros((KINDS, PLANES, BINS), dtype=np.uint64)
    for p in range(3):
        hist[0, p, :len(h0s[p])] = h0s[p]
        hist[1, p, :len(h1s[p])] = h1s[p]
    return csic.CodeStats(hist, bits, pixels)


def test_code_stats_helpers():
    # Y: 64 samples uniform over 16 codes (H0 = 4 = q), residuals single-valued apart from e_0 placed in the same bin (H1 = 0)
    # Cb: constant (H = 0 for both); Cr: two codes 3 : 1 -> H0 = 0.811278..., residuals uniform over 4 -> H1 = 2 = q
    s = _stats([[4] * 16, [16], [12, 4]], [[0, 64], [1, 15], [4, 4, 4, 4]], (4, 3, 2), 64)
    assert s.samples == (64, 16, 16) and s.bits == (4, 3, 2) and s.pixels == 64
    assert s.entropy(0, "Y") == pytest.approx(4.0, abs=1e-12) and s.entropy(1, 0) == 0.0
    assert s.entropy(0, "Cb") == 0.0
    h_cb1 = -(1 / 16) * math.log2(1 / 16) - (15 / 16) * math.log2(15 / 16)
    assert s.entropy("residuals", "Cb") == pytest.approx(h_cb1, abs=1e-12)
    h_cr0 = -(0.75 * math.log2(0.75) + 0.25 * math.log2(0.25))
    assert s.entropy("codes", 2) == pytest.approx(h_cr0, abs=1e-12) and s.entropy(1, 2) == pytest.approx(2.0, abs=1e-12)
    assert s.raw_bits_per_pixel == (64 * 4 + 16 * 3 + 16 * 2) / 64
    assert s.bits_per_pixel(0) == pytest.approx((64 * 4 + 0 + 16 * h_cr0) / 64, abs=1e-12)
    assert s.bits_per_pixel(1) == pytest.approx((0 + 16 * h_cb1 + 16 * 2) / 64, abs=1e-12)
    assert s.bits_per_pixel("best") == pytest.approx((0 + 0 + 16 * h_cr0) / 64, abs=1e-12)
    assert s.bits_per_pixel("best") <= min(s.bits_per_pixel(0), s.bits_per_pixel(1), s.raw_bits_per_pixel)
    # 16 * 0.8113 = 12.98 bits -> 2 bytes; 256 + 12.98 bits -> 34 bytes: rounded up
    assert s.ideal_bytes("best") == 2 and s.ideal_bytes(0) == 34 and s.ideal_bytes(1) == math.ceil((16 * h_cb1 + 32) / 8)
    assert s == _stats([[4] * 16, [16], [12, 4]], [[0, 64], [1, 15], [4, 4, 4, 4]], (4, 3, 2), 64)
    assert s != _stats([[4] * 16, [16], [12, 4]], [[0, 64], [1, 15], [4, 4, 4, 4]], (4, 3, 2), 65)
    assert s != _stats([[4] * 16, [16], [4, 12]], [[0, 64], [1, 15], [4, 4, 4, 4]], (4, 3, 2), 64)
    assert s != csic.Distortion([0] * 6, 64)
    assert repr(s).startswith("CodeStats(samples=(64, 16, 16), bits=(4, 3, 2), pixels=64, raw=5.2500, ")
    assert csic.CodeStats.KINDS == ("codes", "residuals") and csic.CodeStats.PLANES == ("Y", "Cb", "Cr")
    # an empty plane: H = 0, nothing to pay
    e = _stats([[8], [], []], [[8], [], []], (1, 1, 1), 8)
    assert e.samples == (8, 0, 0) and e.entropy(0, 1) == 0.0 and e.bits_per_pixel(0) == 0.0 and e.ideal_bytes("best") == 0
    with pytest.raises(ValueError):
        csic.CodeStats(np.zeros((2, 3, 256)), (8, 8), 4)


def test_a_natural_image_carries_less_than_its_bit_planes(oracle):
    """in128.png at 4:2:0, 6 / 5 / 5: neighbouring luma samples are close, so the left predictor's residuals are cheaper than the codes,
    and the best per-plane choice is below the raw rate."""
    rgb = load_png_rgb(os.path.join(GOLDEN, "inputs", "in128.png"))
    H, W = rgb.shape[:2]
    bits = (6, 5, 5)
    hist = oracle_code_stats(oracle, oracle.rgb_to_argb(rgb), W, H, 2, 0, bits)
    s = csic.CodeStats(hist, bits, W * H)
    assert s.samples == (W * H, W * H // 4, W * H // 4)
    assert s.raw_bits_per_pixel == 6 + 2.5
    assert s.entropy(1, "Y") < s.entropy(0, "Y") <= 6
    assert s.bits_per_pixel("best") < s.raw_bits_per_pixel
    assert s.bits_per_pixel("best") <= min(s.bits_per_pixel(0), s.bits_per_pixel(1))
    assert s.ideal_bytes("best") == math.ceil(s.total_bits("best") / 8) <= s.ideal_bytes(0)


# ---- refusals that need no device --------------------------------------------------------------
def test_arguments_are_checked_before_any_device_is_touched():
    """NULL arguments, the source format, the frame count and the alignments are judged before the plan is read and before any HIP
    call, so a machine without a GPU -- where no plan can exist -- answers them too.  `standin` is zeroed memory in a plan's place: a
    refused call never looks at it, and the two questions that need no device read nothing but its (zero) tuning knobs."""
    L = N.lib()
    standin = C.create_string_buffer(4096)
    raw = C.create_string_buffer(1024 + 256)
    base = (C.addressof(raw) + 255) & ~255
    src, hist = C.c_void_p(base), C.c_void_p(base + 512)
    assert L.csic_code_stats_device(None, src, N.FMT_PLANAR, 1, hist, None) == N.EINVAL_NULL
    assert L.csic_code_stats_device(standin, None, N.FMT_PLANAR, 1, hist, None) == N.EINVAL_NULL
    assert L.csic_code_stats_device(standin, src, N.FMT_PLANAR, 1, None, None) == N.EINVAL_NULL
    assert L.csic_code_stats_host(None, src, 256, N.FMT_PLANAR, 1, hist) == N.EINVAL_NULL
    assert L.csic_code_stats_host(standin, None, 256, N.FMT_PLANAR, 1, hist) == N.EINVAL_NULL
    assert L.csic_code_stats_host(standin, src, 256, N.FMT_PLANAR, 1, None) == N.EINVAL_NULL
    for fmt in (N.FMT_ARGB8888, N.FMT_YCBCR888X, 4, -1):
        assert L.csic_code_stats_device(standin, src, fmt, 1, hist, None) == N.EINVAL_FORMAT
        assert L.csic_code_stats_host(standin, src, 256, fmt, 1, hist) == N.EINVAL_FORMAT
        assert L.csic_code_stats_kernel_name(standin, fmt) == b""
        assert L.csic_code_stats_block_samples(standin, fmt, C.byref(C.c_int64())) == N.EINVAL_FORMAT
    for fmt in (N.FMT_PLANAR, N.FMT_PLANAR_BITS):
        for nframes in (0, -3, 65536):
            assert L.csic_code_stats_device(standin, src, fmt, nframes, hist, None) == N.EINVAL_SIZE
            assert L.csic_code_stats_host(standin, src, 256, fmt, nframes, hist) == N.EINVAL_SIZE
        assert L.csic_code_stats_device(standin, C.c_void_p(base + 128), fmt, 1, hist, None) == N.EINVAL_SIZE
        assert L.csic_code_stats_device(standin, C.c_void_p(base + 16), fmt, 1, hist, None) == N.EINVAL_SIZE
        assert L.csic_code_stats_device(standin, src, fmt, 1, C.c_void_p(base + 512 + 4), None) == N.EINVAL_SIZE
        assert b"aligned" in L.csic_last_error()
    # the two questions that need no device
    b = C.c_int64()
    assert L.csic_code_stats_block_samples(None, N.FMT_PLANAR, C.byref(b)) == N.EINVAL_NULL
    assert L.csic_code_stats_block_samples(standin, N.FMT_PLANAR, None) == N.EINVAL_NULL
    for fmt in (N.FMT_PLANAR, N.FMT_PLANAR_BITS):
        b.value = 0
        assert L.csic_code_stats_block_samples(standin, fmt, C.byref(b)) == N.OK
        assert b.value > 0 and b.value % (32 * 64) == 0 and b.value < 2 ** 32
    assert L.csic_code_stats_kernel_name(None, N.FMT_PLANAR) == b""
    assert L.csic_code_stats_kernel_name(standin, N.FMT_PLANAR).startswith(b"k_cstat_bytes")
    assert (N.STATS_KINDS, N.STATS_PLANES, N.STATS_BINS) == (KINDS, PLANES, BINS)
    # and a plan itself is what a machine without a device cannot have
    if L.csic_device_count() < 1:
        h = C.c_void_p()
        assert L.csic_plan_create(C.byref(_c_params(16, 16, 2, 0, (6, 5, 5), 1, CSQ)), 0, C.byref(h)) == N.ENODEVICE


# ---- the inspect subcommand --------------------------------------------------------------------
def test_inspect_prints_the_header_of_a_container_written_on_the_cpu(oracle, tmp_path, capsys):
    from csic_amd.app import main
    rng = np.random.default_rng(7800)
    W, H, bits = 40, 12, (6, 5, 5)
    cp = _c_params(W, H, 2, 0, bits, 2, CSQ)
    lay = _layout(cp)
    frames = []
    for _ in range(2):
        planes = oracle_planes(oracle, rng.integers(0, 1 << 32, W * H, dtype=np.uint32), W, H, 2, 0, bits, 2)
        frames.append(_frame_buffer(lay, [pack_codes(v, q) for v, q in zip(planes, bits)], 0))
    path = str(tmp_path / "x.csic")
    csic.write_container(path, cp, np.stack(frames))
    assert main(["inspect", "--input", path]) == 0
    out = capsys.readouterr().out
    assert f"Image: {W}x{H}, chroma 4:2:0, bits Y/Cb/Cr 6/5/5, factor 2" in out
    assert f"Frames: 2, payload bytes per frame: {lay.payload_bytes}" in out
    if N.lib().csic_device_count() < 1:
        assert "[ERROR] No code statistics:" in out and "no HIP device" in out and "Frame 0:" not in out
    else:
        assert "Frame 1:" in out and "best" in out
    assert main(["inspect", "--input", str(tmp_path / "missing.csic")]) == 1
    assert main(["inspect"]) == 2
