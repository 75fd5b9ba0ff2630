"""The temporal layer on the host (csic_delta_layout_of, csic_delta_host, csic_undelta_host; include/csic.h) without a GPU, against the
numpy statement of tests/delta_ref.py: difference frames and maps byte for byte on the header's worked vectors, random parameter sets,
planes around a group's and a map dword's edge, constant, identical and noise frames, the wrap and the tie; the inverse, the canaries
outside the payload ranges and behind map_bytes, the in-place form and every refusal with its status."""
import ctypes as C

import numpy as np
import pytest

from delta_ref import frame_buffers, map_buffers, ref_delta, ref_map_layout, ref_undelta
from test_container import CANARY, CSQ, _c_params, _layout, _random_sets
from test_pack_host import codes_of

import csic_amd as csic

N = csic._native


def lib_delta(cp, frames, gop, fill=CANARY, in_place=False):
    """csic_delta_host on frame buffers (nframes, frame_bytes) -> (diff, maps): destinations pre-filled with `fill`."""
    ml = csic.delta_layout(cp)
    src = np.ascontiguousarray(frames)
    diff = src if in_place else np.full_like(src, fill)
    maps = np.full((src.shape[0], ml.map_stride), fill, dtype=np.uint8)
    N.check(N.lib().csic_delta_host(C.byref(cp), src.ctypes.data_as(C.c_void_p), src.shape[0], gop, diff.ctypes.data_as(C.c_void_p),
                                    maps.ctypes.data_as(C.c_void_p)))
    return diff, maps


def lib_undelta(cp, diff, maps, gop, fill=CANARY, in_place=False):
    out = diff if in_place else np.full_like(diff, fill)
    N.check(N.lib().csic_undelta_host(C.byref(cp), diff.ctypes.data_as(C.c_void_p), maps.ctypes.data_as(C.c_void_p), diff.shape[0], gop,
                                      out.ctypes.data_as(C.c_void_p)))
    return out


def check_sequence(cp, frames, bits, gop, tag=None):
    """A sequence of frames (three planes of codes each) through the host codec against the numpy statement.  -> (diffs, maps, ts)."""
    lay, ml = _layout(cp), csic.delta_layout(cp)
    ns = [c.size for c in frames[0]]
    G, off, mb, stride = ref_map_layout(ns)
    assert (list(ml.groups), list(ml.map_offset), ml.map_bytes, ml.map_stride) == (G, off, mb, stride), tag
    diffs, maps, ts = ref_delta(frames, bits, gop)
    src = frame_buffers(lay, frames, bits, CANARY)
    keep = src.copy()
    want_d, want_m = frame_buffers(lay, diffs, bits, CANARY), map_buffers(maps, stride, CANARY)
    got_d, got_m = lib_delta(cp, src, gop)
    assert np.array_equal(src, keep), tag                                      # the source is only read
    assert np.array_equal(got_d, want_d), tag                                  # the difference frames, and the canaries around them
    assert np.array_equal(got_m, want_m), tag                                  # the maps, and the canaries behind map_bytes
    back = lib_undelta(cp, got_d, got_m, gop)
    assert np.array_equal(back, src), tag                                      # the payload ranges restored, canaries untouched
    # in place, both directions
    work = src.copy()
    d2, m2 = lib_delta(cp, work, gop, in_place=True)
    assert d2 is work and np.array_equal(work, want_d) and np.array_equal(m2, want_m), tag
    assert np.array_equal(lib_undelta(cp, work, m2, gop, in_place=True), src), tag
    # the numpy inverse agrees
    for a, b in zip(ref_undelta(diffs, maps, bits, gop), frames):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), tag
    return diffs, maps, ts


def _line_params(n, bits):
    """n x 1, 4:4:4, factor 1: every plane has exactly n samples."""
    return _c_params(n, 1, 4, 4, bits, 1, CSQ)


def _one_plane(c, r, q):
    """Two frames whose Y planes are r then c, the chroma planes zero."""
    z = np.zeros(len(c), dtype=np.int64)
    return [[np.array(r, dtype=np.int64), z, z], [np.array(c, dtype=np.int64), z, z]]


def test_worked_vectors():
    """The vectors of include/csic.h: the Y plane's bytes of the difference frame and the Y section of the map."""
    for c, r, q, want_d, want_m in (([1, 2, 3, 4, 5, 6, 7, 0], [1, 2, 3, 4, 5, 6, 7, 0], 3, "000000", "01000000"),      # identical frames
                                    ([0, 1], [1, 1], 3, "08", "00000000"),                                               # a tie is intra
                                    ([0, 4, 0], [7, 3, 7], 3, "4900", "01000000")):                                      # the wrap
        cp = _line_params(len(c), (q, q, q))
        lay = _layout(cp)
        frames = _one_plane(c, r, q)
        diffs, maps, ts = check_sequence(cp, frames, (q, q, q), 2)
        d, m = lib_delta(cp, frame_buffers(lay, frames, (q, q, q), 0), 2, fill=0)
        assert d[1, lay.y_offset:lay.y_offset + lay.y_bytes].tobytes().hex() == want_d
        assert m[1, :4].tobytes().hex() == want_m and maps[1][:4].hex() == want_m and not m[0].any()
    # the ragged group: q = 2, n = 34, samples 32 and 33 are group 1
    rng = np.random.default_rng(16000)
    c, r = rng.integers(0, 4, 34), rng.integers(0, 4, 34)
    c[32:], r[32:] = (3, 0), (2, 3)
    diffs, maps, ts = check_sequence(_line_params(34, (2, 2, 2)), _one_plane(c, r, 2), (2, 2, 2), 2)
    assert ts[1][0][1] and diffs[1][0][32:].tolist() == [1, 1] and maps[1][0] & 2
    # a group of one sample costs 0 either way: always intra
    c, r = rng.integers(0, 4, 33), rng.integers(0, 4, 33)
    _, _, ts = check_sequence(_line_params(33, (2, 2, 2)), _one_plane(c, r, 2), (2, 2, 2), 2)
    assert not ts[1][0][1]


def test_random_sets_match_the_reference_byte_for_byte(oracle):
    seen = set()
    for i, (W, H, a, b, bits, f, op, rounding, avg, _, rng) in enumerate(_random_sets(30, 16100)):
        nframes = 1 + i % 5
        base = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        frames = []
        for k in range(nframes):
            argb = base.copy()
            if k % 2:                                           # every other frame: the one before with a part redrawn
                lo = int(rng.integers(0, W * H))
                argb[lo:lo + W * H // 3 + 1] = rng.integers(0, 1 << 32, argb[lo:lo + W * H // 3 + 1].size, dtype=np.uint32)
            elif k:
                base = argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32) & np.uint32(0xFF0F0F0F) | (base & np.uint32(0x00F0F0F0))
            frames.append(codes_of(oracle, W, H, a, b, bits, f, op, rounding, avg, argb))
        cp = _c_params(W, H, a, b, bits, f, op, rounding, avg)
        for gop in (1, 2, 3, nframes + 2):
            _, _, ts = check_sequence(cp, frames, bits, gop, (W, H, a, b, bits, f, op, rounding, avg, nframes, gop))
            seen |= {bool(t.any()) for fr in ts if fr for t in fr}
    assert seen == {False, True}


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000, 1025])
def test_planes_around_a_group_and_a_map_dword(n):
    """G = 1, 1, 1, 2, 32 (a map dword exactly full) and 33 (one bit into the next)."""
    rng = np.random.default_rng(16200 + n)
    for bits in ((1, 1, 1), (8, 8, 8), (6, 5, 5), (3, 3, 2)):
        first = [rng.integers(0, 1 << q, n) for q in bits]
        frames = [first]
        for k in range(1, 4):                                   # groups in turn: kept, redrawn, shifted by one code
            nxt = []
            for c, q in zip(frames[-1], bits):
                g = np.arange(n) // 32
                v = np.where(g % 3 == k % 3, rng.integers(0, 1 << q, n), c)
                nxt.append(np.where(g % 3 == (k + 1) % 3, (v + 1) % (1 << q), v))
            frames.append(nxt)
        for gop in (1, 2, 3, 9):
            check_sequence(_line_params(n, bits), frames, bits, gop, (n, bits, gop))


def test_constant_identical_and_noise_frames():
    rng = np.random.default_rng(16300)
    n, bits = 777, (7, 4, 2)
    cp = _line_params(n, bits)
    const = [[np.full(n, v % (1 << q), dtype=np.int64) for q in bits] for v in (0, 255, 37)]
    _, maps, _ = check_sequence(cp, const, bits, 3)
    assert not any(any(m) for m in maps)                        # constant frames cost 0 as they are: every group is a tie
    walk = [np.cumsum(rng.integers(-2, 3, n)) % (1 << q) for q in bits]
    _, maps, ts = check_sequence(cp, [walk] * 4, bits, 4)
    assert all(all(t.all() for t in fr) for fr in ts[1:])       # identical frames: every group that costs anything is inter
    noise = [[rng.integers(0, 1 << q, n) for q in bits] for _ in range(4)]
    check_sequence(cp, noise, bits, 2)
    # the wrap on every width: 0 over 2^q - 1, and back
    for q in range(1, 9):
        top = (1 << q) - 1
        r = np.where(np.arange(64) % 2 == 0, top, top - (top > 0)).astype(np.int64)
        c = np.where(np.arange(64) % 2 == 0, 0, top).astype(np.int64)
        check_sequence(_line_params(64, (q, q, q)), [[r] * 3, [c] * 3, [r] * 3], (q, q, q), 3)


def _status(fn, *args):
    st = fn(*args)
    assert st == N.OK or N.lib().csic_last_error().decode() != ""
    return st


def test_refusals_and_a_refused_call_writes_nothing():
    L = N.lib()
    n, bits = 100, (5, 4, 3)
    cp = _line_params(n, bits)
    lay, ml = _layout(cp), csic.delta_layout(cp)
    rng = np.random.default_rng(16400)
    frames = [[rng.integers(0, 1 << q, n) for q in bits] for _ in range(3)]
    src = frame_buffers(lay, frames, bits, CANARY)
    diff, maps = lib_delta(cp, src, 2)
    out = np.full_like(src, 0x5A)
    mo = np.full_like(maps, 0x5A)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    # the layout
    assert _status(L.csic_delta_layout_of, None, C.byref(ml)) == N.EINVAL_NULL
    assert _status(L.csic_delta_layout_of, C.byref(cp), None) == N.EINVAL_NULL
    # NULLs
    for args in ((None, p(src), 3, 2, p(out), p(mo)), (C.byref(cp), None, 3, 2, p(out), p(mo)), (C.byref(cp), p(src), 3, 2, None, p(mo)),
                 (C.byref(cp), p(src), 3, 2, p(out), None)):
        assert _status(L.csic_delta_host, *args) == N.EINVAL_NULL
    for args in ((None, p(diff), p(maps), 3, 2, p(out)), (C.byref(cp), None, p(maps), 3, 2, p(out)), (C.byref(cp), p(diff), None, 3, 2, p(out)),
                 (C.byref(cp), p(diff), p(maps), 3, 2, None)):
        assert _status(L.csic_undelta_host, *args) == N.EINVAL_NULL
    # nframes, gop
    for nf in (0, -1, 65536):
        assert _status(L.csic_delta_host, C.byref(cp), p(src), nf, 2, p(out), p(mo)) == N.EINVAL_SIZE
        assert _status(L.csic_undelta_host, C.byref(cp), p(diff), p(maps), nf, 2, p(out)) == N.EINVAL_SIZE
    for gop in (0, -3):
        assert _status(L.csic_delta_host, C.byref(cp), p(src), 3, gop, p(out), p(mo)) == N.EINVAL_SIZE
        assert _status(L.csic_undelta_host, C.byref(cp), p(diff), p(maps), 3, gop, p(out)) == N.EINVAL_SIZE
    # a partial overlap: the destination one frame into the source
    big = np.full((4, lay.frame_bytes), CANARY, dtype=np.uint8)
    big[:3] = src
    keep = big.copy()
    assert _status(L.csic_delta_host, C.byref(cp), p(big), 3, 2, p(big[1:]), p(mo)) == N.EINVAL_SIZE
    assert _status(L.csic_undelta_host, C.byref(cp), p(big), p(maps), 3, 2, p(big[1:])) == N.EINVAL_SIZE
    assert np.array_equal(big, keep)
    # parameters the container does not take
    bad = _c_params(n, 1, 4, 4, bits, 1, CSQ)
    bad.in_format = N.FMT_YCBCR888X
    assert _status(L.csic_delta_host, C.byref(bad), p(src), 3, 2, p(out), p(mo)) == N.EINVAL_FORMAT
    bad = _c_params(n, 1, 4, 4, (5, 9, 3), 1, CSQ)
    assert _status(L.csic_undelta_host, C.byref(bad), p(diff), p(maps), 3, 2, p(out)) == N.EINVAL_BITS
    assert np.all(out == 0x5A) and np.all(mo == 0x5A)
    # damaged maps: a padding bit (100 samples = 4 groups: bit 4 of a section is padding), a bit of a key frame's map
    for frame, byte, bit in ((1, ml.map_offset[0], 4), (1, ml.map_offset[2] + 3, 7), (0, ml.map_offset[1], 0), (2, 0, 1)):
        m = maps.copy()
        m[frame, byte] |= 1 << bit
        assert _status(L.csic_undelta_host, C.byref(cp), p(diff), p(m), 3, 2, p(out)) == N.EFORMAT
        assert np.all(out == 0x5A)
        with pytest.raises(csic.CsicIOError):
            csic.undelta_host(cp, diff, m, 2)
    # a real bit flipped decodes, to other frames that delta again
    m = maps.copy()
    m[1, 0] ^= 1
    other = lib_undelta(cp, diff, m, 2)
    assert not np.array_equal(other, src)
    d2, m2 = lib_delta(cp, other, 2)
    assert np.array_equal(lib_undelta(cp, d2, m2, 2), other)
    # the Python layer
    d3, m3 = csic.delta_host(cp, src, 2)
    assert np.array_equal(m3[:, :ml.map_bytes], maps[:, :ml.map_bytes]) and np.array_equal(csic.undelta_host(cp, d3, m3, 2), lib_undelta(cp, diff, maps, 2, fill=0))
    with pytest.raises(csic.IllegalArgumentException):
        csic.delta_host(cp, src[:, :-1], 2)
