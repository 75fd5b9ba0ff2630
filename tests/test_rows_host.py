"""The row-prediction layer on the host (csic_rows_layout_of, csic_rows_host, csic_unrows_host; include/csic.h) without a GPU, against
the numpy statement of tests/rows_ref.py: difference frames and maps byte for byte on the header's worked vectors, random parameter
sets, planes built to order (every group up, every group left, constant, alternating choices, the wrap, a ragged last group) at the
widths 32, 33, 63, 64, 95 and 20 (K = 0: the identity) and at heights that give one band, exactly two and two and a part, every q from
1 to 8; the inverse apart and in place, the canaries outside the payload ranges and behind map_bytes, and every refusal with its
status."""
import ctypes as C

import numpy as np
import pytest

from delta_ref import frame_buffers, map_buffers, ref_map_layout
from rows_ref import BAND, ref_constants, ref_rows, ref_unrows
from test_container import CANARY, CSQ, _c_params, _layout, _random_sets
from test_pack_host import codes_of

import csic_amd as csic

N = csic._native
WIDTHS = (32, 33, 63, 64, 95, 20)


def lib_rows(cp, frames, fill=CANARY):
    """csic_rows_host on frame buffers (nframes, frame_bytes) -> (diff, maps): destinations pre-filled with `fill`."""
    ml = csic.rows_layout(cp)
    src = np.ascontiguousarray(frames)
    diff = np.full_like(src, fill)
    maps = np.full((src.shape[0], ml.map_stride), fill, dtype=np.uint8)
    N.check(N.lib().csic_rows_host(C.byref(cp), src.ctypes.data_as(C.c_void_p), src.shape[0], diff.ctypes.data_as(C.c_void_p), maps.ctypes.data_as(C.c_void_p)))
    return diff, maps


def lib_unrows(cp, diff, maps, fill=CANARY, in_place=False):
    out = diff if in_place else np.full_like(diff, fill)
    N.check(N.lib().csic_unrows_host(C.byref(cp), diff.ctypes.data_as(C.c_void_p), maps.ctypes.data_as(C.c_void_p), diff.shape[0], out.ctypes.data_as(C.c_void_p)))
    return out


def plane_widths(cp):
    g = _layout(cp).geometry
    return [g.y_width, g.chroma_width, g.chroma_width]


def check_frames(cp, frames, bits, tag=None):
    """Frames (three planes of codes each) through the host codec against the numpy statement.  -> (diffs, maps, ts) per frame."""
    lay, ml = _layout(cp), csic.rows_layout(cp)
    widths = plane_widths(cp)
    G, off, mb, stride = ref_map_layout([c.size for c in frames[0]])
    assert (list(ml.groups), list(ml.map_offset), ml.map_bytes, ml.map_stride) == (G, off, mb, stride), tag
    assert list(ml.width) == widths and [(k, s) for k, s in zip(ml.k, ml.band)] == [ref_constants(w) for w in widths], tag
    ref = [ref_rows(f, widths, bits) for f in frames]
    diffs, maps, ts = [r[0] for r in ref], [r[1] for r in ref], [r[2] for r in ref]
    src = frame_buffers(lay, frames, bits, CANARY)
    keep = src.copy()
    want_d, want_m = frame_buffers(lay, diffs, bits, CANARY), map_buffers(maps, stride, CANARY)
    got_d, got_m = lib_rows(cp, src)
    assert np.array_equal(src, keep), tag                                      # the source is only read
    assert np.array_equal(got_d, want_d), tag                                  # the difference frames, and the canaries around them
    assert np.array_equal(got_m, want_m), tag                                  # the maps, and the canaries behind map_bytes
    assert np.array_equal(lib_unrows(cp, got_d, got_m), src), tag              # the payload ranges restored, canaries untouched
    work = got_d.copy()
    assert np.array_equal(lib_unrows(cp, work, got_m, in_place=True), src), tag
    for d, m, f in zip(diffs, maps, frames):                                   # the numpy inverse agrees
        assert all(np.array_equal(x, y) for x, y in zip(ref_unrows(d, m, widths, bits), f)), tag
    return diffs, maps, ts


def _params(W, H, bits):
    """W x H, 4:4:4, factor 1: every plane has W x H samples in rows of W."""
    return _c_params(W, H, 4, 4, bits, 1, CSQ)


def _y_only(x, q):
    z = np.zeros(len(x), dtype=np.int64)
    return [[np.array(x, dtype=np.int64), z, z]]


def test_worked_vectors():
    """The vectors of include/csic.h: the Y plane's bytes of the difference frame and the Y section of the map."""
    ramp = [1, 2, 3, 4, 5, 6, 7, 0] * 4
    w33 = [5 * (i % 33) % 8 for i in range(66)]
    for x, W, H, q, want_d, want_m in (
            (ramp + ramp, 32, 2, 3, "d1581f" * 4 + "00" * 12, "02000000"),                                  # a row repeated
            ([0] * 63 + [1], 32, 2, 3, "00" * 23 + "20", "00000000"),                                        # a tie is 0
            ([7, 3] * 16 + [0, 4] * 16, 32, 2, 3, "573817" * 4 + "d1581f" * 4, "03000000"),                  # the wrap
            (w33, 33, 2, 3, "e8ad85cce417" * 2 + "00" * 13, "07000000")):                                    # delta = 1
        cp = _params(W, H, (q, q, q))
        lay = _layout(cp)
        _, maps, _ = check_frames(cp, _y_only(x, q), (q, q, q))
        d, m = lib_rows(cp, frame_buffers(lay, _y_only(x, q), (q, q, q), 0), fill=0)
        assert d[0, lay.y_offset:lay.y_offset + lay.y_bytes].tobytes().hex() == want_d
        assert m[0, :4].tobytes().hex() == want_m and maps[0][:4].hex() == want_m
    # the ragged group: the header's numbers through the numpy statement (no frame has a plane of 34 samples in rows of 32), and a
    # ragged plane through the library: 95 x 3 has 285 samples, the last group 29
    from rows_ref import ref_rows_plane
    d, t = ref_rows_plane(np.array([1, 2, 3, 0] * 8 + [1, 2]), 32, 2)
    assert t.tolist() == [True, True] and d.tolist() == [1, 3, 2, 2, 3, 1, 0, 0] * 4 + [0, 0]
    rng = np.random.default_rng(23000)
    x = rng.integers(0, 4, 95 * 3)
    x[95:190] = x[:95]
    x[190:] = x[:95]
    diffs, _, ts = check_frames(_params(95, 3, (2, 2, 2)), _y_only(x, 2), (2, 2, 2))
    assert ts[0][0][8] and not diffs[0][0][256:].any()                         # the ragged group is taken from above: u = 0


def test_random_sets_match_the_reference_byte_for_byte(oracle):
    seen = set()
    for i, (W, H, a, b, bits, f, op, rounding, avg, _, rng) in enumerate(_random_sets(36, 23100)):
        W, H = 2 * W + 20, H + 8                                               # rows of up to 212 samples: K = 0 .. 6
        smooth = (np.cumsum(rng.integers(-2, 3, W)).astype(np.uint32) % 256)[None, :] + (np.arange(H, dtype=np.uint32) // 3)[:, None]
        argb = ((smooth % 256) * np.uint32(0x010101)).reshape(-1) ^ (rng.integers(0, 1 << 32, W * H, dtype=np.uint32) & np.uint32(0x00010307))
        frames = [codes_of(oracle, W, H, a, b, bits, f, op, rounding, avg, argb),
                  codes_of(oracle, W, H, a, b, bits, f, op, rounding, avg, rng.integers(0, 1 << 32, W * H, dtype=np.uint32))]
        cp = _c_params(W, H, a, b, bits, f, op, rounding, avg)
        _, _, ts = check_frames(cp, frames[:1 + i % 2], bits, (W, H, a, b, bits, f, op, rounding, avg))
        seen |= {bool(v) for fr in ts for t in fr for v in (t.any(), t.all())}
    assert seen == {False, True}


def _to_order(W, H, q, kind, rng):
    """A plane of W x H codes whose choices are known beforehand."""
    top = (1 << q) - 1
    row = rng.integers(0, top + 1, W)
    if kind == "up":                       # every row the first one: u = 0 wherever there is a reference
        return np.tile(row, H)
    if kind == "left":                     # constant along a row, the rows unrelated: left costs 0 inside a group
        return np.repeat(rng.permutation(H * 7 + 3)[:H] % (top + 1), W)
    if kind == "constant":
        return np.full(W * H, top // 2)
    if kind == "wrap":                     # 2^q - 1 and 2^q - 2 above 0 and 2^q - 1: u = 1 everywhere
        r = np.where(np.arange(W) % 2 == 0, top, top - (top > 0))
        return np.concatenate([(r + k) % (top + 1) for k in range(H)])
    raise AssertionError(kind)


@pytest.mark.parametrize("W", WIDTHS)
def test_planes_built_to_order(W):
    """Heights: one band, exactly two bands, two bands and a part.  A band is 16 K groups = 512 K samples: with w = 32 K + delta, H
    rows are H w samples."""
    rng = np.random.default_rng(23200 + W)
    K, S = ref_constants(W)
    heights = (3, 16, 33) if K == 0 else (BAND - 1, -(-2 * S // W) if 2 * S % W else 2 * S // W, 2 * S // W + 5)
    for q in range(1, 9):
        bits = (q, q, q)
        for H in heights:
            cp = _params(W, H, bits)
            planes = {kind: _to_order(W, H, q, kind, rng) for kind in ("up", "left", "constant", "wrap")}
            frames = [[planes["up"], planes["left"], planes["constant"]], [planes["wrap"], rng.integers(0, 1 << q, W * H), planes["up"][::-1].copy()]]
            diffs, maps, ts = check_frames(cp, frames, bits, (W, H, q))
            if K == 0:                                                         # the identity, and a map of zeros
                assert not any(t.any() for fr in ts for t in fr)
                assert all(np.array_equal(d, x) for fd, fx in zip(diffs, frames) for d, x in zip(fd, fx))
                continue
            assert not ts[0][1].any() and not ts[0][2].any()                   # left, and constant: all ties
            i = np.arange(W * H)
            has_ref = ((i - W >= S * (i // S)).reshape(-1)[: W * H // 32 * 32].reshape(-1, 32)[:, 1:]).all(axis=1)
            busy = np.array([len(set(g.tolist())) > 1 for g in planes["up"][: W * H // 32 * 32].reshape(-1, 32)])
            assert ts[0][0][: has_ref.size][has_ref & busy].all()              # up wherever the whole group has its references


@pytest.mark.parametrize("q", range(1, 9))
def test_alternating_choices_give_map_dwords_of_0x55555555(q):
    """w = 32: a group is a row.  Even rows are 0,1,0,1,..: left costs 16 fold(1) + 15 fold(-1), above a row of zeros -- or at a
    band's start, above nothing -- up costs 16 fold(1), which is less.  Odd rows are all zero: left costs 0, a tie at worst.  So the
    choices alternate group by group from group 0 on, through four bands."""
    W, H = 32, 64
    x = np.where(np.arange(H)[:, None] % 2 == 0, np.arange(W)[None, :] % 2, 0).reshape(-1)
    z = np.zeros(W * H, dtype=np.int64)
    _, maps, ts = check_frames(_params(W, H, (q, q, q)), [[x, z, x]], (q, q, q))
    assert np.array_equal(ts[0][0], np.arange(H) % 2 == 0) and not ts[0][1].any()
    assert np.frombuffer(maps[0], dtype="<u4").tolist() == [0x55555555] * 2 + [0] * 2 + [0x55555555] * 2


def _status(fn, *args):
    st = fn(*args)
    assert st == N.OK or N.lib().csic_last_error().decode() != ""
    return st


def test_refusals_and_a_refused_call_writes_nothing():
    L = N.lib()
    W, H, bits = 40, 10, (5, 4, 3)                                             # 4:2:0: Y rows of 40 (K = 1), chroma rows of 20 (K = 0)
    cp = _c_params(W, H, 2, 0, bits, 1, CSQ)
    lay, ml = _layout(cp), csic.rows_layout(cp)
    assert list(ml.k) == [1, 0, 0] and list(ml.band) == [512, 0, 0]
    rng = np.random.default_rng(23400)
    ns = [W * H, W * H // 4, W * H // 4]
    frames = [[np.tile(rng.integers(0, 1 << q, n // (H if p == 0 else H // 2)), H if p == 0 else H // 2) for p, (q, n) in enumerate(zip(bits, ns))] for _ in range(3)]
    src = frame_buffers(lay, frames, bits, CANARY)
    diff, maps = lib_rows(cp, src)
    assert maps[:, :ml.map_bytes].any()
    out = np.full_like(src, 0x5A)
    mo = np.full_like(maps, 0x5A)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert _status(L.csic_rows_layout_of, None, C.byref(ml)) == N.EINVAL_NULL
    assert _status(L.csic_rows_layout_of, C.byref(cp), None) == N.EINVAL_NULL
    for args in ((None, p(src), 3, p(out), p(mo)), (C.byref(cp), None, 3, p(out), p(mo)), (C.byref(cp), p(src), 3, None, p(mo)), (C.byref(cp), p(src), 3, p(out), None)):
        assert _status(L.csic_rows_host, *args) == N.EINVAL_NULL
    for args in ((None, p(diff), p(maps), 3, p(out)), (C.byref(cp), None, p(maps), 3, p(out)), (C.byref(cp), p(diff), None, 3, p(out)), (C.byref(cp), p(diff), p(maps), 3, None)):
        assert _status(L.csic_unrows_host, *args) == N.EINVAL_NULL
    for nf in (0, -1, 65536):
        assert _status(L.csic_rows_host, C.byref(cp), p(src), nf, p(out), p(mo)) == N.EINVAL_SIZE
        assert _status(L.csic_unrows_host, C.byref(cp), p(diff), p(maps), nf, p(out)) == N.EINVAL_SIZE
    # overlap: forward not even in place; inverse in place only
    big = np.full((4, lay.frame_bytes), CANARY, dtype=np.uint8)
    big[:3] = src
    keep = big.copy()
    assert _status(L.csic_rows_host, C.byref(cp), p(big), 3, p(big), p(mo)) == N.EINVAL_SIZE
    assert _status(L.csic_rows_host, C.byref(cp), p(big), 3, p(big[1:]), p(mo)) == N.EINVAL_SIZE
    assert _status(L.csic_unrows_host, C.byref(cp), p(big), p(maps), 3, p(big[1:])) == N.EINVAL_SIZE
    assert _status(L.csic_rows_host, C.byref(cp), p(big), 3, p(out), p(big[2:])) == N.EINVAL_SIZE      # the maps inside the frames
    assert np.array_equal(big, keep)
    bad = _c_params(W, H, 2, 0, bits, 1, CSQ)
    bad.in_format = N.FMT_YCBCR888X
    assert _status(L.csic_rows_host, C.byref(bad), p(src), 3, p(out), p(mo)) == N.EINVAL_FORMAT
    bad = _c_params(W, H, 2, 0, (5, 9, 3), 1, CSQ)
    assert _status(L.csic_unrows_host, C.byref(bad), p(diff), p(maps), 3, p(out)) == N.EINVAL_BITS
    assert np.all(out == 0x5A) and np.all(mo == 0x5A)
    # damaged maps: Y has 13 groups (bit 13 is padding); the chroma planes have K = 0: any bit of their sections
    for frame, byte, bit in ((1, ml.map_offset[0] + 1, 5), (2, ml.map_offset[0] + 3, 7), (0, ml.map_offset[1], 0), (2, ml.map_offset[2], 2)):
        m = maps.copy()
        m[frame, byte] |= 1 << bit
        assert _status(L.csic_unrows_host, C.byref(cp), p(diff), p(m), 3, p(out)) == N.EFORMAT
        assert np.all(out == 0x5A)
        with pytest.raises(csic.CsicIOError):
            csic.unrows_host(cp, diff, m)
    # a real bit flipped decodes, to another frame that goes through the layer again
    m = maps.copy()
    m[1, 0] ^= 2
    other = lib_unrows(cp, diff, m)
    assert not np.array_equal(other, src)
    d2, m2 = lib_rows(cp, other)
    assert np.array_equal(lib_unrows(cp, d2, m2), other)
    # the Python layer
    d3, m3 = csic.rows_host(cp, src)
    assert np.array_equal(m3[:, :ml.map_bytes], maps[:, :ml.map_bytes]) and np.array_equal(csic.unrows_host(cp, d3, m3), lib_unrows(cp, diff, maps, fill=0))
    with pytest.raises(csic.IllegalArgumentException):
        csic.rows_host(cp, src[:, :-1])
