"""The motion-compensated temporal layer on the host (csic_mc_layout_of, csic_mc_delta_host, csic_mc_undelta_host; include/csic.h)
without a GPU, against the numpy statement of tests/mc_ref.py: difference frames and maps -- tables and nibbles -- byte for byte on the
header's worked vectors, on planes built to order around a group's, a nibble dword's and a block's edge with contents that move, on
random parameter sets (chroma planes narrower than Y); the inverse, the canaries outside the payload ranges and behind map_bytes, every
refusal with its status, and range 0 against csic_delta_host.  The sequence builders here are also what tests/test_gpu_mc.py runs."""
import ctypes as C

import numpy as np
import pytest

from delta_ref import frame_buffers, map_buffers, ref_delta
from mc_ref import candidates, parse_map, ref_mc_delta, ref_mc_layout, ref_mc_undelta
from test_container import CANARY, CSQ, _c_params, _layout, _random_sets
from test_delta_host import lib_delta
from test_pack_host import codes_of

import csic_amd as csic

N = csic._native

TRIPLES = [(q, q, q) for q in range(1, 9)] + [(6, 5, 5), (5, 5, 3), (3, 3, 2)]
SMALL = ((1, 1), (31, 1), (33, 1), (8, 5), (16, 16), (16, 18), (32, 4), (100, 21))
LARGE = ((128, 64), (2731, 3), (200, 100))
CONTENTS = ("random", "identical", "wrap", "shift", "halves", "stripes")
MOST = 5


def plane_params(W, H, bits):
    """W x H, 4:4:4, factor 1: every plane has W H samples in rows of W."""
    return _c_params(W, H, 4, 4, bits, 1, CSQ)


def _moved(prev, disp, rng, q, redraw=0.0):
    """c_i = prev[clamp(i + disp_i)]; a share of the groups redrawn."""
    n = prev.size
    c = prev[np.clip(np.arange(n, dtype=np.int64) + disp, 0, n - 1)]
    if redraw:
        new = np.repeat(rng.random((n + 31) // 32) < redraw, 32)[:n]
        c = np.where(new, rng.integers(0, 1 << q, n), c)
    return c


def sequence(content, W, H, bits, R, rng, nframes=MOST):
    """`nframes` frames of three planes of W H codes whose contents move by vectors inside range max(R, 1)."""
    n = W * H
    if content == "random":
        return [[rng.integers(0, 1 << q, n) for q in bits] for _ in range(nframes)]
    if content == "identical":
        one = [np.cumsum(rng.integers(-1, 2, n)) % (1 << q) for q in bits]
        return [one] * nframes
    if content == "wrap":                                   # 0 over 2^q - 1 in every other sample, and back, one sample along
        even = np.arange(n) % 2 == 0
        tops = [(1 << q) - 1 for q in bits]
        r = [np.where(even, t, max(t - 1, 0)).astype(np.int64) for t in tops]
        c = [np.where(even, 0, t).astype(np.int64) for t in tops]
        return ([r, c] * nframes)[:nframes]
    cand = candidates(max(R, 1))[1:]
    frames = [[rng.integers(0, 1 << q, n) for q in bits]]
    for k in range(1, nframes):
        if content == "shift":                              # the whole plane by one known vector
            dy, dx = cand[int(rng.integers(len(cand)))]
            disp = np.full(n, dy * W + dx, dtype=np.int64)
        elif content == "halves":                           # two halves with different vectors
            (ay, ax), (by, bx) = cand[int(rng.integers(len(cand)))], cand[int(rng.integers(len(cand)))]
            disp = np.where(np.arange(n) < n // 2, ay * W + ax, by * W + bx).astype(np.int64)
        else:                                               # 20 stripes, 20 distinct vectors (as many as the range has): the cap, the ties
            pick = rng.permutation(len(cand))[:20]
            s = np.array([cand[i][0] * W + cand[i][1] for i in pick], dtype=np.int64)
            # stripes of equal length in pairs: equal votes, the rank decides
            disp = s[np.minimum(np.arange(n) * len(s) // max(n, 1), len(s) - 1)]
        frames.append([_moved(c, disp, rng, q, 0.2 if content == "halves" else 0.0) for c, q in zip(frames[-1], bits)])
    return frames


def lib_mc_delta(cp, frames, gop, R, fill=CANARY):
    """csic_mc_delta_host on frame buffers (nframes, frame_bytes) -> (diff, maps): destinations pre-filled with `fill`."""
    ml = csic.mc_layout(cp)
    src = np.ascontiguousarray(frames)
    diff = np.full_like(src, fill)
    maps = np.full((src.shape[0], ml.map_stride), fill, dtype=np.uint8)
    N.check(N.lib().csic_mc_delta_host(C.byref(cp), src.ctypes.data_as(C.c_void_p), src.shape[0], gop, R, diff.ctypes.data_as(C.c_void_p),
                                       maps.ctypes.data_as(C.c_void_p)))
    return diff, maps


def lib_mc_undelta(cp, diff, maps, gop, fill=CANARY):
    out = np.full_like(diff, fill)
    N.check(N.lib().csic_mc_undelta_host(C.byref(cp), diff.ctypes.data_as(C.c_void_p), maps.ctypes.data_as(C.c_void_p), diff.shape[0], gop,
                                         out.ctypes.data_as(C.c_void_p)))
    return out


def check_layout(ml, ns, widths):
    G, toff, off, mb, stride = ref_mc_layout(ns)
    assert (list(ml.groups), list(ml.width), list(ml.table_offset), list(ml.map_offset), ml.map_bytes, ml.map_stride) == (G, list(widths), toff, off, mb, stride)
    assert ml.workspace_frame_bytes >= 3 * 4 * 225
    return mb, stride


def check_sequence(cp, frames, bits, gop, R, tag=None):
    """A sequence of frames (three planes of codes each) through the host codec against the numpy statement.  -> (diffs, maps, info)."""
    lay, ml = _layout(cp), csic.mc_layout(cp)
    widths = [lay.geometry.y_width, lay.geometry.chroma_width, lay.geometry.chroma_width]
    _, stride = check_layout(ml, [c.size for c in frames[0]], widths)
    diffs, maps, info = ref_mc_delta(frames, bits, widths, gop, R)
    src = frame_buffers(lay, frames, bits, CANARY)
    keep = src.copy()
    want_d, want_m = frame_buffers(lay, diffs, bits, CANARY), map_buffers(maps, stride, CANARY)
    got_d, got_m = lib_mc_delta(cp, src, gop, R)
    assert np.array_equal(src, keep), tag                                      # the source is only read
    assert np.array_equal(got_m, want_m), tag                                  # the maps, and the canaries behind map_bytes
    assert np.array_equal(got_d, want_d), tag                                  # the difference frames, and the canaries around them
    assert np.array_equal(lib_mc_undelta(cp, got_d, got_m, gop), src), tag     # the payload ranges restored, canaries untouched
    for a, b in zip(ref_mc_undelta(diffs, maps, bits, gop), frames):           # the numpy inverse agrees
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), tag
    return diffs, maps, info


def _one_plane(c, r):
    """Two frames whose Y planes are r then c, the chroma planes zero."""
    z = np.zeros(len(c), dtype=np.int64)
    return [[np.array(r, dtype=np.int64), z, z], [np.array(c, dtype=np.int64), z, z]]


def test_candidates_are_ranked_as_the_header_says():
    assert candidates(0) == [(0, 0)]
    assert candidates(1) == [(0, 0), (-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1)]
    assert candidates(2)[5:8] == [(-2, 0), (-1, -1), (-1, 1)] and len(candidates(7)) == 225


@pytest.mark.parametrize("R", [1, 2, 7])
def test_the_library_ranks_the_candidates_the_same_way(R):
    """A plane built to order: every candidate is the only zero-cost predictor of six groups (three rows of two), so all get the same
    number of votes and the rank alone orders the table: the zero vector, then the 14 (range 1: all 8) non-zero candidates of lowest rank,
    in rank order."""
    K = candidates(R)
    W = 64
    which = np.repeat(np.arange(len(K)), 3)                  # the candidate of each row
    H = which.size + 2 * R
    rng = np.random.default_rng(18050 + R)
    r = rng.integers(0, 256, W * H)
    c = r.copy()
    for row, k in enumerate(which, start=R):
        at = np.arange(row * W, row * W + W)
        c[at] = r[np.clip(at + K[k][0] * W + K[k][1], 0, W * H - 1)]
    frames = [[r, r, r], [c, c, c]]
    cp = plane_params(W, H, (8, 8, 8))
    _, maps, info = check_sequence(cp, frames, (8, 8, 8), 2, R)
    _, got_m = lib_mc_delta(cp, frame_buffers(_layout(cp), frames, (8, 8, 8), 0), 2, R, fill=0)
    words = np.frombuffer(got_m[1, :64].tobytes(), dtype="<i4").tolist()
    n = min(len(K) - 1, 14)
    assert words[0] == 1 + n and words[1] == 0
    assert words[2:2 + n] == [dy * W + dx for dy, dx in K[1:1 + n]]              # the library's order is the header's rank order


def test_worked_vectors():
    """The vectors of include/csic.h: the Y plane of an 8 x 1 frame, q = 3: the table's words, the nibble section, the plane's bytes."""
    r = [1, 2, 3, 4, 5, 6, 7, 0]
    for c, R, table, section, want_d in (([1, 1, 2, 3, 4, 5, 6, 7], 1, [2, 0, -1], "02000000", "000000"),              # a pan
                                         ([1, 1, 2, 3, 4, 5, 6, 7], 0, [1, 0], "01000000", "f8ffff"),                  # the same without a range
                                         ([1] * 8, 1, [2, 0, -8], "00000000", "499224"),                               # clamping; a tie is intra
                                         (r, 1, [1, 0], "01000000", "000000")):                                        # identical frames
        cp = plane_params(8, 1, (3, 3, 3))
        lay, ml = _layout(cp), csic.mc_layout(cp)
        frames = _one_plane(c, r)
        diffs, maps, info = check_sequence(cp, frames, (3, 3, 3), 2, R)
        d, m = lib_mc_delta(cp, frame_buffers(lay, frames, (3, 3, 3), 0), 2, R, fill=0)
        assert d[1, lay.y_offset:lay.y_offset + lay.y_bytes].tobytes().hex() == want_d
        words = np.frombuffer(m[1, :64].tobytes(), dtype="<i4").tolist()
        assert words == table + [0] * (16 - len(table)) and info[1][0][0] == words
        assert m[1, ml.map_offset[0]:ml.map_offset[0] + 4].tobytes().hex() == section and not m[0].any()
    assert bytes(m[1, :12]).hex() == "01000000" + "00" * 8
    _, m = lib_mc_delta(cp, frame_buffers(lay, _one_plane([1, 1, 2, 3, 4, 5, 6, 7], r), (3, 3, 3), 0), 2, 1, fill=0)
    assert bytes(m[1, :12]).hex() == "0200000000000000ffffffff"


@pytest.mark.parametrize("W,H", SMALL + LARGE)
def test_planes_built_to_order_match_the_reference_byte_for_byte(W, H):
    rng = np.random.default_rng(18000 + 100 * W + H)
    small = (W, H) in SMALL
    seen = set()
    for i, bits in enumerate(TRIPLES if small else [(8, 8, 8), (6, 5, 5), (3, 3, 2), (1, 1, 1)]):
        cp = plane_params(W, H, bits)
        for j, content in enumerate(CONTENTS):
            R = ((0, 1, 2, 7) if small else (1, 2, 0))[(i + j) % (4 if small else 3)]
            nframes, gop = ((1, 1), (2, 2), (5, 3), (5, 7))[(i + 2 * j) % 4] if small else (2, 2)
            _, maps, info = check_sequence(cp, sequence(content, W, H, bits, R, rng, nframes), bits, gop, R, (W, H, bits, content, R, nframes, gop))
            seen |= {int(t[0]) for fr in info if fr for t, _ in fr}
    assert 1 in seen and (max(seen) > 1 or W * H == 1)


def test_twenty_stripes_fill_the_table_and_ties_go_by_rank():
    """20 distinct vectors of range 2 in stripes of equal length: 14 of them make the table, T = 15; the tied ones are in rank order."""
    W, H, bits, R = 64, 100, (8, 8, 8), 2
    rng = np.random.default_rng(18100)
    frames = sequence("stripes", W, H, bits, R, rng, 2)
    _, _, info = check_sequence(plane_params(W, H, bits), frames, bits, 2, R)
    table, nib = info[1][0]
    assert table[0] == 15 and table[1] == 0 and len(set(table[1:])) == 15 and nib.max() == 15
    # the votes counted again, group by group
    c, r = frames[1][0], frames[0][0]
    ss = [dy * W + dx for dy, dx in candidates(R)]
    votes = [0] * len(ss)
    for g in range(W * H // 32):
        at = np.arange(32 * g, 32 * g + 32)
        costs = []
        for s in ss:
            d = (c[at] - r[np.clip(at + s, 0, W * H - 1)]) % 256
            e = (d[1:] - d[:-1]) % 256
            costs.append(int(np.where(e < 128, 2 * e, 2 * (256 - e) - 1).sum()))
        votes[costs.index(min(costs))] += 1
    order = sorted((k for k in range(1, len(ss)) if votes[k]), key=lambda k: (-votes[k], k))
    assert len(order) == 20 and table[2:] == [ss[k] for k in order[:14]]
    assert len({votes[k] for k in order[:14]}) < 14                             # some are tied: the rank decided


def test_random_sets_match_the_reference_byte_for_byte(oracle):
    """Frames from the oracle's planar form: subsampled chroma planes have their own row width."""
    for i, (W, H, a, b, bits, f, op, rounding, avg, _, rng) in enumerate(_random_sets(24, 18200)):
        nframes, R = 1 + i % 4, (0, 1, 2, 3, 7)[i % 5]
        argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32).reshape(H, W)
        frames = []
        for k in range(nframes):                            # the picture panned by (k, 2 k), the edges repeated
            rows, cols = np.clip(np.arange(H) + k, 0, H - 1), np.clip(np.arange(W) + 2 * k, 0, W - 1)
            frames.append(codes_of(oracle, W, H, a, b, bits, f, op, rounding, avg, np.ascontiguousarray(argb[rows][:, cols]).reshape(-1)))
        cp = _c_params(W, H, a, b, bits, f, op, rounding, avg)
        for gop in (1, 2, nframes + 2):
            check_sequence(cp, frames, bits, gop, R, (W, H, a, b, bits, f, op, rounding, avg, nframes, gop, R))


def test_range_zero_makes_the_choices_of_csic_delta_host():
    rng = np.random.default_rng(18300)
    for (W, H), bits in zip(((33, 1), (16, 18), (100, 21), (200, 100)), ((3, 3, 2), (8, 8, 8), (6, 5, 5), (1, 1, 1))):
        cp = plane_params(W, H, bits)
        lay, ml, dl = _layout(cp), csic.mc_layout(cp), csic.delta_layout(cp)
        for content in ("halves", "identical", "random"):
            src = frame_buffers(lay, sequence(content, W, H, bits, 0, rng), bits, CANARY)
            for gop in (1, 3, 9):
                d0, m0 = lib_delta(cp, src, gop)
                d1, m1 = lib_mc_delta(cp, src, gop, 0)
                assert np.array_equal(d0, d1)
                for k in range(src.shape[0]):
                    for p, (table, nib) in enumerate(parse_map(m1[k, :ml.map_bytes], [W * H] * 3)):
                        G = dl.groups[p]
                        sec = m0[k, dl.map_offset[p]:dl.map_offset[p] + 4 * ((G + 31) // 32)]
                        assert np.array_equal(nib[:G], np.unpackbits(sec, bitorder="little")[:G])
                        assert table.tolist() == ([1] + [0] * 15 if k % gop else [0] * 16)


def _status(fn, *args):
    st = fn(*args)
    assert st == N.OK or N.lib().csic_last_error().decode() != ""
    return st


def test_refusals_and_a_refused_call_writes_nothing():
    L = N.lib()
    W, H, bits = 20, 5, (5, 4, 3)                            # 100 samples = 4 groups: nibbles 4 .. 7 of a section are padding
    cp = plane_params(W, H, bits)
    lay, ml = _layout(cp), csic.mc_layout(cp)
    rng = np.random.default_rng(18400)
    src = frame_buffers(lay, sequence("halves", W, H, bits, 2, rng, 3), bits, CANARY)
    diff, maps = lib_mc_delta(cp, src, 2, 2)
    out = np.full_like(src, 0x5A)
    mo = np.full_like(maps, 0x5A)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    # the layout
    assert _status(L.csic_mc_layout_of, None, C.byref(ml)) == N.EINVAL_NULL
    assert _status(L.csic_mc_layout_of, C.byref(cp), None) == N.EINVAL_NULL
    # NULLs
    for args in ((None, p(src), 3, 2, 2, p(out), p(mo)), (C.byref(cp), None, 3, 2, 2, p(out), p(mo)), (C.byref(cp), p(src), 3, 2, 2, None, p(mo)),
                 (C.byref(cp), p(src), 3, 2, 2, p(out), None)):
        assert _status(L.csic_mc_delta_host, *args) == N.EINVAL_NULL
    for args in ((None, p(diff), p(maps), 3, 2, p(out)), (C.byref(cp), None, p(maps), 3, 2, p(out)), (C.byref(cp), p(diff), None, 3, 2, p(out)),
                 (C.byref(cp), p(diff), p(maps), 3, 2, None)):
        assert _status(L.csic_mc_undelta_host, *args) == N.EINVAL_NULL
    # nframes, gop, range
    for nf in (0, -1, 65536):
        assert _status(L.csic_mc_delta_host, C.byref(cp), p(src), nf, 2, 2, p(out), p(mo)) == N.EINVAL_SIZE
        assert _status(L.csic_mc_undelta_host, C.byref(cp), p(diff), p(maps), nf, 2, p(out)) == N.EINVAL_SIZE
    for gop in (0, -3):
        assert _status(L.csic_mc_delta_host, C.byref(cp), p(src), 3, gop, 2, p(out), p(mo)) == N.EINVAL_SIZE
        assert _status(L.csic_mc_undelta_host, C.byref(cp), p(diff), p(maps), 3, gop, p(out)) == N.EINVAL_SIZE
    for R in (-1, 8, 100):
        assert _status(L.csic_mc_delta_host, C.byref(cp), p(src), 3, 2, R, p(out), p(mo)) == N.EINVAL_SIZE
    # in place is not allowed, nor a partial overlap, nor maps inside the frames
    big = np.full((4, lay.frame_bytes), CANARY, dtype=np.uint8)
    big[:3] = src
    keep = big.copy()
    assert _status(L.csic_mc_delta_host, C.byref(cp), p(big), 3, 2, 2, p(big), p(mo)) == N.EINVAL_SIZE
    assert _status(L.csic_mc_undelta_host, C.byref(cp), p(big), p(maps), 3, 2, p(big)) == N.EINVAL_SIZE
    assert _status(L.csic_mc_delta_host, C.byref(cp), p(big), 3, 2, 2, p(big[1:]), p(mo)) == N.EINVAL_SIZE
    assert _status(L.csic_mc_undelta_host, C.byref(cp), p(big), p(maps), 3, 2, p(big[1:])) == N.EINVAL_SIZE
    assert _status(L.csic_mc_delta_host, C.byref(cp), p(big), 1, 2, 2, p(out), p(big[0, 256:])) == N.EINVAL_SIZE
    assert np.array_equal(big, keep)
    # parameters the container does not take
    bad = plane_params(W, H, bits)
    bad.in_format = N.FMT_YCBCR888X
    assert _status(L.csic_mc_delta_host, C.byref(bad), p(src), 3, 2, 2, p(out), p(mo)) == N.EINVAL_FORMAT
    bad = plane_params(W, H, (5, 9, 3))
    assert _status(L.csic_mc_undelta_host, C.byref(bad), p(diff), p(maps), 3, 2, p(out)) == N.EINVAL_BITS
    assert np.all(out == 0x5A) and np.all(mo == 0x5A)
    # damaged maps.  Frame 1 is the delta frame; its table of plane 0 has T entries
    T = int(maps[1, 0])
    assert 1 <= T < 15 and not maps[1, 1:4].any()

    def word(m, frame, plane, t, v):
        m[frame, 64 * plane + 4 * t:64 * plane + 4 * t + 4] = np.frombuffer(np.array([v], dtype="<i4").tobytes(), dtype=np.uint8)

    def nibble(m, frame, plane, g, v):
        at = ml.map_offset[plane] + g // 2
        m[frame, at] = (int(m[frame, at]) & (0xF0 if g % 2 == 0 else 0x0F)) | (v << (4 * (g % 2)))

    damage = {"T above 15": lambda m: word(m, 1, 0, 0, 16), "T negative": lambda m: word(m, 1, 2, 0, -1),
              "a nibble above T": lambda m: nibble(m, 1, 0, 2, T + 1), "a nibble above T = 0": lambda m: (word(m, 1, 1, 0, 0), nibble(m, 1, 1, 0, 1)),
              "an unused word": lambda m: word(m, 1, 1, 15, 5), "the word behind T": lambda m: word(m, 1, 0, T + 1, -3),
              "word 1": lambda m: word(m, 1, 2, 1, 1), "a padding nibble": lambda m: nibble(m, 1, 0, 4, 1),
              "the last padding nibble": lambda m: nibble(m, 1, 2, 7, 1), "a key frame's nibble": lambda m: nibble(m, 0, 1, 0, 1),
              "a key frame's table": lambda m: word(m, 2, 0, 0, 1), "a key frame's word": lambda m: word(m, 2, 2, 9, 7)}
    for name, hurt in damage.items():
        m = maps.copy()
        hurt(m)
        if name == "a nibble above T = 0":                   # (T = 0 alone leaves nibbles above it: clear the plane's, set one)
            m[1, ml.map_offset[1]:ml.map_offset[1] + 4] = 0
            m[1, 64:128] = 0
            nibble(m, 1, 1, 0, 1)
        assert _status(L.csic_mc_undelta_host, C.byref(cp), p(diff), p(m), 3, 2, p(out)) == N.EFORMAT, name
        assert np.all(out == 0x5A), name
        with pytest.raises(csic.CsicIOError):
            csic.mc_undelta_host(cp, diff, m, 2)
    # what decodes: T = 0 with nibbles of zero; any displacement, INT32_MIN and INT32_MAX included; the result deltas again
    for plane, t, v in ((0, 1, None), (0, T, -2 ** 31), (1, int(maps[1, 64]), 2 ** 31 - 1), (2, int(maps[1, 128]), 12345)):
        m = maps.copy()
        if v is None:
            m[1, 0:64] = 0
            m[1, ml.map_offset[0]:ml.map_offset[0] + 4] = 0
        elif t >= 2:
            word(m, 1, plane, t, v)
        other = lib_mc_undelta(cp, diff, m, 2)
        frames = [[np.array([(int.from_bytes(other[k, o:o + nb].tobytes(), "little") >> (i * q)) & ((1 << q) - 1) for i in range(W * H)], dtype=np.int64)
                   for o, nb, q in zip((lay.y_offset, lay.cb_offset, lay.cr_offset), (lay.y_bytes, lay.cb_bytes, lay.cr_bytes), bits)] for k in range(3)]
        assert np.array_equal(frame_buffers(lay, frames, bits, CANARY), other)
        want = ref_mc_undelta([[np.array([(int.from_bytes(diff[k, o:o + nb].tobytes(), "little") >> (i * q)) & ((1 << q) - 1) for i in range(W * H)], dtype=np.int64)
                                for o, nb, q in zip((lay.y_offset, lay.cb_offset, lay.cr_offset), (lay.y_bytes, lay.cb_bytes, lay.cr_bytes), bits)] for k in range(3)],
                              [bytes(m[k, :ml.map_bytes]) for k in range(3)], bits, 2)
        assert all(np.array_equal(a, b) for fa, fb in zip(want, frames) for a, b in zip(fa, fb))
        d2, m2 = lib_mc_delta(cp, other, 2, 2)
        assert np.array_equal(lib_mc_undelta(cp, d2, m2, 2), other)
    # the Python layer
    d3, m3 = csic.mc_delta_host(cp, src, 2, 2)
    assert np.array_equal(m3[:, :ml.map_bytes], maps[:, :ml.map_bytes]) and np.array_equal(csic.mc_undelta_host(cp, d3, m3, 2), lib_mc_undelta(cp, diff, maps, 2, fill=0))
    with pytest.raises(csic.IllegalArgumentException):
        csic.mc_delta_host(cp, src[:, :-1], 2, 2)
    with pytest.raises(csic.IllegalArgumentException):
        csic.mc_delta_host(cp, src, 2, 8)
