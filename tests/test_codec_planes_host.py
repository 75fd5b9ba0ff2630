"""The built-to-order code planes of tests/codec_planes.py, checked without a GPU and with the numpy reference alone: each builder's
condition is an assertion here, so that tests/test_gpu_codec_planes.py shows the device codecs what its docstring says and nothing
moves silently.  Every built frame also goes through both host codecs (check_frame of test_rice_host.py and test_pack_host.py), and
every foreign stream is accepted by its host decoder before a device ever sees it.  Every comparison is exact."""
import numpy as np
import pytest

from codec_planes import (BLOCK, FOREIGN_N, LONG_RUN_SLOTS, SHUFFLED_GROUPS, SHUFFLED_N, TRIPLES, foreign_frames, full_chunk_dwords, full_chunk_frame,
                          full_cost_group, groups_of_mode, long_run_groups, long_runs, modes_of, planes_for, pools, reachable_modes, runs_frame,
                          shuffled_frame, widths_of)
from test_container import CANARY, CSQ, _c_params, _frame_buffer, _layout
import test_pack_host as grp
import test_rice_host as rice
from test_pack_host import plane_bytes, ref_groups
from test_rice_host import ref_chunk, ref_encode_rice, ref_modes

import csic_amd as csic

N = csic._native
QS = range(1, 9)


def _both(planes, bits, decode):
    """check_frame of both host codecs on an n x 1, 4:4:4, factor-1 frame."""
    assert len({c.size for c in planes}) == 1 and all(0 <= c.min() and c.max() < (1 << q) and c.dtype == np.int64 for c, q in zip(planes, bits))
    cp = _c_params(planes[0].size, 1, 4, 4, bits, 1, CSQ)
    lay = _layout(cp)
    assert [lay.geometry.y_width * lay.geometry.y_height] + [lay.geometry.chroma_samples] * 2 == [c.size for c in planes]
    rice.check_frame(cp, planes, bits, decode=decode)
    grp.check_frame(cp, planes, bits, decode=decode)
    return cp


@pytest.mark.parametrize("q", QS)
def test_groups_of_mode_gives_distinct_groups_of_that_mode(q):
    rng = np.random.default_rng(13500 + q)
    assert reachable_modes(q) == [15] + [k for k in range(q + 1) if k != q - 1]
    for k in reachable_modes(q):
        got = groups_of_mode(q, k, rng, 8)
        assert len(got) == (min(8, 1 << q) if k == 15 else 8), (q, k)
        assert len({c.tobytes() for c in got}) == len(got)
        assert all(c.shape == (32,) and ref_modes(ref_groups(c, q)[2], q).tolist() == [k] for c in got), (q, k)
    assert groups_of_mode(q, q - 1, rng, 2) == []              # never the cheapest
    assert sorted(pools(q)) == sorted(reachable_modes(q))


@pytest.mark.parametrize("q", QS)
def test_runs_and_shuffled_frames_hold_every_mode_and_every_width(q):
    runs, shuf = runs_frame(q), shuffled_frame(q)
    ks = reachable_modes(q)[1:]
    assert runs[0].size == 32 * BLOCK * len(ks) <= 65536
    m = ref_modes(ref_groups(runs[0], q)[2], q).reshape(len(ks), BLOCK)
    for b, k in enumerate(ks):                                 # one block per mode: lane t's R offset is 31 k t
        assert np.all(m[b] == k), (q, k)
        assert len({runs[0][32 * (BLOCK * b + i):][:32].tobytes() for i in range(BLOCK)}) >= 8
        off = 31 * k * np.arange(BLOCK)                        # the lanes' bit offsets in R: every residue that 31 k t can take
        assert set((off % 32).tolist()) == set(range(0, 32, int(np.gcd(k, 32)))), (q, k)
        if k == 1:                                             # a 31-bit run that never fills its dword: only RcWriter::finish() writes it
            assert np.any((off % 32 == 0) & (off > 0))
    assert (1 in ks) == (q != 2)
    assert shuf[0].size == SHUFFLED_N and SHUFFLED_N % 32 and SHUFFLED_GROUPS % BLOCK and (SHUFFLED_GROUPS + BLOCK - 1) // BLOCK == 3
    assert SHUFFLED_N < 25000
    assert modes_of(runs[0], q) | modes_of(shuf[0], q) == set(reachable_modes(q))
    assert modes_of(shuf[0], q) == set(reachable_modes(q))
    assert widths_of(runs[0], q) | widths_of(shuf[0], q) == set(range(q + 1))
    bits = (q, q, q)
    _both(runs, bits, decode=False)
    _both(shuf, bits, decode=False)


@pytest.mark.parametrize("bits", TRIPLES)
def test_planes_of_three_widths(bits):
    """planes_for: plane p is the builder's at bits[p], cycled by whole groups to the longest plane's n; what test 1 of the GPU module
    asserts about the batch holds on the CPU."""
    runs = planes_for(runs_frame, bits)
    n = runs[0].size
    assert n == max(32 * BLOCK * q for q in bits) and all(c.size == n for c in runs)
    shuf = planes_for(shuffled_frame, bits, n)
    for p, q in enumerate(bits):
        assert np.array_equal(runs[p][:runs_frame(q)[p].size], runs_frame(q)[p])
        assert np.array_equal(shuf[p][:SHUFFLED_N // 32 * 32], shuffled_frame(q)[p][:SHUFFLED_N // 32 * 32])
        assert modes_of(runs[p], q) | modes_of(shuf[p], q) == set(reachable_modes(q))
        assert widths_of(runs[p], q) | widths_of(shuf[p], q) == set(range(q + 1))
    _both(planes_for(shuffled_frame, bits), bits, decode=False)
    _both(planes_for(full_chunk_frame, bits), bits, decode=False)


LONGEST = {8: [(0, 31), (1, 62), (2, 124)], 7: [(0, 31), (1, 62)], 6: [(0, 31)], 5: [(0, 15)], 4: [(0, 7)], 3: [(0, 3)], 2: [(0, 1)], 1: []}
ZEROS = {8: 62, 7: 62, 6: 62, 5: 30, 4: 14, 3: 6, 2: 2}


@pytest.mark.parametrize("q", QS)
def test_long_run_groups(q):
    assert [(k, r) for k, r, _ in long_runs(q)] == LONGEST[q] and all(z == ZEROS[q] for _, _, z in long_runs(q))
    planes = long_run_groups(q)
    c = planes[0]
    G = 64 * max(len(LONGEST[q]), 1)
    assert c.size == 32 * G < 25000
    _, anchors, u = ref_groups(c, q)
    m = ref_modes(u, q)
    for i, (k, r) in enumerate(LONGEST[q]):
        rows = u[64 * i:64 * i + 64]
        assert np.all(m[64 * i:64 * i + 64] == k)
        assert np.all((rows > 0).sum(axis=1) == 1) and np.all(rows.max(axis=1) == 2 * r)       # one outlier, the rest of the group constant
        assert {int(j) for j in rows.argmax(axis=1)} == set(LONG_RUN_SLOTS)
        assert np.all((rows.max(axis=1) >> k) == ZEROS[q])
    assert len(set(anchors.tolist())) == min(64, 1 << q)
    if q >= 6:                                                 # a dword of U without a terminator: a plateau of the running count
        R, U, z = ref_chunk(u, m, q)
        assert z == G
        words = U[:U.size // 32 * 32].reshape(-1, 32)
        assert np.any(words.sum(axis=1) == 0)
        # and a run of 62 zeros that starts at bit 2 or later of its dword makes RcWriter::unary flush twice
        ones = np.flatnonzero(U)
        starts = np.concatenate([[0], ones[:-1] + 1])
        assert np.any(((ones - starts) == 62) & (starts % 32 >= 2))
    _both(planes, (q, q, q), decode=True)


@pytest.mark.parametrize("q", QS)
def test_full_chunk_frame(q):
    planes = full_chunk_frame(q)
    c = planes[0]
    assert c.size == 3 * BLOCK * 32 < 25000
    _, _, u = ref_groups(c, q)
    m = ref_modes(u, q)
    if q >= 2:
        g = full_cost_group(q)
        ug = ref_groups(g, q)[2]
        assert ref_modes(ug, q).tolist() == [q - 2] and 31 * (q - 2) + int(((ug[0, 1:] >> (q - 2)) + 1).sum()) == 31 * q
        for b, at in ((0, 100), (2, 255)):
            mb = m[BLOCK * b:BLOCK * b + BLOCK]
            assert mb[at] == q - 2 and np.all(np.delete(mb, at) == q)
    else:
        assert np.all(m[:BLOCK] == 1) and np.all(m[2 * BLOCK:] == 1)
    assert np.all(m[BLOCK:2 * BLOCK] == 15)
    info = []
    coded = ref_encode_rice(planes, (q, q, q), info)
    assert len(info) == 9
    want = full_chunk_dwords(q)
    assert want == (248 * q + 1 if q >= 2 else 248)
    for p in range(3):
        blocks = info[3 * p:3 * p + 3]
        assert [i[0] for i in blocks] == [p] * 3
        dwords = [(rb + 31) // 32 + (ub + 31) // 32 for _, _, rb, ub, _ in blocks]
        assert dwords == [want, 0, want], (q, dwords)
        d = [i[1] for i in blocks]
        assert d[1] - d[0] == want and d[2] == d[1]
    rl = rice.rice_layout(_c_params(c.size, 1, 4, 4, (q, q, q), 1, CSQ))
    assert len(coded) == rl.fixed_bytes + 4 * 6 * want
    _both(planes, (q, q, q), decode=False)


@pytest.mark.parametrize("q", QS)
def test_foreign_streams_are_valid(q):
    """Streams that another encoder may write -- every group at mode k = 0 .. q (k = q - 1 among them, and at k = 0 a run of 2^q - 1
    zeros), every group stored at least w = 0 .. q bits wide: within bound_bytes, and the host decoders accept them and return the frame."""
    planes, rice_streams, grp_streams = foreign_frames(q)
    bits = (q, q, q)
    assert planes[0].size == FOREIGN_N and ref_groups(planes[0], q)[2].max() == (1 << q) - 1
    cp = _both(planes, bits, decode=True)
    frame = _frame_buffer(_layout(cp), [plane_bytes(c, q) for c in planes], CANARY)
    rl, pk = rice.rice_layout(cp), grp.lib_layout(cp)
    assert [k for k, _ in rice_streams] == list(range(q + 1)) == [w for w, _ in grp_streams]
    for k, coded in rice_streams:
        assert rl.fixed_bytes <= len(coded) <= rl.bound_bytes, (q, k)
        nib = rice._nibbles(np.frombuffer(coded, dtype=np.uint8), rl.modes_offset[0], rl.groups[0])
        assert set(nib.tolist()) == {15, k}
        st, back = rice.rice_unpack(cp, coded)
        assert st == N.OK and np.array_equal(back, frame), (q, k)
    assert len({s for _, s in rice_streams}) == q + 1
    for w, coded in grp_streams:
        assert pk.fixed_bytes <= len(coded) <= pk.bound_bytes, (q, w)
        nib = rice._nibbles(np.frombuffer(coded, dtype=np.uint8), pk.widths_offset[0], pk.groups[0])
        assert nib.min() == w and np.array_equal(nib, np.maximum(ref_groups(planes[0], q)[0], w))
        st, back = grp.lib_unpack(cp, coded)
        assert st == N.OK and np.array_equal(back, frame), (q, w)
    assert grp_streams[0][1] == grp.ref_encode(planes, bits)   # force = 0 is the encoder's own stream
