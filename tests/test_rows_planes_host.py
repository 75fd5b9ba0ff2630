"""The planes of tests/rows_planes.py meet their conditions: proved here with numpy alone (the statement of tests/rows_ref.py, and
rows_variant's copies of it with one rule changed), then every plane goes through the host codec (check_frames of
tests/test_rows_host.py: byte for byte, both directions, apart and in place).  The set is one plan per pair of q = 1 .. 8 and
delta = 0 .. 31, (32 + delta) x 19 at 4:4:4 and factor 1 -- K = 1, two or three bands, a ragged tail wherever delta != 0 -- with q in
the Y plane and two other bit widths beside it.  No GPU."""
import numpy as np
import pytest

from rows_planes import HEIGHT, NAMES, TARGETS, VARIANTS, built_frames, contest_seconds, built_planes, plan_bits, relations, rows_variant
from rows_ref import ref_rows_plane
from test_rows_host import _params, check_frames

QS = range(1, 9)
DELTAS = range(32)


def _contest(q, delta):
    return built_planes(q)[delta]["contest"], 32 + delta


# the variants that are the definition itself on some planes: nothing else may go unnoticed
def _equivalent(name, q, delta):
    if name in ("far_as_near", "no_far", "tail"):
        return delta == 0                      # no far slots, and n = 32 x 19 is a multiple of 32
    return name == "no_fold" and q == 1        # folding one bit is the identity


@pytest.mark.parametrize("q", QS)
def test_the_statement_without_a_switch_is_the_reference(q):
    for delta in DELTAS:
        for name in NAMES:
            x, w = built_planes(q)[delta][name], 32 + delta
            assert x.size == w * HEIGHT and x.min() >= 0 and x.max() < 1 << q
            got, want = rows_variant(x, w, q), ref_rows_plane(x, w, q)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (q, delta, name)


@pytest.mark.parametrize("q", QS)
def test_relations_and_choices_of_the_contest_planes(q):
    """Each of cost_up - cost_left = -1, 0, +1 in at least 2 groups, at least half of the groups on their target, both choices in the
    map; the ragged group's choice flips if its phantom slots are counted; the band-second groups are "up" with u = 0."""
    for delta in DELTAS:
        x, w = _contest(q, delta)
        d = relations(x, w, q)
        assert all((d == want).sum() >= 2 for want in TARGETS), (q, delta, [(d == want).sum() for want in TARGETS])
        assert 2 * (d == np.array(TARGETS)[np.arange(d.size) % 3]).sum() >= d.size, (q, delta)
        t = ref_rows_plane(x, w, q)[1]
        assert t.any() and not t.all(), (q, delta)
        if delta:
            assert x.size % 32 and rows_variant(x, w, q, tail=True)[1][-1] != t[-1], (q, delta)
            seconds = contest_seconds(x.size, w)
            assert 17 in seconds and all(g % 16 == 1 for g in seconds)
            for g in seconds:
                assert t[g] and not x[32 * g:32 * g + delta].any() and x[32 * g - w:32 * g + delta - w].any(), (q, delta, g)
                assert np.array_equal(x[32 * g + delta:32 * g + 32], x[32 * g + delta - w:32 * g + 32 - w]), (q, delta, g)


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_every_wrong_variant_shows_on_every_contest_plane(name):
    for q in QS:
        for delta in DELTAS:
            x, w = _contest(q, delta)
            want = ref_rows_plane(x, w, q)
            got = rows_variant(x, w, q, **VARIANTS[name])
            same = np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            assert same == _equivalent(name, q, delta), (name, q, delta)


def test_every_path_of_the_shift_is_taken():
    """rw_reference (csrc/csic_rows.hip) shifts by delta Q bits through rw_shift<Q, WS>, WS = ceil(delta Q / 32), and hands
    bits = 32 WS - delta Q to the alignbit: the Y planes of the set reach all 44 pairs, and every pair with WS >= 1 and bits = 0."""
    taken = {(q, -(-delta * q // 32), 32 * -(-delta * q // 32) - delta * q) for q in QS for delta in built_planes(q)}
    assert {(q, ws) for q, ws, _ in taken} == {(q, ws) for q in QS for ws in range(q + 1)} and len({(q, ws) for q, ws, _ in taken}) == 44
    whole = {(q, ws) for q in QS for ws in range(1, q + 1) if 32 * ws % q == 0 and 32 * ws // q <= 31}
    assert {(q, ws) for q, ws, bits in taken if bits == 0 and ws >= 1} == whole and len(whole) == 12
    # and each q is the Y plane of a plan, each of the others a chroma plane of one
    assert {plan_bits(q)[0] for q in QS} == {plan_bits(q)[1] for q in QS} == {plan_bits(q)[2] for q in QS} == set(QS)


@pytest.mark.parametrize("q", QS)
def test_host_codec_on_every_plane(q):
    for delta in DELTAS:
        bits, frames = built_frames(q, delta)
        cp = _params(32 + delta, HEIGHT, bits)
        _, _, ts = check_frames(cp, frames, bits, (q, delta))
        assert all(not t.any() for t in ts[1] + ts[2])                     # constant planes: every group a tie
