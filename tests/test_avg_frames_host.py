"""The builders of tests/avg_frames.py, proved on the CPU before tests/test_gpu_avg_frames.py relies on them: ref_avg states what
orc_process_avg computes (random parameters and every built frame), the levers hold, the counted facts about the forward
transform's chroma arithmetic are what the cube gives, the palette and the windows reach the corners they are built for, the two
second opinions on the oracle agree with it (cube: AVG at 4:4:4 factor 1 is the closed form; palette: a magnified frame's AVG output
is the closed form of the unmagnified one), and every fault of avg_frames.FAULTS is noticed by the set of frames named for it
wherever the table below says it can matter -- and by none of them where it says it cannot."""
import numpy as np
import pytest

import avg_frames as af

CSQ = (3, 1, 2)
ROUNDINGS = (af.FLOOR, af.TRUNC)
MF_IDS = [f"{a}{b}-f{f}" for a, b, f in af.MODE_FACTORS]


def _op(orc, W, H, a=4, b=4, bits=(8, 8, 8), f=1, rounding=0, fmt=af.YCC):
    return orc.OracleParams(width=W, height=H, chroma_a=a, chroma_b=b, y_bits=bits[0], cb_bits=bits[1], cr_bits=bits[2], factor=f, op=CSQ,
                            rounding=rounding, out_format=fmt)


def _avg(orc, frame, a, b, f, rounding, fmt=af.YCC, bits=(8, 8, 8)):
    H, W = frame.shape
    return orc.process(_op(orc, W, H, a, b, bits, f, rounding, fmt), frame, form="avg")


def _ref(frame, a, b, f, rounding, fmt=af.YCC, bits=(8, 8, 8), fault=None, detail=False):
    H, W = frame.shape
    return af.ref_avg(frame, W, H, a, b, bits, f, rounding, fmt, fault, detail)


def _palette_frames(a, b, f):
    h, v = af.HV[a, b]
    return [af.magnified(af.palette(), f, h, v), af.magnified_cut(af.palette(), f, h, v)]


def _residue_frames(a, b, f):
    return [af.residue_frame(W, H, content) for W, H in af.residue_shapes(a, b, f) for content in af.RESIDUE_CONTENTS]


# ---- the statement ---------------------------------------------------------------------------------
def test_ref_avg_is_the_oracle_on_random_parameters(oracle):
    rng = np.random.default_rng(0xA761)
    for _ in range(400):
        W, H = int(rng.integers(1, 45)), int(rng.integers(1, 30))
        a, b = af.MODES[int(rng.integers(0, 6))]
        f, rounding, fmt = int(rng.choice(af.FACTORS)), int(rng.integers(0, 2)), int(rng.integers(0, 2))
        bits = tuple(int(x) for x in rng.integers(1, 9, 3))
        frame = rng.integers(0, 1 << 32, (H, W), dtype=np.uint32)
        want = oracle.process(_op(oracle, W, H, a, b, bits, f, rounding, fmt), frame, form="avg")
        assert np.array_equal(af.ref_avg(frame, W, H, a, b, bits, f, rounding, fmt), want), (W, H, a, b, bits, f, rounding, fmt)


@pytest.mark.parametrize("a,b,f", af.MODE_FACTORS, ids=MF_IDS)
def test_ref_avg_is_the_oracle_on_every_built_frame(oracle, a, b, f):
    """Palette (both magnified forms), windows and residues (every shape, every content), both roundings, both packed formats; a
    mixed bit triple on the YCbCr side."""
    for rounding in ROUNDINGS:
        frames = _palette_frames(a, b, f) + [af.windows_frame(a, b, f, rounding)[0]] + _residue_frames(a, b, f)
        for k, frame in enumerate(frames):
            for fmt, bits in ((af.YCC, (8, 8, 8)), (af.ARGB, (8, 8, 8)), (af.YCC, (5, 6, 3))):
                assert np.array_equal(_ref(frame, a, b, f, rounding, fmt, bits), _avg(oracle, frame, a, b, f, rounding, fmt, bits)), \
                    (rounding, k, frame.shape, fmt, bits)


# ---- the levers and the counted facts ----------------------------------------------------------------
def _oracle_ycc(orc, colours, rounding):
    """(Y, Cb, Cr) of ARGB colours by the oracle's own forward transform."""
    colours = np.asarray(colours, dtype=np.uint32).reshape(1, -1)
    out = orc.process(_op(orc, colours.size, 1, rounding=rounding), colours, form="closed").reshape(-1)
    return out & 255, (out >> 8) & 255, (out >> 16) & 255


def test_the_levers_hold(oracle):
    v = np.arange(256)
    c = np.arange(1, 256)
    for rounding in ROUNDINGS:
        y, cb, cr = _oracle_ycc(oracle, af.gray(v), rounding)
        assert np.array_equal(y, v) and (cb == 128).all() and (cr == 128).all()
        for mine, table, other in ((1, af.colour_for_cb, af.other_of_cb), (2, af.colour_for_cr, af.other_of_cr)):
            got = _oracle_ycc(oracle, table[rounding][1:], rounding)
            assert np.array_equal(got[mine], c), (rounding, mine)
            assert np.array_equal(got[3 - mine], other[rounding][1:]), (rounding, mine)
            assert (table[rounding][1:] >> 24 == 0xFF).all() and table[rounding][0] == 0
        assert np.array_equal(af.through_lever("cb", c, rounding), af.colour_for_cb[rounding][1:])
        assert np.array_equal(af.through_lever("y", v, rounding), af.gray(v))


def test_forward_is_the_oracle_on_the_palette(oracle):
    pal = af.palette().reshape(-1)
    for rounding in ROUNDINGS:
        y, cb, cr, _, _ = af.forward(pal, rounding)
        oy, ob, orr = _oracle_ycc(oracle, pal, rounding)
        assert np.array_equal(y, oy) and np.array_equal(cb, ob) and np.array_equal(cr, orr)


def test_counted_facts_of_the_chroma_arithmetic():
    """Over the whole cube: the clamp 256 -> 255 fires for one colour per channel (pure blue, pure red), a quotient of 255 without it
    has 19 colours in Cb and 33 in Cr, each threshold value of u has more than 500 colours; every chroma value 1 .. 255 is reached and 0
    is not; with the other channel at 128 only 7 .. 249 (8 .. 249 when rounding toward zero) are."""
    ub, ur = af.cube_numerators()
    assert np.flatnonzero(ub == 65536).tolist() == [0x0000FF] and np.flatnonzero(ur == 65536).tolist() == [0xFF0000]
    assert ub.max() == 65536 and ur.max() == 65536 and ub.min() >= 0 and ur.min() >= 0
    assert int(((ub >= 65280) & (ub < 65536)).sum()) == 19 and int(((ur >= 65280) & (ur < 65536)).sum()) == 33
    for t in af.THRESHOLD_U:
        assert (ub == t).sum() > 500 and (ur == t).sum() > 500, t
    for rounding, lowest in ((af.FLOOR, 7), (af.TRUNC, 8)):
        cb, cr = af.cube_chroma(rounding)
        for mine, other in ((cb, cr), (cr, cb)):
            assert np.array_equal(np.unique(mine), np.arange(1, 256))
            assert np.array_equal(np.unique(mine[other == 128]), np.arange(lowest, 250))
    # the rule the device code states for rounding toward zero, on every u the cube reaches: u < 32768 rounds up
    for u, c in ((ub, af.cube_chroma(af.TRUNC)[0]), (ur, af.cube_chroma(af.TRUNC)[1])):
        assert np.array_equal(np.minimum((u + np.where(u < 32768, 255, 0)) >> 8, 255), c)


# ---- the cube ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cube_outputs(oracle):
    """The oracle on the cube at 4:4:4, factor 1, YCbCr output: {(rounding, form)}, computed once."""
    cube = af.cube()
    out = {(rounding, form): oracle.process(_op(oracle, 4096, 4096, rounding=rounding), cube, form=form) for rounding in ROUNDINGS for form in ("avg", "closed")}
    for x in out.values():
        x.setflags(write=False)
    return out


@pytest.mark.parametrize("rounding", ROUNDINGS)
def test_on_the_cube_avg_is_the_closed_form(cube_outputs, rounding):
    assert np.array_equal(cube_outputs[rounding, "avg"], cube_outputs[rounding, "closed"])
    # and the chroma the lever tables are built from is the oracle's
    closed = cube_outputs[rounding, "closed"].reshape(-1)
    cb, cr = af.cube_chroma(rounding)
    assert np.array_equal(cb, (closed >> 8) & 255) and np.array_equal(cr, (closed >> 16) & 255)


@pytest.mark.parametrize("rounding", ROUNDINGS)
def test_ref_avg_is_the_oracle_on_the_cube(cube_outputs, rounding):
    assert np.array_equal(af.ref_avg(af.cube(), 4096, 4096, 4, 4, (8, 8, 8), 1, rounding, af.YCC), cube_outputs[rounding, "avg"])


# ---- the palette -------------------------------------------------------------------------------------
def test_palette_membership():
    pal = af.palette()
    assert pal.shape[1] == af.PALETTE_WIDTH and pal.size <= 4096 and (pal >> 24 == 0xFF).all()
    colours = set((pal.reshape(-1) & 0xFFFFFF).tolist())
    assert set(af.NAMED) <= colours
    ub_all, ur_all = af.cube_numerators()
    _, _, _, ub, ur = af.forward(np.array(sorted(colours), dtype=np.uint32), af.FLOOR)
    for u, u_all in ((ub, ub_all), (ur, ur_all)):
        assert int((u >= 65280).sum()) == int((u_all >= 65280).sum())         # every colour at or above a quotient of 255 ...
        assert int((u == 65536).sum()) == 1                                    # ... and the one the clamp fires for
        for t in af.THRESHOLD_U:
            assert int((u == t).sum()) >= 8, t
        for lb in af.LOW_BYTES:
            assert int(((u < 32768) & ((u & 255) == lb)).sum()) >= 8, lb
        assert ((u > 32512) & (u < 32768)).any() and (u <= 32512).any() and (u >= 32768).any()     # both sides of the TRUNC threshold
    assert int((ub >= 65280).sum()) == 20 and int((ur >= 65280).sum()) == 34
    for rounding in ROUNDINGS:
        for table in (af.colour_for_cb, af.colour_for_cr):
            assert set((table[rounding][1:] & 0xFFFFFF).tolist()) <= colours


@pytest.mark.parametrize("a,b,f", af.MODE_FACTORS, ids=MF_IDS)
def test_a_magnified_palette_averages_to_its_closed_form(oracle, a, b, f):
    """The second opinion on orc_process_avg: every aligned max(f, h) x max(f, v) region of the frame is one colour, so every block
    and every pooling window averages equal values, cut regions included (the clamped coordinates repeat the same colour)."""
    h, v = af.HV[a, b]
    pal = af.palette()
    for rounding in ROUNDINGS:
        for fmt in (af.YCC, af.ARGB):
            closed = oracle.process(_op(oracle, pal.shape[1], pal.shape[0], rounding=rounding, fmt=fmt), pal, form="closed")
            for cut, frame in enumerate(_palette_frames(a, b, f)):
                assert frame.shape == (pal.shape[0] * max(f, v) - cut, pal.shape[1] * max(f, h) - cut)
                want = af.magnified_expectation(closed, f, h, v, bool(cut))
                assert np.array_equal(_avg(oracle, frame, a, b, f, rounding, fmt), want), (rounding, fmt, cut)


# ---- the windows -------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b,f", af.MODE_FACTORS, ids=MF_IDS)
def test_the_windows_reach_the_ends_and_both_sides_of_every_tie(a, b, f):
    """Per instantiation and rounding: the maximal block sum h v 255 in Cb and Cr and the maximal pool sum f f 255 in Y, Cb and Cr; in the
    chroma stage (n = h v > 1) a block sum on the tie (remainder n / 2, rounds up) and one below it (n / 2 - 1) in Cb and in Cr; in the
    spatial stage (f > 1) the same for Y (remainders f f / 2 and f f / 2 - 1) and for Cb, Cr wherever block averages can produce a tie:
    a pooling block sums one block average per unit (a chroma block cut to the pooling block, m = min(h, f) min(v, f) pixels), so
    its sum is a multiple of m and a tie exists only for m < f f; the nearest sum below it then has remainder f f / 2 - m."""
    h, v = af.HV[a, b]
    n, ff, m = h * v, f * f, min(h, f) * min(v, f)
    for rounding in ROUNDINGS:
        frame, where = af.windows_frame(a, b, f, rounding)
        assert frame.shape[1] % 8 == 0 and frame.shape[1] // 4 > 32 and len({(wy, wx) for _, _, wy, wx in where}) == len(where)
        _, d = _ref(frame, a, b, f, rounding, detail=True)
        for s in d["block_sums"]:
            assert s.max() == n * 255
            if n > 1:
                assert (s % n == n // 2).any() and (s % n == n // 2 - 1).any()
        for k, s in enumerate(d["pool_sums"]):
            assert s.max() == ff * 255, k
        if f > 1:
            sy = d["pool_sums"][0]
            assert (sy % ff == ff // 2).any() and (sy % ff == ff // 2 - 1).any()
            for s in d["pool_sums"][1:]:
                if m < ff:
                    assert (s % ff == ff // 2).any() and (s % ff == ff // 2 - m).any()
                else:
                    assert (s % m == 0).all()


def test_the_window_recipes_dictate_their_channel(oracle):
    """At 4:4:4, factor 1 the plan's output is the forward transform: the dictated channel of every window holds the recipe."""
    for rounding in ROUNDINGS:
        for a, b, f in ((2, 0, 4), (1, 1, 2), (4, 4, 8)):
            frame, where = af.windows_frame(a, b, f, rounding)
            ycc = oracle.process(_op(oracle, frame.shape[1], frame.shape[0], rounding=rounding), frame, form="closed")
            recipes = {ch: dict(af.window_recipes(*af.HV[a, b], f, ch)) for ch in af.CHANNELS}
            for ch, name, wy, wx in where:
                got = (ycc[8 * wy:8 * wy + 8, 8 * wx:8 * wx + 8] >> (8 * af.CHANNELS.index(ch))) & 255
                assert np.array_equal(got, recipes[ch][name]), (rounding, a, b, f, ch, name)


# ---- the kill table ----------------------------------------------------------------------------------
ALL_F = (1, 2, 4, 8)
EVERYWHERE = {m: ALL_F for m in af.MODES}
# fault -> (chroma mode -> the factors at which it can matter, the roundings, the sets that must notice it).  Written out by hand:
#   block_half_missing   needs a block of more than one pixel;  pool_half_missing a pooling block of more than one
#   one_stage            needs both, and a pooling block that holds more than one block average: f > h or f > v
#   edge_virtual_block   needs a pooling window that reaches past the last real chroma block into a further one, and a last real block
#                        of more than one pixel in that direction: h >= 2 with f > h, or v = 2 with f >= 4
#   edge_no_row_hold     the vertical half of that: v = 2 with f >= 4
WHERE = {
    "no_clamp": (EVERYWHERE, (0, 1), ("palette",)),
    "trunc_threshold_32512": (EVERYWHERE, (1,), ("palette",)),
    "block_half_missing": ({(4, 4): (), (2, 2): ALL_F, (2, 0): ALL_F, (1, 1): ALL_F, (4, 0): ALL_F, (1, 0): ALL_F}, (0, 1), ("windows",)),
    "pool_half_missing": ({m: (2, 4, 8) for m in af.MODES}, (0, 1), ("windows",)),
    "one_stage": ({(4, 4): (), (2, 2): (2, 4, 8), (2, 0): (4, 8), (1, 1): (2, 4, 8), (4, 0): (2, 4, 8), (1, 0): (4, 8)}, (0, 1), ("windows",)),
    "edge_virtual_block": ({(4, 4): (), (2, 2): (4, 8), (2, 0): (4, 8), (1, 1): (8,), (4, 0): (4, 8), (1, 0): (4, 8)}, (0, 1), ("residues",)),
    "edge_no_row_hold": ({(4, 4): (), (2, 2): (), (2, 0): (4, 8), (1, 1): (), (4, 0): (4, 8), (1, 0): (4, 8)}, (0, 1), ("residues",)),
    "f8_left_half_twice": ({m: (8,) for m in af.MODES}, (0, 1), ("windows", "residues")),
}


def _set(name, a, b, f, rounding):
    if name == "palette":
        return _palette_frames(a, b, f)
    if name == "windows":
        return [af.windows_frame(a, b, f, rounding)[0]]
    return _residue_frames(a, b, f)


def test_the_table_names_every_fault():
    assert sorted(WHERE) == sorted(af.FAULTS)
    for modes, roundings, sets in WHERE.values():
        assert sorted(modes) == sorted(af.MODES) and set(roundings) <= {0, 1} and set(sets) <= {"palette", "windows", "residues"}


@pytest.mark.parametrize("fault", af.FAULTS)
def test_kill_table(oracle, fault):
    """Wherever the table says the fault can matter, at least one frame of EACH set named for it differs from the oracle's output;
    wherever it says it cannot, no frame of those sets does (so the table understates nothing)."""
    modes, roundings, sets = WHERE[fault]
    survivors, overstated = [], []
    for a, b, f in af.MODE_FACTORS:
        for rounding in ROUNDINGS:
            applies = f in modes[a, b] and rounding in roundings
            for name in sets:
                killed = False
                for frame in _set(name, a, b, f, rounding):
                    if not np.array_equal(_ref(frame, a, b, f, rounding, fault=fault), _avg(oracle, frame, a, b, f, rounding)):
                        killed = True
                        break
                if applies and not killed:
                    survivors.append((a, b, f, rounding, name))
                if killed and not applies:
                    overstated.append((a, b, f, rounding, name))
    assert not survivors, f"{fault} is not noticed by: {survivors}"
    assert not overstated, f"{fault} matters where the table says it cannot: {overstated}"
