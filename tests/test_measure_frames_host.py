"""The frame builders of tests/measure_frames.py, proved on the CPU against the oracle and the numpy statements of the definitions
(sse_numpy, ssim_numpy) before tests/test_gpu_measure_frames.py relies on them: the three levers hold, the q table is what the
oracle's outputs give at every window position, the built set reaches the corners of the SSIM quotient and of the sum widths in
every kernel class, the maximal-error frame and the palette give the stated squared errors, the replay pair differs as described,
and no (class, lever, layout) is skipped."""
import numpy as np
import pytest

import measure_frames as mf
from test_distortion_host import forward
from test_ssim_host import ONE, _channels, _windows, float_ssim

SSIM_CLASSES = ("fast<f1>", "fast<f2>", "gen<hold>", "gen<hold,ycc-in>", "gen<avg>", "gen<avg,ycc-in>")
ORDERS = (mf.CSQ, mf.SCQ)                     # one order of each class (chroma before spatial, spatial before chroma)


def _pairs(orc, frame, W, H, c):
    """The six (reference, output) pairs of (H, W) arrays of a frame under a class's parameters and bits c["bits"]."""
    frame = np.asarray(frame, dtype=np.uint32).reshape(H, W)
    o_rgb, o_ycc = mf.oracle_outputs(orc, frame, W, H, c)
    return _channels(frame, o_rgb, o_ycc, c["f"], c["rounding"], c["in_format"])


# ---- the levers hold -------------------------------------------------------------------------------
def test_gray_pixels_have_y_v_and_neutral_chroma():
    v = np.arange(256)
    for rounding in (0, 1):
        y, cb, cr = forward(mf.gray(v), rounding)
        assert np.array_equal(y, v) and (cb == 128).all() and (cr == 128).all()


@pytest.mark.parametrize("f", [1, 2, 4, 8])
def test_gray_y_pairs_equal_the_closed_form_under_hold(oracle, f):
    """Both order classes, the six chroma modes, both roundings, two quantisers, a ragged shape: the chroma settings and the order
    do not leak into Y, and the chroma channels of a gray frame are (128, 128 & mask) throughout."""
    rng = np.random.default_rng(600 + f)
    W, H = 27, 19
    p = rng.integers(0, 256, (H, W))
    for op in ORDERS:
        for a, b in mf.CHROMA:
            for rounding in (0, 1):
                for q in (8, 3):
                    c = dict(mf._cls("x", a, b, f, op, rounding), bits=(q, 8, 8))
                    pairs = _pairs(oracle, mf.gray(p), W, H, c)
                    x, y = mf.y_pairs_closed_form(p, f, q)
                    assert np.array_equal(pairs[3][0], x) and np.array_equal(pairs[3][1], y), (op, a, b, rounding, q)
                    for k in (4, 5):
                        assert (pairs[k][0] == 128).all() and (pairs[k][1] == 128).all()


@pytest.mark.parametrize("f", [1, 2, 4, 8])
def test_gray_y_pairs_under_avg_are_the_rounded_block_mean(oracle, f):
    """What the oracle's AVG does to Y: output (ro, co) = (sum of the f x f block at (ro f, co f), coordinates clamped to the frame,
    + f f / 2) >> 2 log2 f, then cut to y_bits -- the mean rounded half up; the chroma averaging never touches Y."""
    rng = np.random.default_rng(700 + f)
    W, H = 27, 19
    p = rng.integers(0, 256, (H, W))
    for a, b in mf.CHROMA:
        for rounding in (0, 1):
            for q in (8, 3):
                c = dict(mf._cls("x", a, b, f, mf.CSQ, rounding, avg=True), bits=(q, 8, 8))
                pairs = _pairs(oracle, mf.gray(p), W, H, c)
                x, y = mf.y_pairs_closed_form(p, f, q, avg=True)
                assert np.array_equal(pairs[3][0], x) and np.array_equal(pairs[3][1], y), (a, b, rounding, q)
    # and on a two-valued block the mean is not the held pixel: held_white at f = 2 averages (255 + 0 + 0 + 0 + 2) >> 2 = 64
    x, y = mf.y_pairs_closed_form(mf.recipe("held_white", 2), 2, 8, avg=True)
    assert (y == 64).all()


@pytest.mark.parametrize("avg", [False, True])
def test_ycc_input_planes_are_independent(oracle, avg):
    """Changing one plane of a YCbCr-input frame changes only its own channel's pairs in Y, Cb, Cr."""
    rng = np.random.default_rng(800 + avg)
    W, H = 24, 16
    planes = [rng.integers(0, 256, (H, W)) for _ in range(3)]
    for f, op, (a, b) in ((1, mf.CSQ, (2, 0)), (2, mf.SCQ, (1, 0)), (4, mf.CSQ, (4, 0)), (8, mf.SCQ, (1, 1)), (2, mf.CSQ, (2, 2))):
        if avg and op != mf.CSQ:
            continue
        c = dict(mf._cls("x", a, b, f, op, avg=avg, in_format=mf.YCC), bits=(5, 4, 6))
        base = _pairs(oracle, mf.ycc(*planes), W, H, c)
        for k in range(3):
            assert np.array_equal(base[3 + k][0], planes[k])                     # the reference channel is the input plane itself
            changed = list(planes)
            changed[k] = 255 - planes[k]
            got = _pairs(oracle, mf.ycc(*changed), W, H, c)
            for m in range(3):
                same = all(np.array_equal(u, v) for u, v in zip(base[3 + m], got[3 + m]))
                assert same == (m != k), (f, op, a, b, k, m)


def test_the_palette_gives_the_stated_chroma():
    for colour, per_rounding in mf.PALETTE_CHROMA.items():
        for rounding in (0, 1):
            y, cb, cr = forward(np.array([colour], dtype=np.uint32), rounding)
            assert (int(cb[0]), int(cr[0])) == per_rounding[rounding]
    # blue / yellow: Cb 255 / 1; red / cyan: Cr 255 / 1; red's Cb 85 / 86 and blue's Cr 107 / 108 depend on the rounding
    P = mf.PALETTE_CHROMA
    assert [P[mf.BLUE][r][0] for r in (0, 1)] == [255, 255] and [P[mf.YELLOW][r][0] for r in (0, 1)] == [1, 1]
    assert [P[mf.RED][r][1] for r in (0, 1)] == [255, 255] and [P[mf.CYAN][r][1] for r in (0, 1)] == [1, 1]
    assert [P[mf.RED][r][0] for r in (0, 1)] == [85, 86] and [P[mf.BLUE][r][1] for r in (0, 1)] == [107, 108]
    pat = mf.recipe("cols")
    fr = mf.palette(pat, np.zeros((8, 8), dtype=int))
    assert (fr[:, 0::2] == mf.BLUE).all() and (fr[:, 1::2] == mf.YELLOW).all()
    fr = mf.palette(pat, np.ones((8, 8), dtype=int))
    assert (fr[:, 0::2] == mf.RED).all() and (fr[:, 1::2] == mf.CYAN).all()


# ---- the built set: counted, then held to the q table and the coverage conditions ----------------------
def test_nothing_is_skipped():
    classes = mf.classes()
    assert sorted({c["cls"] for c in classes}) == sorted(SSIM_CLASSES)
    fast = [(c["f"], mf.HOLD[c["a"], c["b"]], c["rounding"]) for c in classes if c["cls"].startswith("fast")]
    assert sorted(fast) == sorted((f, (h, v), r) for f in (1, 2) for h in (1, 2, 4) for v in (1, 2) for r in (0, 1))
    assert sorted((c["f"], c["op"]) for c in classes if c["cls"] == "gen<hold>") == sorted((f, op) for f in (2, 4, 8) for op in ORDERS)
    cases = mf.cases()
    per_class = {True: 4, False: 5}           # YCbCr input: the ycc lever at four quantisers; ARGB: gray at four and the palette
    assert len(cases) == sum(per_class[c["in_format"] == mf.YCC] for c in classes) * len(mf.LAYOUTS)
    assert len({mf.case_key(c) for c in cases}) == len(cases)
    for c in classes:
        mine = [k for k in cases if mf.class_id(k) == mf.class_id(c)]
        assert len(mine) == per_class[c["in_format"] == mf.YCC] * len(mf.LAYOUTS)
        assert {(k["W"], k["H"]) for k in mine} == set(mf.LAYOUTS)
    assert [mf.key_windows(n) for n in (1, 31, 32, 33, 65)] == [[0], [0, 30], [0, 31], [0, 31, 32], [0, 31, 32, 63, 64]]


def test_every_recipe_passes_through_every_key_window():
    for lever, names in (("gray", mf.RECIPE_SETS[8]), ("ycc", mf.RECIPE_SETS[4]), ("palette", mf.PALETTE_SET)):
        for W, H in mf.LAYOUTS:
            frames, where = mf.build_frames(lever, names, 2, W, H)
            nwin = (W // 8) * (H // 8)
            assert frames.shape == (len(names), H, W) and len(where) == len(names)
            for ch in range(3):
                if where[0][ch] is None:
                    continue
                for wi in mf.key_windows(nwin):
                    assert sorted(where[z][ch][wi] for z in range(len(names))) == sorted(names), (lever, W, H, ch, wi)
    # the three planes of a ycc mosaic hold different recipes in every window
    _, where = mf.build_frames("ycc", mf.RECIPE_SETS[8], 1, 40, 104)
    assert all(len({wy[i], wb[i], wr[i]}) == 3 for wy, wb, wr in where for i in range(65))


@pytest.fixture(scope="module")
def built(oracle):
    """Every case with its reference, by class name."""
    out = {name: [] for name in SSIM_CLASSES}
    for case in mf.cases():
        out[case["cls"]].append((case, mf.reference(oracle, case)))
    return out


def test_the_q_table_holds_at_every_window_position(built):
    """Position independence of the reference: wherever a recipe of the table sits in a mosaic of a HOLD plan, in whichever
    layout and frame of the batch, the Y channel's q is the table's."""
    hits = {k: 0 for k in mf.Q_TABLE}
    for name in ("fast<f1>", "fast<f2>", "gen<hold>", "gen<hold,ycc-in>"):
        for case, ref in built[name]:
            if case["lever"] == "palette":
                continue
            for z, (wy, _, _) in enumerate(ref["where"]):
                qy = ref["map"][z, 3].reshape(-1)
                for wi, rname in enumerate(wy):
                    key = (rname, case["bits"][0], case["f"])
                    if key in mf.Q_TABLE:
                        assert qy[wi] == mf.Q_TABLE[key], (mf.case_key(case), z, wi, rname)
                        hits[key] += 1
    assert all(hits.values()), [k for k, n in hits.items() if not n]


def _window_facts(orc, case, ref):
    """Of the one-window layout: per frame and channel (q, s1, s2, 64 |N|, D >> 10), N and D in exact Python integers."""
    out = []
    for z, frame in enumerate(ref["frames"]):
        for ch, (x, y) in enumerate(_pairs(orc, frame, 8, 8, case)):
            xw, yw = _windows(x)[0, 0], _windows(y)[0, 0]
            n, d = float_ssim(xw, yw)
            out.append((int(ref["map"][z, ch, 0, 0]), ch, int(xw.sum()), int(yw.sum()), 64 * abs(n), d >> 10, bool((xw == xw[0]).all())))
    return out


@pytest.mark.parametrize("name", SSIM_CLASSES)
def test_coverage_of_the_built_set(oracle, built, name):
    """Conditions on the built set, per SSIM kernel class (not measurements): the corners of ssim_q / div_exact and of the packed sums
    that noise does not reach.  The minima of the chroma channels the reference gives (recorded, not fixed in advance):
      fast<f1>          Cb -56128, Cr -38849        fast<f2>          Cb -32592, Cr -32592
      gen<hold>         Cb -57124, Cr -57124        gen<hold,ycc-in>  Cb -57126, Cr -57126
    (asserted here only as negative; test_recorded_chroma_minima holds the figures)."""
    facts = [t for case, ref in built[name] if (case["W"], case["H"]) == (8, 8) for t in _window_facts(oracle, case, ref)]
    qs = np.concatenate([ref["map"].reshape(-1) for _, ref in built[name]])
    assert any(q == ONE and not const for q, ch, s1, s2, n64, d10, const in facts), "q == 65536 on a window that is not constant"
    assert (qs == 0).any()
    assert ((qs != 0) & (np.abs(qs) < 256)).any()
    assert any(s2 == 0 and s1 > 0 for q, ch, s1, s2, n64, d10, const in facts)
    assert max(n64 for q, ch, s1, s2, n64, d10, const in facts) >= 2 ** 59
    assert max(n64 for q, ch, s1, s2, n64, d10, const in facts) < 2 ** 63
    assert 2 ** 44 <= max(d10 for q, ch, s1, s2, n64, d10, const in facts) < 2 ** 47
    assert any(s1 == 16320 and s2 == 16320 for q, ch, s1, s2, n64, d10, const in facts)
    if name in ("gen<hold>", "gen<hold,ycc-in>"):
        assert qs.min() <= -50000
    if name == "fast<f2>":
        assert qs.min() <= -30000
    if name.startswith("fast") or name == "gen<hold,ycc-in>":
        for ch in (4, 5):
            low = min(int(ref["map"][:, ch].min()) for _, ref in built[name])
            assert low < 0, (name, ch, low)


def test_recorded_chroma_minima(built):
    """The figures of test_coverage_of_the_built_set's docstring are what the reference gives."""
    want = {"fast<f1>": (-56128, -38849), "fast<f2>": (-32592, -32592), "gen<hold>": (-57124, -57124), "gen<hold,ycc-in>": (-57126, -57126)}
    for name, lows in want.items():
        assert tuple(min(int(ref["map"][:, ch].min()) for _, ref in built[name]) for ch in (4, 5)) == lows, name


# ---- distortion ------------------------------------------------------------------------------------
def test_held_white_at_factor_8_is_the_maximal_error_frame(oracle):
    """Every output pixel's 8 x 8 block holds 63 black pixels against a white output: 63 * 255^2 per lane of k_dist_gen in Y (and
    R, G, B), 64 lanes of it in a wave -- the sum the 32-bit lane and wave accumulators are said to hold."""
    W = H = 128
    p, _ = mf.mosaic(("held_white",), 8, W, H)
    for op in ORDERS:
        c = dict(mf._cls("gen<hold>", 2, 0, 8, op), bits=(8, 8, 8))
        x, y = _pairs(oracle, mf.gray(p), W, H, c)[3]
        per_output = ((x - y) ** 2).reshape(16, 8, 16, 8).sum(axis=(1, 3))
        assert (per_output == 63 * 65025).all()
        assert 64 * 63 * 65025 == 262180800 < 2 ** 32
        sse, _, _ = mf.measure(oracle, mf.gray(p), W, H, c)
        assert sse == [256 * 63 * 65025] * 4 + [0, 0]


def test_palette_frames_give_the_stated_chroma_errors(oracle):
    """`cols` in the Cb pair (blue at even columns, yellow at odd ones) under a horizontal hold of 2 or 4: every yellow pixel is
    measured against blue's Cb, 254^2 each; in the Cr pair red against cyan the same in Cr.  Under 4:4:4 nothing is lost."""
    for pair, ch in ((0, 4), (1, 5)):
        frame = mf.palette(mf.recipe("cols"), np.full((8, 8), pair))
        for rounding in (0, 1):
            for (a, b), lost in (((4, 4), 0), ((2, 2), 32), ((1, 1), 32), ((2, 0), 32)):
                c = dict(mf._cls("fast<f1>", a, b, 1, mf.CSQ, rounding), bits=(8, 8, 8))
                sse, _, _ = mf.measure(oracle, frame, 8, 8, c)
                assert sse[ch] == lost * 254 ** 2 and sse[3] == 0, (pair, rounding, a, b, sse)
    # `rows` under 4:4:0: the odd rows (yellow) replay the last sample of the even row above (blue)
    frame = mf.palette(mf.recipe("rows"), np.zeros((8, 8), dtype=int))
    sse, _, _ = mf.measure(oracle, frame, 8, 8, dict(mf._cls("fast<f1>", 4, 0, 1), bits=(8, 8, 8)))
    assert sse[4] == 32 * 254 ** 2 and sse[5] == 32 * (149 - 107) ** 2


# ---- the replay pair -------------------------------------------------------------------------------
@pytest.mark.parametrize("lever,in_format", [("palette", mf.ARGB), ("ycc", mf.YCC)])
@pytest.mark.parametrize("a,b", [(2, 0), (4, 0), (1, 0)])
@pytest.mark.parametrize("W", [40, 43])
def test_the_replay_pair_differs_in_its_odd_rows_as_described(oracle, lever, in_format, a, b, W):
    H = 16
    h = mf.HOLD[a, b][0]
    col = (W - 1) // h * h
    c = dict(mf._cls("x", a, b, 1, in_format=in_format), bits=(8, 8, 8))
    on, off = (mf.replay_frames(W, H, h, lever, shift) for shift in (0, 1))
    assert (on != off).sum() == 2 * (H // 2) and (on[1::2] == off[1::2]).all()
    p_on, p_off = _pairs(oracle, on, W, H, c), _pairs(oracle, off, W, H, c)
    for ch in (4, 5):
        (x_on, y_on), (x_off, y_off) = p_on[ch], p_off[ch]
        assert (x_on[1::2] == 128).all() and (x_off[1::2] == 128).all()                  # the odd rows' own chroma is neutral
        # frame 0: the one pixel above decides the whole odd row; frame 1: the odd rows measure as neutral
        assert np.array_equal(y_on[1::2], np.repeat(x_on[0::2, col:col + 1], W, axis=1))
        assert (y_on[1::2] != 128).all() and (y_off[1::2] == 128).all()
        # the even rows hold their own samples: neutral but for the hold group of the extreme pixel
        assert (y_on[0::2, :col] == 128).all() and np.array_equal(y_on[0::2, col], x_on[0::2, col])
    sse_on, sse_off = (mf.measure(oracle, fr, W, H, c)[0] for fr in (on, off))
    assert sse_on[4] > sse_off[4] and sse_on[5] > sse_off[5]
