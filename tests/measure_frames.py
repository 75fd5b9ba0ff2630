"""Input frames built to order for the measurement units (csic_distortion_*, csic_ssim_*).  The units are fused: a kernel reads the
input frame, forms the plan's output in registers and emits only sums and the map of quotients, so the (reference, output) pairs its
arithmetic meets are whatever the pipeline makes of the input.  Three levers dictate them:

  gray     ARGB pixels with R = G = B = v: Y == v, Cb == Cr == 128 under both roundings, so the Y channel sees exactly
           (v, out(v) & y_mask) with out() the plan's hold or average (y_pairs_closed_form); R, G, B come along through the
           inverse transform and hit its clamp.
  ycc      YCbCr input (in_format = YCBCR888X): the three reference channels are the input bytes, one dictated plane each.
  palette  four ARGB colours, blue / yellow (Cb 255 / 1) and red / cyan (Cr 255 / 1): near-maximal chroma contrast for the
           kernels that take ARGB input only.

A frame is a mosaic of 8 x 8 recipe windows (recipe()); mosaic() returns it with the recipe that sits in each window.  This module
holds numpy closed forms of the recipes and of the Y lever only -- NO copy of the definitions: expected sums and maps come from
oracle_sse / oracle_ssim (sse_numpy / ssim_numpy on the oracle's outputs) through reference(), which computes each case once and
is shared by tests/test_measure_frames_host.py (which proves the levers, the q table and the coverage of the built set on the
CPU) and tests/test_gpu_measure_frames.py."""
import itertools

import numpy as np

from test_distortion_host import oracle_params, sse_numpy
from test_ssim_host import ssim_numpy

ARGB, YCC = 0, 1
CSQ, SCQ = (3, 1, 2), (1, 3, 2)                 # chroma before spatial, spatial before chroma: one order of each class
CHROMA = [(4, 4), (2, 2), (2, 0), (1, 1), (4, 0), (1, 0)]
HOLD = {(4, 4): (1, 1), (2, 2): (2, 1), (2, 0): (2, 2), (1, 1): (4, 1), (4, 0): (1, 2), (1, 0): (4, 2)}      # (a, b) -> (h, v)
NEUTRAL = 128

# the palette: ARGB colour -> (Cb, Cr) under rounding 0 / 1 (Y is whatever the colour gives)
BLUE, YELLOW, RED, CYAN = 0xFF0000FF, 0xFFFFFF00, 0xFFFF0000, 0xFF00FFFF
PALETTE_CHROMA = {BLUE: ((255, 107), (255, 108)), YELLOW: ((1, 149), (1, 149)), RED: ((85, 255), (86, 255)), CYAN: ((171, 1), (171, 1))}
PAIRS = ((BLUE, YELLOW), (RED, CYAN))           # (colour of pattern >= 128, colour of pattern < 128): the Cb pair, the Cr pair

_I, _J = np.mgrid[0:8, 0:8]


# ---- recipes: 8 x 8 byte patterns P(i, j), row i, column j -------------------------------------
def recipe(name, f=1):
    """The pattern of recipe `name` at factor f ("held": i % f == 0 and j % f == 0), (8, 8) int64."""
    held = (_I % f == 0) & (_J % f == 0)
    full = lambda v: np.full((8, 8), v, dtype=np.int64)
    if name.startswith("const"):
        return full(int(name[5:]))
    if name == "neutral":
        return full(NEUTRAL)
    if name == "step127_128":
        return 127 + ((_I + _J) & 1)
    if name == "checker":
        return 255 * ((_I + _J) & 1)
    if name == "half":
        return 255 * (_J >> 2)
    if name == "held_white":
        return np.where(held, 255, 0)
    if name == "held_black":
        return np.where(held, 0, 255)
    if name == "dots":                          # 48 white pixels of 64 at every factor: lossless at factor 1, where D is largest
        return np.where((_I % 2 == 0) & (_J % 2 == 0), 0, 255)
    if name == "anti":
        a = 255 * (((_I // f) + (_J // f)) & 1)
        return np.where(held, a, 255 - a)
    if name in ("cols", "cols_c", "pairs", "pairs_c", "quads_c", "rows", "rows_c"):
        bit = {"cols": _J & 1, "pairs": (_J >> 1) & 1, "quads": (_J >> 2) & 1, "rows": _I & 1}[name.split("_")[0]]
        return 255 * (bit if name.endswith("_c") else 1 - bit)          # cols: 255 at even columns; cols_c: 255 at odd columns
    if name == "ramp":
        return 10 * _J + 3 * _I
    if name in ("band_low", "band_high"):
        v = np.random.default_rng(0xBA2D).integers(0, 4, (8, 8))
        return v if name == "band_low" else 252 + v
    raise KeyError(name)


# The recipes of a mosaic by quantiser width (the same for the three channels): each set ends with the neutral filler.
RECIPE_SETS = {
    8: ("const0", "const255", "checker", "half", "held_white", "held_black", "anti", "cols", "cols_c", "band_low", "band_high", "dots", "neutral"),
    1: ("const127", "step127_128", "const255", "neutral"),
    4: ("ramp", "band_high", "neutral"),
    6: ("band_low", "band_high", "neutral"),
}
# the two-valued recipes the palette lever can carry; cols .. rows_c alternate inside and across the 4-pixel hold groups
PALETTE_SET = ("const0", "const255", "checker", "half", "held_white", "anti", "cols", "cols_c", "pairs", "pairs_c", "quads_c", "rows", "rows_c")

# q of the Y channel under HOLD: (recipe, y_bits, f) -> q, computed from the definition in tests/test_ssim_host.py
Q_TABLE = {("const0", 8, f): 65536 for f in (1, 2, 4, 8)}
Q_TABLE.update({("const255", 8, f): 65536 for f in (1, 2, 4, 8)})
Q_TABLE.update({("const127", 1, f): 0 for f in (1, 2, 4, 8)})
Q_TABLE.update({("step127_128", 1, 1): 1538, ("checker", 8, 1): 65536, ("ramp", 4, 1): 63346})
Q_TABLE.update({("half", 8, f): 65536 for f in (1, 2, 4)})
Q_TABLE.update({("held_white", 8, 2): 145, ("held_white", 8, 4): 121, ("held_white", 8, 8): 111})
Q_TABLE.update({("held_black", 8, f): 0 for f in (2, 4, 8)})
Q_TABLE.update({("anti", 8, 2): -32594, ("anti", 8, 4): -57126, ("cols", 8, 2): 185, ("cols_c", 8, 2): 0})

# (W, H) of the window layouts: one window; 31; 32, exactly one block; 33, one real window in the second block; nwx = 1; 5 x 13
LAYOUTS = ((8, 8), (248, 8), (256, 8), (264, 8), (8, 264), (40, 104))
WPB = 32                                        # windows per block of the SSIM kernels


def key_windows(nwin):
    """The first window, the last one and the windows on each side of every block edge."""
    edges = [w for e in range(WPB, nwin, WPB) for w in (e - 1, e)]
    return sorted({0, nwin - 1, *edges})


# ---- the levers ------------------------------------------------------------------------------------
def gray(p):
    p = np.asarray(p).astype(np.uint32)
    return np.uint32(0xFF000000) | (p * np.uint32(0x010101))


def ycc(y, cb, cr):
    return np.asarray(y).astype(np.uint32) | (np.asarray(cb).astype(np.uint32) << 8) | (np.asarray(cr).astype(np.uint32) << 16)


def palette(p, pair):
    """pair: (H, W) array of 0 / 1, the Cb or the Cr pair of PAIRS per pixel."""
    hi = np.where(np.asarray(pair) == 0, np.uint32(PAIRS[0][0]), np.uint32(PAIRS[1][0]))
    lo = np.where(np.asarray(pair) == 0, np.uint32(PAIRS[0][1]), np.uint32(PAIRS[1][1]))
    return np.where(np.asarray(p) >= 128, hi, lo).astype(np.uint32)


def y_pairs_closed_form(p, f, y_bits, avg=False):
    """The Y channel's (reference, output) pair of every pixel of a gray frame with pattern p (H, W): the output is the held pixel
    (r - r % f, c - c % f) under HOLD, whatever the order and the chroma mode; under AVG the mean of the f x f block, coordinates
    clamped to the frame, rounded half up; either one cut to its top y_bits."""
    p = np.asarray(p, dtype=np.int64)
    H, W = p.shape
    r, c = np.arange(H), np.arange(W)
    if avg:
        rr = np.minimum((r // f * f)[:, None] + np.arange(f)[None, :], H - 1)              # (H, f)
        cc = np.minimum((c // f * f)[:, None] + np.arange(f)[None, :], W - 1)
        out = (p[rr[:, None, :, None], cc[None, :, None, :]].sum(axis=(2, 3)) + f * f // 2) // (f * f)
    else:
        out = p[(r // f * f)[:, None], (c // f * f)[None, :]]
    return p, out & (0xFF00 >> y_bits & 0xFF)


# ---- mosaics ---------------------------------------------------------------------------------------
def mosaic(names, f, W, H, rot=0):
    """A (H, W) pattern tiled with recipe windows, cut at the right and bottom edge where W or H is no multiple of 8: the tile in tile
    row ty, tile column tx holds names[(ty * ceil(W / 8) + tx + rot) % len(names)].  Returns (pattern int64 (H, W), the recipe
    names of the WHOLE windows, row-major, as the SSIM map numbers them)."""
    nty, ntx = -(-H // 8), -(-W // 8)
    p = np.zeros((8 * nty, 8 * ntx), dtype=np.int64)
    where = []
    for ty in range(nty):
        for tx in range(ntx):
            name = names[(ty * ntx + tx + rot) % len(names)]
            p[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8] = recipe(name, f)
            if 8 * ty + 8 <= H and 8 * tx + 8 <= W:
                where.append(name)
    return p[:H, :W], where


def build_frames(lever, names, f, W, H):
    """len(names) frames (rotation z in frame z, so that every recipe passes through every window) -> (frames uint32 (n, H, W),
    where[z][channel] = the recipe names per window of Y, Cb, Cr (None for a channel the lever does not dictate))."""
    frames, where = [], []
    n = len(names)
    for z in range(n):
        p, wy = mosaic(names, f, W, H, z)
        if lever == "gray":
            frames.append(gray(p))
            where.append((wy, None, None))
        elif lever == "ycc":
            pb, wb = mosaic(names, f, W, H, z + 1)                   # the three planes hold different recipes in every window
            pr, wr = mosaic(names, f, W, H, z + 2)
            frames.append(ycc(p, pb, pr))
            where.append((wy, wb, wr))
        elif lever == "palette":
            win = (np.arange(H)[:, None] // 8) * -(-W // 8) + np.arange(W)[None, :] // 8
            frames.append(palette(p, (win + z) & 1))                 # the Cb and the Cr pair alternate from window to window
            where.append((None, wy, wy))
        else:
            raise KeyError(lever)
    return np.stack(frames).astype(np.uint32), where


# ---- the kernel classes and the cases ----------------------------------------------------------------
def _cls(name, a, b, f, op=CSQ, rounding=0, avg=False, in_format=ARGB, force=False):
    return dict(cls=name, a=a, b=b, f=f, op=op, rounding=rounding, avg=avg, in_format=in_format, force=force)


def classes():
    """One parameter set per kernel class and variant of it: the class name is measure_kernel_name's without the unit's stem.
    `force` = reached under CSIC_TUNE_FORCE_GENERIC (chroma before spatial at factor 2 on whole windows is the fast class)."""
    out = [_cls(f"fast<f{f}>", a, b, f, CSQ, rounding) for f in (1, 2) for a, b in CHROMA for rounding in (0, 1)]
    out += [_cls("gen<hold>", a, b, f, op, rounding, force=(f == 2 and op == CSQ))
            for (f, op), (a, b), rounding in zip(itertools.product((2, 4, 8), (CSQ, SCQ)), [(2, 0), (1, 0), (4, 0), (2, 2), (1, 1), (2, 0)], (0, 1, 1, 0, 0, 1))]
    out += [_cls("gen<hold,ycc-in>", a, b, f, op, in_format=YCC)
            for f, op, (a, b) in zip((1, 2, 4, 8), (CSQ, SCQ, CSQ, SCQ), [(2, 0), (1, 0), (4, 0), (1, 1)])]
    out += [_cls("gen<avg>", a, b, f, CSQ, rounding, avg=True) for f, (a, b), rounding in zip((1, 2, 4, 8), [(2, 0), (4, 4), (1, 0), (2, 2)], (0, 1, 0, 1))]
    out += [_cls("gen<avg,ycc-in>", a, b, f, CSQ, avg=True, in_format=YCC) for f, (a, b) in zip((1, 2, 4), [(1, 0), (2, 0), (4, 4)])]
    return out


def class_id(c):
    return "{cls}-{a}{b}-f{f}-{o}-r{rounding}".format(o="".join(map(str, c["op"])), **c)


def levers_of(c):
    """(lever, bits, recipe names) of every mosaic set a class is run on."""
    if c["in_format"] == YCC:
        return [("ycc", q, RECIPE_SETS[q]) for q in (8, 1, 4, 6)]
    return [("gray", q, RECIPE_SETS[q]) for q in (8, 1, 4, 6)] + [("palette", 8, PALETTE_SET)]


def cases(cls_list=None):
    """Every (class, lever set, layout): the list the host module counts and the GPU module runs."""
    return [dict(c, lever=lever, bits=(q, q, q), names=names, W=W, H=H)
            for c in (classes() if cls_list is None else cls_list) for lever, q, names in levers_of(c) for W, H in LAYOUTS]


def case_key(case):
    return (class_id(case), case["lever"], case["bits"], case["W"], case["H"])


def oracle_kw(case):
    return dict(a=case["a"], b=case["b"], bits=case["bits"], f=case["f"], op=case["op"], rounding=case["rounding"], in_format=case["in_format"])


def oracle_outputs(orc, frame, W, H, case):
    """The oracle's packed (ARGB, YCbCr) outputs of one frame under a case's (or class's) parameters."""
    form = "avg" if case["avg"] else "stream"
    return [orc.process(oracle_params(orc, W, H, fmt=fmt, **oracle_kw(case)), frame, form=form) for fmt in (orc.FMT_ARGB, orc.FMT_YCC)]


def measure(orc, frame, W, H, case):
    """(sse[6], ssim sums[6], ssim map (6, H / 8, W / 8)) of one frame: sse_numpy and ssim_numpy on the oracle's outputs."""
    frame = np.asarray(frame, dtype=np.uint32).reshape(H, W)
    o_rgb, o_ycc = oracle_outputs(orc, frame, W, H, case)
    sse = sse_numpy(frame, o_rgb, o_ycc, case["f"], case["rounding"], case["in_format"])
    if W < 8 or H < 8:
        return sse, None, None
    sums, qmap = ssim_numpy(frame, o_rgb, o_ycc, case["f"], case["rounding"], case["in_format"])
    return sse, sums, qmap


_REFERENCE = {}


def reference(orc, case):
    """The frames of a case with what the units must measure on them, computed once per process and left unchanged:
    dict(frames (n, H, W), where, sse (n, 6) uint64, sums (n, 6) int64, map (n, 6, H / 8, W / 8) int32)."""
    key = case_key(case)
    if key not in _REFERENCE:
        frames, where = build_frames(case["lever"], case["names"], case["f"], case["W"], case["H"])
        m = [measure(orc, fr, case["W"], case["H"], case) for fr in frames]
        ref = dict(frames=frames, where=where, sse=np.array([x[0] for x in m], dtype=np.uint64),
                   sums=np.array([x[1] for x in m], dtype=np.int64), map=np.stack([x[2] for x in m]).astype(np.int32))
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFERENCE[key] = ref
    return _REFERENCE[key]


# ---- the replay pair -------------------------------------------------------------------------------
def replay_frames(W, H, h, lever, shift):
    """Two-frame material of the 4:x:0 replay row at factor 1: every pixel has neutral chroma (gray 128 / YCbCr (128, 128, 128)),
    except that column last_sample_col - shift of each even row carries an extreme chroma -- the palette's four colours in turn
    (ARGB) or Cb / Cr in {0, 255} in turn (YCbCr).  shift = 0: that one pixel decides the chroma of the whole odd row below;
    shift = 1: nothing takes its chroma from it but (where it is a sample point) pixels of its own row."""
    col = (W - 1) // h * h - shift
    if lever == "palette":
        frame = np.full((H, W), 0xFF808080, dtype=np.uint32)
        frame[0::2, col] = np.resize(np.array([BLUE, RED, YELLOW, CYAN], dtype=np.uint32), len(range(0, H, 2)))
        return frame
    cb, cr = np.full((H, W), NEUTRAL), np.full((H, W), NEUTRAL)
    k = len(range(0, H, 2))
    cb[0::2, col] = np.resize([255, 0, 255, 0], k)
    cr[0::2, col] = np.resize([0, 0, 255, 255], k)
    return ycc(np.full((H, W), NEUTRAL), cb, cr)
