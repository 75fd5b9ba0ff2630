"""The definition of csic_decode_view_* (include/csic.h) in numpy, over the oracle's packed output replicated to the frame's size
-- csic_decode_*'s frame -- plus the inputs the view tests share and six WRONG rules that those inputs must tell from the right one
(tests/test_view_ref.py proves that they do; tests/test_gpu_view.py compares the kernels with view() on the same inputs).  A helper
module: no tests in here."""
import functools
import itertools
from collections import namedtuple

import numpy as np

ARGB, YCC, PLANAR, BITS = 0, 1, 2, 3
SCALES = (1, 2, 4, 8, 16)
FACTORS = (1, 2, 4, 8)
MODES = [(4, 4), (2, 2), (2, 0), (1, 1), (1, 0)]          # 4:4:4, 4:2:2, 4:2:0, 4:1:1, 4:1:0
CSQ, SCQ = (3, 1, 2), (1, 3, 2)                          # one order of each class: chroma first, spatial first
SHAPES = [(64, 48), (37, 35), (130, 70)]

View = namedtuple("View", "x0 y0 width height scale")
Case = namedtuple("Case", "W H a b bits f op avg kind")   # kind: "noise" or "gradient"


def oracle_params(orc, c, fmt):
    return orc.OracleParams(width=c.W, height=c.H, chroma_a=c.a, chroma_b=c.b, y_bits=c.bits[0], cb_bits=c.bits[1], cr_bits=c.bits[2],
                            factor=c.f, op=c.op, rounding=0, out_format=fmt)


def frame(c):
    """The input frame of a case, ARGB uint32 (H * W): noise, or a vertical gradient (rows differ, columns do not)."""
    rng = np.random.default_rng(7000 + c.W * 131 + c.H * 17 + c.f)
    if c.kind == "noise":
        return rng.integers(0, 1 << 32, c.W * c.H, dtype=np.uint32) | np.uint32(0xFF000000)
    r = np.arange(c.H, dtype=np.uint32)[:, None] * np.uint32(255) // np.uint32(max(c.H - 1, 1))
    px = (r << np.uint32(16)) | ((np.uint32(255) - r) << np.uint32(8)) | (r >> np.uint32(1)) | np.uint32(0xFF000000)
    return np.ascontiguousarray(np.broadcast_to(px, (c.H, c.W))).reshape(-1)


def replicate(o, W, H, f):
    """decode(r, c) = o(r / f, c / f)"""
    return o[np.arange(H)[:, None] // f, np.arange(W)[None, :] // f]


@functools.lru_cache(maxsize=None)
def _decoded_cached(orc, c, fmt):
    d = decoded(orc, c, fmt, frame(c))
    d.flags.writeable = False                      # shared between tests
    return d


def decoded(orc, c, fmt, argb=None):
    """csic_decode_*'s frame of a case: the oracle's packed output in `fmt`, replicated (as _expected of tests/test_gpu_decode.py).
    The frame of the case's own input is computed once and shared."""
    if argb is None:
        return _decoded_cached(orc, c, fmt)
    return replicate(orc.process(oracle_params(orc, c, fmt), argb, form="avg" if c.avg else "stream"), c.W, c.H, c.f)


def _bytes(px):
    return np.stack([(px >> np.uint32(8 * k)) & np.uint32(0xFF) for k in range(4)], axis=-1).astype(np.int64)


def _pack(b):
    b = b.astype(np.uint32)
    return b[..., 0] | (b[..., 1] << np.uint32(8)) | (b[..., 2] << np.uint32(16)) | (b[..., 3] << np.uint32(24))


def box(frame_px, v, rounding=True, clip=False):
    """The definition over a decoded frame (H, W) uint32: sums of the s x s decoded bytes, + s s / 2, >> 2 log2 s.  clip: source
    coordinates past the frame's edge take the edge (only the wrong rules need it)."""
    s = v.scale
    rows = v.y0 + np.arange(v.height * s)
    cols = v.x0 + np.arange(v.width * s)
    if clip:
        rows, cols = np.clip(rows, 0, frame_px.shape[0] - 1), np.clip(cols, 0, frame_px.shape[1] - 1)
    else:
        assert v.x0 >= 0 and v.y0 >= 0 and rows[-1] < frame_px.shape[0] and cols[-1] < frame_px.shape[1], v
    b = _bytes(frame_px[rows[:, None], cols[None, :]]).reshape(v.height, s, v.width, s, 4).sum(axis=(1, 3))
    return _pack((b + ((s * s) >> 1 if rounding else 0)) >> (2 * (s.bit_length() - 1)))


def view(orc, c, v, fmt=ARGB, argb=None):
    """What csic_decode_view_* must give for case c, view v and output format fmt."""
    return box(decoded(orc, c, fmt, argb), v)


def ycc_to_argb(px):
    """YCbCrUtils.ycbcr2rgb on packed YCbCr pixels (Y | Cb << 8 | Cr << 16) -> ARGB, alpha 0xFF."""
    b = _bytes(px)
    y, cb, cr = b[..., 0], b[..., 1] - 128, b[..., 2] - 128
    r = np.clip((298 * y + 409 * cr + 128) >> 8, 0, 255)
    g = np.clip((298 * y - 100 * cb - 208 * cr + 128) >> 8, 0, 255)
    bl = np.clip((298 * y + 516 * cb + 128) >> 8, 0, 255)
    return _pack(np.stack([bl, g, r, np.full_like(r, 255)], axis=-1))


# ---- six wrong rules: each a plausible implementation slip; (orc, case, view) -> ARGB view ---------------------------------------
def wrong_average_first(orc, c, v):
    """the samples are averaged and the mean is inverse-transformed"""
    return ycc_to_argb(box(decoded(orc, c, YCC), v))


def wrong_truncate(orc, c, v):
    return box(decoded(orc, c, ARGB), v, rounding=False)


def wrong_origin(orc, c, v):
    """boxes snapped to the grid of the scale"""
    return box(decoded(orc, c, ARGB), v._replace(x0=v.x0 // v.scale * v.scale, y0=v.y0 // v.scale * v.scale))


def wrong_swap(orc, c, v):
    return box(decoded(orc, c, ARGB), v._replace(x0=v.y0, y0=v.x0), clip=True)


def wrong_no_replication(orc, c, v):
    """source coordinates taken as coordinates of the decimated frame"""
    o = orc.process(oracle_params(orc, c, ARGB), frame(c), form="avg" if c.avg else "stream")
    return box(o, v, clip=True)


def wrong_no_replay(orc, c, v):
    """rows without chroma samples take the sample of their own column, not the last sample of the row above"""
    lay, y, cb, cr = orc.planar(oracle_params(orc, c, ARGB), frame(c), avg=c.avg)
    plain = type(lay).from_buffer_copy(lay)
    plain.replay_last = 0
    return box(replicate(orc.planar_reconstruct(plain, y, cb, cr, ARGB), c.W, c.H, c.f), v)


WRONG_RULES = [wrong_average_first, wrong_truncate, wrong_origin, wrong_swap, wrong_no_replication, wrong_no_replay]


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------
def views_of(W, H, s):
    """The views a W x H frame takes at scale s: the whole frame, one that ends exactly at the right and bottom edges, x0 in {1, 3}
    with y0 odd, and widths 1, 4, 5 and 8 -- those that fit."""
    out = []
    fw, fh = W // s, H // s
    if fw >= 1 and fh >= 1:
        out.append(View(0, 0, fw, fh, s))
    for w, h in ((4, 2), (5, 3)):                                      # flush with the right and bottom edges
        if w * s <= W and h * s <= H:
            out.append(View(W - w * s, H - h * s, w, h, s))
    for (x0, y0), w in zip(((1, 3), (3, 5), (1, 1), (3, 7)), (1, 4, 5, 8)):
        h = min(3, (H - y0) // s)
        if h >= 1 and x0 + w * s <= W:
            out.append(View(x0, y0, w, h, s))
    return out


def sweep_cases():
    """Every scale meets every factor, chroma mode, order class and sampling on the three shapes, spread so that the whole sweep
    stays small: the shape, bit set and input kind rotate with the combination."""
    bitsets = [(8, 8, 8), (6, 5, 5), (3, 3, 2), (1, 1, 1)]
    out = []
    for n, ((a, b), f, (op, avg)) in enumerate(itertools.product(MODES, FACTORS, ((CSQ, False), (SCQ, False), (CSQ, True)))):
        W, H = SHAPES[(n // 3 + n) % 3]
        out.append(Case(W, H, a, b, bitsets[n % 4], f, op, avg, "noise" if n % 2 else "gradient"))
    return out


# the inputs the six wrong rules must be told from the right one on: noise at 4:4:4 8/8/8 (average first, truncation), a vertical
# gradient and noise under 4:2:0 at factors 1 to 4 (origin, swap, replication, replay)
DISCRIMINATING = [Case(130, 70, 4, 4, (8, 8, 8), 1, CSQ, False, "noise"), Case(130, 70, 2, 0, (8, 8, 8), 2, CSQ, False, "gradient"),
                  Case(130, 70, 2, 0, (8, 8, 8), 1, CSQ, False, "noise"), Case(64, 48, 2, 0, (6, 5, 5), 4, SCQ, False, "noise"),
                  Case(37, 35, 1, 0, (8, 8, 8), 2, CSQ, False, "noise")]


def cases_and_views():
    """(case, view) pairs of the GPU sweep."""
    for c in sweep_cases() + DISCRIMINATING:
        for s in SCALES:
            for v in views_of(c.W, c.H, s):
                yield c, v
