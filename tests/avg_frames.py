"""Input frames built to order for the AVG sampling extension (box-filtered chroma, then f x f pooling: k_avg with its edge blocks,
k_avg_generic, k_planar_avg_f1, k_planar_avg_tile, k_planar_avg_gen, k_pbits_gen<avg>), a numpy statement of its definition with
switchable faults, and the levers that dictate one channel at a time.

  ref_avg   the definition of include/csic.h and of the comment above orc_process_avg, vectorised: clamped index arrays, block sums
            by reshaping.  `fault` switches in ONE deliberate error (FAULTS), so that tests/test_avg_frames_host.py can prove on
            the CPU that the built frames would notice it.  The norm stays orc_process_avg: the host test holds ref_avg to it.
  levers    gray(v): Y = v, Cb = Cr = 128 under both roundings.  colour_for_cb[rounding][c] / colour_for_cr[rounding][c], c = 1 .. 255:
            an ARGB colour whose Cb (Cr) is c, with the other channel as near to 128 as the cube allows; other_of_cb / other_of_cr
            record what the other channel turned out to be.  Built from the whole colour cube once per process.

Four sets of frames:
  cube      cube(): all 2^24 colours as 4096 x 4096.
  palette   palette(): at most 4096 colours as a 64-wide image -- the corners of the forward transform's chroma arithmetic
            (palette_parts()); magnified() / magnified_cut() blow every colour up to one max(f, h) x max(f, v) region, so that the
            AVG output is the closed form of the palette image itself (a second opinion on the oracle).
  windows   windows_frame(): a mosaic of 8 x 8 recipe windows (window_recipes), one channel dictated per window.
  residues  residue_shapes() x RESIDUE_CONTENTS: every (W mod 8, H mod max(f, v)) of an instantiation, at most 23 x 23.
Expected outputs are NOT taken from this module by the GPU tests: they come from the oracle."""
import functools

import numpy as np

ARGB, YCC = 0, 1
FLOOR, TRUNC = 0, 1
MODES = [(4, 4), (2, 2), (2, 0), (1, 1), (4, 0), (1, 0)]
HV = {(4, 4): (1, 1), (2, 2): (2, 1), (2, 0): (2, 2), (1, 1): (4, 1), (4, 0): (1, 2), (1, 0): (4, 2)}          # (a, b) -> (h, v)
FACTORS = (1, 2, 4, 8)
MODE_FACTORS = [(a, b, f) for a, b in MODES for f in FACTORS]                                            # the 24 instantiations
FAULTS = ("no_clamp", "trunc_threshold_32512", "block_half_missing", "pool_half_missing", "one_stage", "edge_virtual_block",
          "edge_no_row_hold", "f8_left_half_twice")
BIAS = 32896                                    # ub = cbI + BIAS, ur = crI + BIAS: the biased dot products of fwd_c / fwd_c_pk

_I, _J = np.mgrid[0:8, 0:8]


def _ilog2(x):
    return int(x).bit_length() - 1


# ---- the forward transform -------------------------------------------------------------------------
def forward(px, rounding, fault=None):
    """(Y, Cb, Cr, ub, ur) of ARGB pixels, int32 arrays of px's shape: RGB2YCbCr with `(x + 128) >> 8` (FLOOR) or `(x + 128) / 256`
    rounding toward zero (TRUNC), + 128, clamped to 0 .. 255.  ub, ur are the numerators before the division, biased as the device
    code has them (>= 0).  Faults: no_clamp keeps a quotient of 256; trunc_threshold_32512 rounds toward zero only below u = 32512."""
    px = np.asarray(px, dtype=np.uint32)
    r, g, b = ((px >> 16) & 255).astype(np.int32), ((px >> 8) & 255).astype(np.int32), (px & 255).astype(np.int32)
    y = (77 * r + 150 * g + 29 * b + 128) >> 8
    nb, nr = -43 * r - 85 * g + 128 * b, 128 * r - 107 * g - 21 * b
    return y, _chroma(nb, rounding, fault), _chroma(nr, rounding, fault), nb + BIAS, nr + BIAS


def _chroma(num, rounding, fault=None):
    """A chroma numerator (int32) -> the channel's value."""
    t = num + 128
    if rounding == TRUNC:
        neg = t < (-256 if fault == "trunc_threshold_32512" else 0)
        q = np.where(neg, -((-t) >> 8), t >> 8) + 128
    else:
        q = (t >> 8) + 128
    q = np.maximum(q, 0)
    return q if fault == "no_clamp" else np.minimum(q, 255)


@functools.lru_cache(maxsize=None)
def _cube_raw_numerators():
    """The two chroma numerators of the 2^24 colours in cube order (colour = R << 16 | G << 8 | B), from three 256-entry ramps."""
    k = np.arange(256, dtype=np.int32)
    r, g, b = k[:, None, None], k[None, :, None], k[None, None, :]
    return (-43 * r - 85 * g + 128 * b).reshape(-1), (128 * r - 107 * g - 21 * b).reshape(-1)


def inverse(y, cb, cr):
    """YCbCr2RGB -> packed ARGB, uint32."""
    c, d, e = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = np.clip((298 * c + 409 * e + 128) >> 8, 0, 255).astype(np.uint32)
    g = np.clip((298 * c - 100 * d - 208 * e + 128) >> 8, 0, 255).astype(np.uint32)
    b = np.clip((298 * c + 516 * d + 128) >> 8, 0, 255).astype(np.uint32)
    return np.uint32(0xFF000000) | (r << 16) | (g << 8) | b


# ---- the definition, vectorised ------------------------------------------------------------------------
def ref_avg(frame, W, H, a, b, bits, f, rounding, fmt, fault=None, detail=False):
    """The AVG output of one ARGB frame, (Ho, Wo) uint32; with detail=True also a dict of intermediates: ub, ur (H, W), block_sums
    (Cb, Cr) of the chroma blocks whose origin lies in the frame, pool_sums (Y, Cb, Cr) of the output pixels.

    Chroma stage: the h x v block of pixel (r, c) starts at (r - r % v, c - c % h); its pixels are read at coordinates clamped to the
    frame; Cb' = (sum + n / 2) >> log2 n, n = h v.  Spatial stage: output (ro, co) sums the f x f pixels from (ro f, co f), coordinates
    clamped to the frame -- a pixel beyond the frame IS the clamped pixel, with that pixel's own block average -- and rounds
    (sum + f f / 2) >> 2 log2 f.  Then the quantiser, then the inverse transform for ARGB output."""
    assert fault is None or fault in FAULTS, fault
    px = np.asarray(frame, dtype=np.uint32).reshape(H, W)
    h, v = HV[a, b]
    n, nlog, flog2 = h * v, _ilog2(h * v), 2 * _ilog2(f)
    y, cb, cr, ub, ur = forward(px, rounding, fault)
    RW, RH = max(f, h), max(f, v)
    Wp, Hp = -(-W // RW) * RW, -(-H // RH) * RH                               # the frame padded to whole regions ...
    ri, ci = np.minimum(np.arange(Hp), H - 1), np.minimum(np.arange(Wp), W - 1)     # ... through clamped coordinates
    Wo, Ho = -(-W // f), -(-H // f)
    bhalf = 0 if fault == "block_half_missing" else n >> 1
    phalf = 0 if fault == "pool_half_missing" else (f * f) >> 1

    def pool(x):                                                              # x: (Hp, Wp) -> the sums of its f x f blocks
        if fault == "f8_left_half_twice" and f == 8:
            return 2 * x.reshape(Hp // 8, 8, Wp // 8, 8)[:, :, :, :4].sum(axis=(1, 3))
        return x.reshape(Hp // f, f, Wp // f, f).sum(axis=(1, 3))

    def per_pixel(blocks):                                                    # one value per block -> one per pixel of the padded frame
        return np.repeat(np.repeat(blocks, v, axis=0), h, axis=1)

    def held(x):                                                              # the padded frame as the spatial stage sees it
        if fault == "edge_virtual_block":                                     # blocks beyond the frame average their clamped pixels
            return x
        if fault == "edge_no_row_hold":                                       # the last real column is held, the last real row is not
            return x[:, ci]
        return x[ri][:, ci]

    sy = pool(y[ri][:, ci])
    outs, bsums, psums = [(sy + phalf) >> flog2], [], [sy]
    for c in (cb, cr):
        bs = c[ri][:, ci].reshape(Hp // v, v, Wp // h, h).sum(axis=(1, 3))    # sums of the h x v blocks, clamped pixels
        if fault == "one_stage":
            sc = pool(held(per_pixel(bs)))
            o = (sc + ((n * f * f) >> 1)) >> (nlog + flog2)
        else:
            sc = pool(held(per_pixel((bs + bhalf) >> nlog)))
            o = (sc + phalf) >> flog2
        outs.append(o)
        bsums.append(bs[:-(-H // v), :-(-W // h)])
        psums.append(sc)
    masks = [(0xFF00 >> q) & 0xFF for q in bits]
    qy, qb, qr = ((o[:Ho, :Wo] & m).astype(np.uint32) for o, m in zip(outs, masks))
    out = (qy | (qb << 8) | (qr << 16)) if fmt == YCC else inverse(qy, qb, qr)
    if not detail:
        return out
    return out, dict(ub=ub, ur=ur, block_sums=tuple(bsums), pool_sums=tuple(s[:Ho, :Wo] for s in psums))


# ---- the levers ------------------------------------------------------------------------------------
def gray(v):
    v = np.asarray(v).astype(np.uint32)
    return np.uint32(0xFF000000) | (v * np.uint32(0x010101))


@functools.lru_cache(maxsize=None)
def cube_numerators():
    """(ub, ur) of the 2^24 colours in cube order, int32; the same under both roundings."""
    ub, ur = (x + BIAS for x in _cube_raw_numerators())
    for x in (ub, ur):
        x.setflags(write=False)
    return ub, ur


@functools.lru_cache(maxsize=None)
def cube_chroma(rounding):
    """(Cb, Cr) of the 2^24 colours, uint8."""
    cb, cr = (_chroma(x, rounding).astype(np.uint8) for x in _cube_raw_numerators())
    for x in (cb, cr):
        x.setflags(write=False)
    return cb, cr


@functools.lru_cache(maxsize=None)
def _lever_table(rounding, channel):
    """(colour[256] uint32, other[256] int): per value of the channel the first colour of the cube that has it with the other
    chroma channel nearest to 128; colour 0 / other -1 where the cube has none."""
    cb, cr = cube_chroma(rounding)
    mine, other = (cb, cr) if channel == "cb" else (cr, cb)
    flat = mine.astype(np.int32) * 256 + np.abs(other.astype(np.int32) - 128)
    present = np.bincount(flat, minlength=65536).reshape(256, 256) > 0
    targets = (np.arange(256) * 256 + present.argmax(axis=1))[present.any(axis=1)]
    want = np.zeros(65536, dtype=bool)
    want[targets] = True
    idx = np.flatnonzero(want[flat])
    vals, first = np.unique(flat[idx], return_index=True)
    colour, oth = np.zeros(256, dtype=np.uint32), np.full(256, -1, dtype=np.int64)
    colour[vals >> 8] = idx[first].astype(np.uint32) | np.uint32(0xFF000000)
    oth[vals >> 8] = other[idx[first]]
    colour.setflags(write=False)
    oth.setflags(write=False)
    return colour, oth


class _Lever:
    """table[rounding] -> the 256-entry array; built from the cube on first use, then cached."""
    def __init__(self, channel, which):
        self.channel, self.which = channel, which

    def __getitem__(self, rounding):
        return _lever_table(int(rounding), self.channel)[self.which]


colour_for_cb, colour_for_cr = _Lever("cb", 0), _Lever("cr", 0)
other_of_cb, other_of_cr = _Lever("cb", 1), _Lever("cr", 1)


def through_lever(channel, values, rounding):
    """ARGB pixels whose `channel` ("y", "cb", "cr") holds `values` (Y: 0 .. 255, chroma: 1 .. 255)."""
    values = np.asarray(values)
    if channel == "y":
        return gray(values)
    assert values.min() >= 1 and values.max() <= 255
    return (colour_for_cb if channel == "cb" else colour_for_cr)[rounding][values]


# ---- the cube ----------------------------------------------------------------------------------------
def cube():
    return np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)


# ---- the palette -------------------------------------------------------------------------------------
NAMED = (0x000000, 0xFFFFFF, 0xFF0000, 0x00FF00, 0x0000FF, 0x00FFFF, 0xFF00FF, 0xFFFF00)     # black, white, primaries, secondaries
THRESHOLD_U = (32511, 32512, 32513, 32767, 32768, 32769)
LOW_BYTES = (0, 1, 255)
PER_CORNER = 8
PALETTE_WIDTH = 64


def _spread(idx, count):
    """`count` of the indices, first and last included."""
    return idx if len(idx) <= count else idx[np.linspace(0, len(idx) - 1, count).astype(np.int64)]


@functools.lru_cache(maxsize=None)
def palette_parts():
    """The colours (24-bit cube indices) the palette holds, by reason."""
    ub, ur = cube_numerators()
    parts = {"named": np.array(NAMED, dtype=np.int64)}
    parts["high"] = np.flatnonzero((ub >= 65280) | (ur >= 65280))
    for name, u in (("cb", ub), ("cr", ur)):
        for t in THRESHOLD_U:
            parts[name, "u", t] = _spread(np.flatnonzero(u == t), PER_CORNER)
        low = u < 32768
        for lb in LOW_BYTES:
            parts[name, "low byte", lb] = _spread(np.flatnonzero(low & ((u & 255) == lb)), PER_CORNER)
    for rounding in (FLOOR, TRUNC):
        for name, table in (("cb", colour_for_cb), ("cr", colour_for_cr)):
            parts[name, "lever", rounding] = (table[rounding][1:] & np.uint32(0xFFFFFF)).astype(np.int64)
    return parts


@functools.lru_cache(maxsize=None)
def palette():
    """(rows, 64) uint32 ARGB: every colour of palette_parts() once, the last row filled up with gray 128."""
    allc = np.concatenate([np.asarray(p, dtype=np.int64) for p in palette_parts().values()])
    _, first = np.unique(allc, return_index=True)
    colours = allc[np.sort(first)]
    assert len(colours) <= 4096
    rows = -(-len(colours) // PALETTE_WIDTH)
    img = np.full(rows * PALETTE_WIDTH, 0x808080, dtype=np.int64)
    img[:len(colours)] = colours
    img = (img.astype(np.uint32) | np.uint32(0xFF000000)).reshape(rows, PALETTE_WIDTH)
    img.setflags(write=False)
    return img


def magnified(pal, f, h, v):
    """Every pixel of pal as one max(f, h) x max(f, v) region: the AVG output of this frame is the closed form of pal at 4:4:4, factor
    1, each pixel repeated max(f, h) / f x max(f, v) / f times."""
    return np.kron(pal, np.ones((max(f, v), max(f, h)), dtype=np.uint32))


def magnified_cut(pal, f, h, v):
    """magnified() without its last column and last row: the last regions are cut, and the edge path has to complete them."""
    return np.ascontiguousarray(magnified(pal, f, h, v)[:-1, :-1])


def magnified_expectation(closed, f, h, v, cut):
    """The AVG output of magnified() / magnified_cut() from `closed`, the 4:4:4 factor-1 output of the palette image."""
    mx, my = max(f, h), max(f, v)
    out = np.kron(closed, np.ones((my // f, mx // f), dtype=np.uint32))
    if cut:
        H, W = closed.shape[0] * my - 1, closed.shape[1] * mx - 1
        out = out[:-(-H // f), :-(-W // f)]
    return np.ascontiguousarray(out)


# ---- the windows -------------------------------------------------------------------------------------
CHANNELS = ("y", "cb", "cr")
TIE_BASES = {"y": (0, 127, 254), "cb": (1, 127, 254), "cr": (1, 127, 254)}
WINDOWS_PER_ROW = 24


def pool_units(h, v, f):
    """How the chroma blocks divide a pooling block: (unit width, unit height, units per pooling block, the unit's index inside its
    pooling block per pixel of a window).  A unit is a chroma block cut to the pooling block; the spatial stage sums one block average
    per unit, unit-area times."""
    uw, uh = min(h, f), min(v, f)
    return uw, uh, (f // uw) * (f // uh), ((_I % f) // uh) * (f // uw) + (_J % f) // uw


def window_recipes(h, v, f, channel):
    """[(name, (8, 8) pattern of channel values)] for one channel of a plan with chroma blocks h x v and factor f.
      max, min          constant at 255 / at the minimum (0 for Y, 1 for chroma)
      checker<c>        c and c + 1 alternating
      half, half_rows   255 beside the minimum, half and half
      pool<k>of<n>_c<c> in each f x f pooling block the first k pixels are c + 1, the rest c: k = n / 2 - 1, n / 2, n = f f
      block<k>of<n>_c<c> the same in each h x v chroma block, n = h v
      pool_tie_c<c> / pool_below_c<c>   whole chroma blocks at c + 1: half of the units of each pooling block / one unit fewer -- the
                        tie of the spatial stage and the nearest sum below it that block-constant chroma can reach
      two_stage_c<c>    every second unit's chroma blocks hold n / 2 pixels of c + 1 (block average c + 1, true mean c + 1/2), the others
                        are c: two roundings give c + 1, one rounding of the whole sum gives c"""
    lo = 0 if channel == "y" else 1
    if channel == "y":
        h = v = 1
    full = lambda x: np.full((8, 8), x, dtype=np.int64)
    out = [("max", full(255)), ("min", full(lo))]
    out += [(f"checker{c}", c + ((_I + _J) & 1)) for c in TIE_BASES[channel]]
    out += [("half", np.where(_J < 4, 255, lo)), ("half_rows", np.where(_I < 4, 255, lo))]
    if f > 1:
        lin, n = (_I % f) * f + (_J % f), f * f
        out += [(f"pool{k}of{n}_c{c}", c + (lin < k)) for c in TIE_BASES[channel] for k in (n // 2 - 1, n // 2)]
    nb = h * v
    blin = (_I % v) * h + (_J % h)
    if nb > 1:
        out += [(f"block{k}of{nb}_c{c}", c + (blin < k)) for c in TIE_BASES[channel] for k in (nb // 2 - 1, nb // 2)]
    if nb > 1 and f > 1:
        _, _, U, ulin = pool_units(h, v, f)
        if U >= 2:
            for c in TIE_BASES[channel]:
                out.append((f"pool_tie_c{c}", c + (ulin < U // 2)))
                out.append((f"pool_below_c{c}", c + (ulin < U // 2 - 1)))
                out.append((f"two_stage_c{c}", c + (((ulin & 1) == 1) & (blin < nb // 2))))
    return [(name, np.asarray(p, dtype=np.int64)) for name, p in out]


def windows_frame(a, b, f, rounding):
    """(frame (H, 192) uint32, where): the recipes of Y, then Cb, then Cr, one 8 x 8 window each, WINDOWS_PER_ROW to a row of windows,
    the rest of the last row gray 128; where[k] = (channel, recipe name, window row, window column)."""
    h, v = HV[a, b]
    wins = [(ch, name, p) for ch in CHANNELS for name, p in window_recipes(h, v, f, ch)]
    rows = -(-len(wins) // WINDOWS_PER_ROW)
    frame = np.full((8 * rows, 8 * WINDOWS_PER_ROW), 0xFF808080, dtype=np.uint32)
    where = []
    for k, (ch, name, p) in enumerate(wins):
        wy, wx = divmod(k, WINDOWS_PER_ROW)
        frame[8 * wy:8 * wy + 8, 8 * wx:8 * wx + 8] = through_lever(ch, p, rounding)
        where.append((ch, name, wy, wx))
    return frame, where


# ---- the residues ------------------------------------------------------------------------------------
BLUE, YELLOW, RED, CYAN = 0xFF0000FF, 0xFFFFFF00, 0xFFFF0000, 0xFF00FFFF
RESIDUE_CONTENTS = ("random", "loud", "loud_runs")


def residue_shapes(a, b, f):
    """Every (W mod 8, H mod max(f, v)): W = 16 + rw, H = 2 max(f, v) + rh."""
    th = max(f, HV[a, b][1])
    return [(16 + rw, 2 * th + rh) for rw in range(8) for rh in range(th)]


def residue_frame(W, H, content, seed=0):
    """random: random colours.  loud: gray 128 everywhere except the last real column, which alternates blue / yellow, and the last
    real row, which alternates red / cyan -- what is held decides the output.  loud_runs: the same with the colours changing every
    8 pixels, so that no chroma block and no pooling block averages the two colours of a pair back to gray."""
    if content == "random":
        return np.random.default_rng([0xA7E, W, H, seed]).integers(0, 1 << 32, (H, W), dtype=np.uint32)
    step = 1 if content == "loud" else 8
    frame = np.full((H, W), 0xFF808080, dtype=np.uint32)
    frame[:, W - 1] = np.where((np.arange(H) // step) % 2 == 0, np.uint32(BLUE), np.uint32(YELLOW))
    frame[H - 1, :] = np.where((np.arange(W) // step) % 2 == 0, np.uint32(RED), np.uint32(CYAN))
    return frame


def small_shape(f):
    """A frame narrower than one tile (pair of tiles at factor 8): the plans fall to the one-pixel-per-lane kernels."""
    return (7 if f == 8 else 3, 2 * f + 1)
