"""Planar frames built to order for the readers of CSIC_FMT_PLANAR and CSIC_FMT_PLANAR_BITS (k_recon, k_rbits, k_decode, k_decode_gen, the
k_cstat_* kernels): what a reader sees is chosen here and not left to the forward path -- the codes of every sample, and every byte and
bit the formats do not own.  A helper module without tests: tests/test_plane_frames_host.py proves the builders' conditions and holds
ref_pixels against the oracle on the CPU, tests/test_gpu_plane_frames.py feeds the frames to the device.

Planes are three arrays of CODES (int64, values < 2^q, read-only) in storage order: n = y_width * y_height for Y, chroma_samples for Cb
and Cr.  A `plan` is a csic.Plan or, where there is no device, a HostPlan of the same parameters: only its layouts are read."""
import types

import numpy as np

import csic_amd as csic

N = csic._native
ARGB, YCC, PLANAR, BITS = N.FMT_ARGB8888, N.FMT_YCBCR888X, N.FMT_PLANAR, N.FMT_PLANAR_BITS


# The cases of tests/test_gpu_plane_frames.py, the smallest at which the readers take each of their paths (the reasoning of the comment
# above PLANE_READERS in tests/test_gpu_debug_build.py): 64 x 40 -- module width % 4 == 0, the fast path, whole blocks of the
# straight-line body and a checked rest; 37 x 21 -- every group position by position and the general decode; 36 x 22 -- rows ragged
# against 4 and 8; 30 x 34 at factor 4, spatial before chroma, 4:2:0 -- a partial last chroma row; 5 x 3 and 1 x 1.
CSQ, SCQ = (3, 1, 2), (1, 3, 2)                              # one order of each class: chroma before spatial, spatial before chroma
CHROMA = [(4, 4), (2, 2), (2, 0), (1, 1)]
SHAPES = [(64, 40, 1), (64, 40, 2), (37, 21, 1), (37, 21, 2), (36, 22, 2), (36, 22, 4), (36, 22, 8), (30, 34, 4), (5, 3, 1), (1, 1, 1)]
AVG_SHAPES = [(64, 40, 1), (64, 40, 2)]                      # AVG: replay_last == 0, and hold_v can be 2
TRIPLES = [(8, 8, 8), (7, 6, 5), (1, 1, 1), (3, 8, 2), (5, 3, 7), (4, 4, 4)]         # (the last one so that every width 1 .. 8 occurs)
# sha256 of the R, G, B bytes of the inverse transform over all 2^24 (Y, Cb, Cr), Y slowest: tests/test_oracle_kat.py::test_exhaustive_cube_inverse
INVERSE_CUBE_DIGEST = "83c0ae221be960c1a5a1bc4ea6ecf886dda2e0becaa21c489ca81cdd0da98435"


def combos(W, H, f):
    """[(a, b, order)] that shape (W, H, f) is crossed with."""
    if (W, H, f) == (30, 34, 4):
        return [(2, 0, SCQ)]
    return [(a, b, op) for a, b in CHROMA for op in (CSQ, SCQ)]


def pack_codes(values, q):
    """8-bit sample values -> the plane's ceil(s q / 8) bytes: code v >> (8 - q) at bits [i q, i q + q), LSB first."""
    codes = np.asarray(values, dtype=np.uint8).reshape(-1).astype(np.uint64) >> np.uint64(8 - q)
    s = codes.size
    groups = np.zeros(((s + 7) // 8) * 8, dtype=np.uint64)
    groups[:s] = codes
    acc = (groups.reshape(-1, 8) << (np.arange(8, dtype=np.uint64) * np.uint64(q))).sum(axis=1, dtype=np.uint64)
    return acc.astype("<u8").view(np.uint8).reshape(-1, 8)[:, :q].reshape(-1)[:(s * q + 7) // 8]


def _frame_from_codes(csic, pl, fmt, planes, bits, fill=0xA5):
    """A frame buffer of `fmt` that holds the given codes (one array per plane), everything else `fill`."""
    if fmt == BITS:
        lay = pl.planar_bits_layout
        offs, data = (lay.y_offset, lay.cb_offset, lay.cr_offset), [pack_codes(c.astype(np.uint8) << (8 - q), q) for c, q in zip(planes, bits)]
    else:
        lay = pl.planar_layout
        # the low bits of a PLANAR byte are ignored: set them
        offs, data = (lay.y_offset, lay.cb_offset, lay.cr_offset), [(c.astype(np.uint8) << (8 - q)) | ((1 << (8 - q)) - 1) for c, q in zip(planes, bits)]
    buf = np.full(lay.frame_bytes, fill, dtype=np.uint8)
    for off, d in zip(offs, data):
        buf[off:off + d.size] = d
    return buf


class HostPlan:
    """The layouts of a parameter set, and the two unpackers of csic.Plan over them, where no plan can exist (no device)."""

    def __init__(self, c_params):
        self.c_params = c_params

    planar_layout = csic.Plan.planar_layout
    planar_bits_layout = csic.Plan.planar_bits_layout
    unpack_planar_bits = csic.Plan.unpack_planar_bits
    split_planar = csic.Plan.split_planar


def host_plan(W, H, a=4, b=4, bits=(8, 8, 8), f=1, op=(3, 1, 2), avg=False):
    return HostPlan(csic.make_c_params(W, H, a, b, *bits, f, op, sampling=csic.Sampling.AVG if avg else csic.Sampling.HOLD_DECIMATE))


def bits_of(plan):
    return plan.c_params.y_bits, plan.c_params.cb_bits, plan.c_params.cr_bits


def sample_counts(plan):
    g = plan.planar_layout
    return g.y_width * g.y_height, int(g.chroma_samples), int(g.chroma_samples)


# ---- frames -------------------------------------------------------------------------------------------------------------------------
def _fill_bytes(fill, count):
    """`fill`: a byte value, or a numpy Generator (a seeded random byte stream)."""
    if isinstance(fill, np.random.Generator):
        return fill.integers(0, 256, count, dtype=np.uint8)
    return np.full(count, int(fill), dtype=np.uint8)


def _low_bits(low_bits, q, count):
    mask = (1 << (8 - q)) - 1
    if low_bits is None or (isinstance(low_bits, str) and low_bits == "zeros"):
        return np.zeros(count, dtype=np.uint8)
    if isinstance(low_bits, np.random.Generator):
        return low_bits.integers(0, 256, count, dtype=np.uint8) & np.uint8(mask)
    assert low_bits == "ones", low_bits
    return np.full(count, mask, dtype=np.uint8)


def regions(plan, fmt):
    """Where a frame's bytes are: per plane (offset, bytes that hold samples, bytes a full last chroma row would take, offset of what
    follows, bits of the last sample byte that hold a sample -- 0: all eight)."""
    g = plan.planar_layout
    n, cs, _ = sample_counts(plan)
    full = int(g.chroma_width) * int(g.chroma_height)
    if fmt == BITS:
        lay = plan.planar_bits_layout
        q = (lay.y_bits, lay.cb_bits, lay.cr_bits)
    else:
        lay, q = g, (8, 8, 8)
    offs = (int(lay.y_offset), int(lay.cb_offset), int(lay.cr_offset), int(lay.frame_bytes))
    return [(offs[p], (s * q[p] + 7) // 8, (w * q[p] + 7) // 8, offs[p + 1], (s * q[p]) % 8) for p, (s, w) in enumerate(((n, n), (cs, full), (cs, full)))]


def frame_of(plan, fmt, y, cb, cr, fill, low_bits=None):
    """One frame buffer (uint8, frame_bytes of the plan's planar_layout or planar_bits_layout) that holds the codes y, cb, cr.  `fill`
    -- 0x00, 0xFF or a numpy Generator -- goes everywhere the format does not own: the padding after each plane, the chroma bytes or
    bits behind chroma_samples and, in a BITS frame, the unused high bits of each plane's last byte.  For PLANAR, `low_bits` (None /
    "zeros", "ones" or a Generator) is OR-ed below each code."""
    q3 = bits_of(plan)
    reg = regions(plan, fmt)
    buf = _fill_bytes(fill, reg[2][3])
    for (off, nbytes, _, _, used), c, q, s in zip(reg, (y, cb, cr), q3, sample_counts(plan)):
        c = np.asarray(c).reshape(-1)
        assert c.size == s and (s == 0 or (0 <= c.min() and c.max() < (1 << q))), (c.size, s, q)
        v = c.astype(np.uint8) << (8 - q)
        if fmt == BITS:
            d = pack_codes(v, q)
            if used:
                d[-1] |= buf[off + nbytes - 1] & np.uint8((0xFF << used) & 0xFF)
        else:
            d = v | _low_bits(low_bits, q, s)
        assert d.size == nbytes
        buf[off:off + nbytes] = d
    return buf


def unowned(plan, fmt):
    """{name: (byte indices, mask)} of every region the format does not own and that is not empty."""
    out = {}
    for p, (off, nbytes, full, nxt, used) in enumerate(regions(plan, fmt)):
        name = ("y", "cb", "cr")[p]
        if used:
            out[name + ".high_bits"] = (np.array([off + nbytes - 1]), (0xFF << used) & 0xFF)
        if full > nbytes:
            out[name + ".row_tail"] = (np.arange(off + nbytes, off + full), 0xFF)
        if nxt > off + full:
            out[name + ".padding"] = (np.arange(off + full, nxt), 0xFF)
    return out


# ---- the definition, in numpy -------------------------------------------------------------------------------------------------------
def chroma_sample_index(lay, j):
    """csic.h, csic_planar_layout: the chroma sample that stream position j takes."""
    j = np.asarray(j, dtype=np.int64)
    r, c = j // lay.module_width, j % lay.module_width
    k = (r // lay.hold_v) * lay.chroma_width + c // lay.hold_h
    if lay.replay_last:
        k = np.where(r % lay.hold_v == 0, k, ((r - 1) // lay.hold_v) * lay.chroma_width + lay.chroma_width - 1)
    return k


def ref_pixels(lay, y8, cb8, cr8, fmt):
    """Planes of 8-bit VALUES (BITS: code << (8 - q); PLANAR: the byte as stored) -> the packed pixels (y_height, y_width) uint32 in
    `fmt`: position j takes Y[j] and the chroma sample of chroma_sample_index; ARGB through the inverse transform as
    tests/test_oracle_kat.py::test_exhaustive_cube_inverse writes it, alpha 0xFF; YCC is Y | Cb << 8 | Cr << 16."""
    n = lay.y_width * lay.y_height
    # (one sample per position: k(j) = j, and the gather of 2^24 samples is not worth its time)
    k = slice(None) if lay.hold_h == 1 and lay.hold_v == 1 else chroma_sample_index(lay, np.arange(n, dtype=np.int64))
    y = np.asarray(y8).reshape(-1).astype(np.int32)
    cb, cr = np.asarray(cb8).reshape(-1).astype(np.int32)[k], np.asarray(cr8).reshape(-1).astype(np.int32)[k]
    assert y.size == n
    if fmt == YCC:
        out = y | (cb << 8) | (cr << 16)
    else:
        d, e = cb - 128, cr - 128
        r = np.clip((298 * y + 409 * e + 128) >> 8, 0, 255)
        g = np.clip((298 * y - 100 * d - 208 * e + 128) >> 8, 0, 255)
        b = np.clip((298 * y + 516 * d + 128) >> 8, 0, 255)
        out = (r << 16) | (g << 8) | b | np.int32(-16777216)
    return out.astype(np.int32).view(np.uint32).reshape(lay.y_height, lay.y_width)


def values_of(planes, bits):
    """Codes -> the 8-bit values they stand for."""
    return [np.asarray(c).astype(np.uint8) << (8 - q) for c, q in zip(planes, bits)]


def ref_decode(small, W, H, f):
    """Replication: decode(r, c) = small[r // f, c // f]."""
    return small[np.arange(H)[:, None] // f, np.arange(W)[None, :] // f]


def clamps_fired(y8, cb8, cr8):
    """Which of the inverse transform's six clamps fire on the triples: {"r_lo", "r_hi", "g_lo", "g_hi", "b_lo", "b_hi"}."""
    y, d, e = (np.asarray(v).reshape(-1).astype(np.int64) - o for v, o in zip((y8, cb8, cr8), (0, 128, 128)))
    raw = {"r": (298 * y + 409 * e + 128) >> 8, "g": (298 * y - 100 * d - 208 * e + 128) >> 8, "b": (298 * y + 516 * d + 128) >> 8}
    return {ch + "_lo" for ch, v in raw.items() if (v < 0).any()} | {ch + "_hi" for ch, v in raw.items() if (v > 255).any()}


# ---- plane builders -----------------------------------------------------------------------------------------------------------------
def _frozen(planes):
    planes = tuple(np.ascontiguousarray(c, dtype=np.int64) for c in planes)
    for c in planes:
        c.setflags(write=False)
    return planes


def random_planes(plan, seed):
    rng = np.random.default_rng(seed)
    return _frozen(rng.integers(0, 1 << q, s) for s, q in zip(sample_counts(plan), bits_of(plan)))


def index_planes(plan):
    """y = j mod 2^qy, cb = k mod 2^qb, cr = (k >> qb) mod 2^qr: neighbouring samples differ in Y and in Cb, and a chroma sample
    2^qb away differs in Cr, so a wrong sample index changes the pixel for certain (up to 2^(qb + qr) samples), not just probably."""
    (n, cs, _), (qy, qb, qr) = sample_counts(plan), bits_of(plan)
    j, k = np.arange(n, dtype=np.int64), np.arange(cs, dtype=np.int64)
    return _frozen((j % (1 << qy), k % (1 << qb), (k >> qb) % (1 << qr)))


def extreme_planes(plan):
    """Three sets of planes: all zero, all ones (every code 2^q - 1), and 0 / 2^q - 1 alternating per sample."""
    counts, bits = sample_counts(plan), bits_of(plan)
    return [_frozen(np.zeros(s, dtype=np.int64) for s in counts),
            _frozen(np.full(s, (1 << q) - 1, dtype=np.int64) for s, q in zip(counts, bits)),
            _frozen((np.arange(s, dtype=np.int64) & 1) * ((1 << q) - 1) for s, q in zip(counts, bits))]


def cube_shape(bits):
    return 256, 1 << (sum(bits) - 8)


def cube_planes(bits):
    """Every code triple exactly once, for a 4:4:4 factor-1 frame of 256 x 2^(qy + qb + qr - 8): position i holds y = i >> (qb + qr),
    cb = (i >> qr) mod 2^qb, cr = i mod 2^qr -- at (8, 8, 8) the order of test_exhaustive_cube_inverse."""
    qy, qb, qr = bits
    assert qy + qb + qr >= 8
    i = np.arange(1 << (qy + qb + qr), dtype=np.int64)
    return _frozen((i >> (qb + qr), (i >> qr) & ((1 << qb) - 1), i & ((1 << qr) - 1)))


def slice_layout(count):
    """The layout of `count` consecutive positions of a 4:4:4 factor-1 stream (chroma sample k = j) as ref_pixels reads it."""
    return types.SimpleNamespace(y_width=count, y_height=1, module_width=count, chroma_width=count, hold_h=1, hold_v=1, replay_last=0)
