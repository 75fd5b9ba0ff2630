"""The readers of the planar formats -- k_recon, k_rbits, k_decode, k_decode_gen and the three k_cstat_* kernels, which share
csrc/csic_plane_read.h and one checked-access layer -- on frames built to order (tests/plane_frames.py; its builders and its numpy
reference are proved on the CPU in tests/test_plane_frames_host.py).  The frame is built on the host and uploaded, so what a reader
meets is not left to the forward path: any code triple, any byte behind a plane, any bit below the quantiser.  One check serves every
test (_read_all / _expected): a frame in PLANAR and in BITS through reconstruct (default kernels, CSIC_TUNE_VARIANT 9, non-temporal
accesses off), decode (default and variant 9) and code statistics (fast and CSIC_TUNE_FORCE_GENERIC); pixels against ref_pixels in
both output formats and, for ARGB, against oracle.planar_reconstruct; counts against plane_hists on the codes; every output buffer with
a canary behind it.  Every comparison is exact.  Where to find the case for each edge:

  test_built_planes           every shape of plane_frames.SHAPES (and AVG on AVG_SHAPES) x 4:4:4 / 4:2:2 / 4:2:0 / 4:1:1 x one order of each
                              class x six bit triples x random, index, all-zero, all-ones and alternating planes, random fill.
  test_fill_independence      random planes under the three fills: the same output from every reader; PLANAR with the bits below the
                              quantiser set: the same counts, and pixels of the RAW bytes.
  test_batches                three different frames with three different fills in one call, frame k against its own reference.
  test_quantised_cubes        every code triple of (6, 5, 5), (3, 3, 2), (5, 6, 5), (8, 4, 4) once, through every reader and expanded by
                              the fast k_decode at factors 2, 4, 8.
  test_the_whole_cube         all 2^24 (Y, Cb, Cr) through k_recon, k_rbits and k_decode_gen: the inverse transform on the whole cube.
  test_bit_offsets_past_2_32  4096 x 131073 at 8 / 8 / 8: every plane crosses bit 2^32.
Run with `-m gpu` on an MI355X."""
import hashlib

import numpy as np
import pytest

from plane_frames import (ARGB, AVG_SHAPES, BITS, INVERSE_CUBE_DIGEST, CHROMA, CSQ, PLANAR, SHAPES, TRIPLES, YCC, bits_of, combos, cube_planes, cube_shape,
                          extreme_planes, frame_of, index_planes, random_planes, ref_decode, ref_pixels, regions, sample_counts, slice_layout,
                          values_of)
from test_code_stats_host import plane_hists

pytestmark = pytest.mark.gpu

CANARY = -286331154                      # 0xEEEEEEEE as int32
SEEN = set()                             # the stems of every decode kernel the module ran


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    assert csic_amd._native.lib().csic_device_count() >= 1
    return csic_amd


def _plan(csic, W, H, a=4, b=4, bits=(8, 8, 8), f=1, op=CSQ, avg=False):
    cp = csic.make_c_params(W, H, a, b, *bits, f, op, sampling=csic.Sampling.AVG if avg else csic.Sampling.HOLD_DECIMATE)
    return csic.Plan(cp, 0)


def _oracle_layout(oracle, pl, avg=False):
    c = pl.c_params
    return oracle.planar_layout(oracle.OracleParams(width=c.width, height=c.height, chroma_a=c.chroma_a, chroma_b=c.chroma_b, y_bits=c.y_bits,
                                                    cb_bits=c.cb_bits, cr_bits=c.cr_bits, factor=c.factor, op=tuple(c.op)), avg)


def _upload(frames):
    import torch
    return torch.from_numpy(np.ascontiguousarray(frames)).cuda()


def _canaried(call, count):
    """call(d_out) on `count` pixels of a buffer with a canary tail -> the pixels, uint32 on the host."""
    import torch
    buf = torch.full((count + 64,), CANARY, dtype=torch.int32, device="cuda:0")
    call(buf[:count])
    host = buf.cpu().numpy()
    assert (host[count:] == CANARY).all(), "the canary behind the output was overwritten"
    return host[:count].view(np.uint32)


def _canaried_on_device(call, count):
    """As _canaried for the large frames: the pixels stay on the device (a flat int32 tensor), only the tail comes to the host."""
    import torch
    buf = torch.full((count + 64,), CANARY, dtype=torch.int32, device="cuda:0")
    call(buf[:count])
    assert bool((buf[count:] == CANARY).all()), "the canary behind the output was overwritten"
    return buf[:count]


def _read_all(csic, pl, src, nf=1, fmts=(PLANAR, BITS)):
    """Every reader on the device frames src[fmt] (nf frames each) -> {key: host array}."""
    N = csic._native
    W, H, Wo, Ho = pl.width, pl.height, pl.out_width, pl.out_height
    out = {}
    for fmt in fmts:
        recon = pl.reconstruct_device if fmt == PLANAR else pl.reconstruct_bits_device
        for knob, value, rest in ((N.TUNE_VARIANT, 0, 0), (N.TUNE_VARIANT, 9, 0), (N.TUNE_NONTEMPORAL, 0, 1)):
            pl.tune(knob, value)
            for o in (ARGB, YCC):
                out["reconstruct", fmt, knob, value, o] = _canaried(lambda d: recon(src[fmt], d, nf, o), nf * Wo * Ho).reshape(nf, Ho, Wo)
            pl.tune(knob, rest)
        for variant in (0, 9):
            pl.tune(N.TUNE_VARIANT, variant)
            for o in (ARGB, YCC):
                SEEN.add(pl.decode_kernel_name(fmt, o).split("<")[0])
                out["decode", fmt, variant, o] = _canaried(lambda d: pl.decode_device(src[fmt], fmt, d, nf, o), nf * W * H).reshape(nf, H, W)
        pl.tune(N.TUNE_VARIANT, 0)
        for force in (0, 1):
            pl.tune(N.TUNE_FORCE_GENERIC, force)
            assert pl.code_stats_kernel_name(fmt).startswith("k_cstat_gen") == bool(force)
            out["code stats", fmt, force] = pl.code_stats_device(src[fmt], fmt, nf).cpu().numpy().view(np.uint64)
        pl.tune(N.TUNE_FORCE_GENERIC, 0)
    return out


def _hists(planes, bits):
    return np.stack([np.stack(x) for x in zip(*[plane_hists(c, q) for c, q in zip(planes, bits)])])


def _expected(oracle, pl, olay, keys, values, codes):
    """What _read_all must give under `keys`: values[fmt] = per frame the three planes of 8-bit values that the frame of that format
    holds, codes = per frame the three planes of codes."""
    lay, f = pl.planar_layout, pl.c_params.factor
    px = {}
    for fmt, frames in values.items():
        for o in (ARGB, YCC):
            px[fmt, o] = np.stack([ref_pixels(lay, *v, o) for v in frames])
        assert all(np.array_equal(p, oracle.planar_reconstruct(olay, *v, oracle.FMT_ARGB)) for p, v in zip(px[fmt, ARGB], frames))
    hist = np.stack([_hists(c, bits_of(pl)) for c in codes])
    want = {}
    for key in keys:
        if key[0] == "reconstruct":
            want[key] = px[key[1], key[-1]]
        elif key[0] == "decode":
            want[key] = np.stack([ref_decode(p, pl.width, pl.height, f) for p in px[key[1], key[-1]]])
        else:
            want[key] = hist
    return want


def _check(csic, oracle, pl, olay, frames_of_codes, fills, tag, low_bits=None, fmts=(PLANAR, BITS)):
    """frames_of_codes: per frame three planes of codes; fills: per frame its fill.  Builds the frames of each format, runs every
    reader over them as one batch and holds each frame against its own reference.  Returns what the readers gave."""
    bits = bits_of(pl)
    host = {fmt: np.stack([frame_of(pl, fmt, *c, fill=fill, low_bits=low_bits) for c, fill in zip(frames_of_codes, fills)]) for fmt in fmts}
    values = {fmt: [values_of(c, bits) if fmt == BITS or low_bits is None else pl.split_planar(fr) for c, fr in zip(frames_of_codes, host[fmt])]
              for fmt in fmts}
    got = _read_all(csic, pl, {fmt: _upload(h) for fmt, h in host.items()}, len(frames_of_codes), fmts)
    want = _expected(oracle, pl, olay, got.keys(), values, frames_of_codes)
    for key, g in got.items():
        assert np.array_equal(g, want[key]), (key, tag)
    return got


def _cases(W, H, f, avg):
    for a, b, op in ([(a, b, CSQ) for a, b in CHROMA] if avg else combos(W, H, f)):
        for bits in TRIPLES:
            yield a, b, op, bits


_SHAPE_CASES = [(W, H, f, False) for W, H, f in SHAPES] + [(W, H, f, True) for W, H, f in AVG_SHAPES]
_SHAPE_IDS = [f"{W}x{H}-f{f}" + ("-avg" if avg else "") for W, H, f, avg in _SHAPE_CASES]


# ---- a. built planes, every reader ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,f,avg", _SHAPE_CASES, ids=_SHAPE_IDS)
def test_built_planes(csic, oracle, W, H, f, avg):
    rng = np.random.default_rng(5100 + W + f)
    for a, b, op, bits in _cases(W, H, f, avg):
        with _plan(csic, W, H, a, b, bits, f, op, avg) as pl:
            olay = _oracle_layout(oracle, pl, avg)
            for name, planes in [("random", random_planes(pl, int(rng.integers(1 << 30)))), ("index", index_planes(pl))] + \
                    list(zip(("zeros", "ones", "alternating"), extreme_planes(pl))):
                _check(csic, oracle, pl, olay, [planes], [rng], (W, H, f, avg, a, b, op, bits, name))


# ---- b. fill independence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,f,avg", _SHAPE_CASES, ids=_SHAPE_IDS)
def test_fill_independence(csic, oracle, W, H, f, avg):
    """The padding after each plane, the tail behind a partial last chroma row and the high bits of a bit plane's last byte under
    0x00, 0xFF and random bytes: every reader gives the same pixels and the same counts.  A PLANAR byte with bits below the quantiser
    set counts as its code, and reconstructs and decodes as the byte it is."""
    rng = np.random.default_rng(5200 + W + f)
    for a, b, op, bits in _cases(W, H, f, avg):
        with _plan(csic, W, H, a, b, bits, f, op, avg) as pl:
            olay = _oracle_layout(oracle, pl, avg)
            planes = random_planes(pl, int(rng.integers(1 << 30)))
            tag = (W, H, f, avg, a, b, op, bits)
            runs = [_check(csic, oracle, pl, olay, [planes], [fill], tag + (str(fill),)) for fill in (0x00, 0xFF, rng)]
            for other in runs[1:]:
                assert runs[0].keys() == other.keys() and all(np.array_equal(runs[0][k], other[k]) for k in other), tag
            for low in ("ones", rng):
                got = _check(csic, oracle, pl, olay, [planes], [rng], tag + ("low bits", str(low)), low_bits=low, fmts=(PLANAR,))
                for force in (0, 1):
                    assert np.array_equal(got["code stats", PLANAR, force], runs[0]["code stats", PLANAR, force]), tag


# ---- c. batches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,f", [(200, 26, 1), (64, 40, 2)])
def test_batches(csic, oracle, W, H, f):
    rng = np.random.default_rng(5300 + W)
    for a, b, op in combos(W, H, f):
        for bits in ((8, 8, 8), (7, 6, 5), (5, 3, 7)):
            with _plan(csic, W, H, a, b, bits, f, op) as pl:
                frames = [random_planes(pl, 1), index_planes(pl), random_planes(pl, 2)]
                assert not np.array_equal(frames[0][0], frames[2][0])
                _check(csic, oracle, pl, _oracle_layout(oracle, pl), frames, [0x00, 0xFF, rng], (W, H, f, a, b, op, bits))


# ---- d. quantised cubes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [(6, 5, 5), (3, 3, 2), (5, 6, 5), (8, 4, 4)])
def test_quantised_cubes(csic, oracle, bits):
    """Every code triple of the quantiser once, at 4:4:4 and factor 1, through every reader; then the same planes under plans of
    factor 2, 4 and 8 whose OUTPUT dimensions are the cube's, where the fast k_decode expands every triple."""
    rng = np.random.default_rng(5400 + sum(bits))
    W, H = cube_shape(bits)
    planes = cube_planes(bits)
    with _plan(csic, W, H, 4, 4, bits) as pl:
        _check(csic, oracle, pl, _oracle_layout(oracle, pl), [planes], [rng], ("cube", bits))
        src = {fmt: _upload(frame_of(pl, fmt, *planes, fill=rng)) for fmt in (PLANAR, BITS)}
        px = {o: ref_pixels(pl.planar_layout, *values_of(planes, bits), o) for o in (ARGB, YCC)}
    for f in (2, 4, 8):
        with _plan(csic, W * f, H * f, 4, 4, bits, f) as big:
            assert sample_counts(big) == (W * H,) * 3 and all(regions(big, fmt)[2][3] == src[fmt].numel() for fmt in src)
            for fmt in (PLANAR, BITS):
                for o in (ARGB, YCC):
                    assert big.decode_kernel_name(fmt, o).startswith("k_decode<"), big.decode_kernel_name(fmt, o)
                    got = _canaried(lambda d: big.decode_device(src[fmt], fmt, d, 1, o), W * f * H * f).reshape(H * f, W * f)
                    assert np.array_equal(got, ref_decode(px[o], W * f, H * f, f)), (bits, f, fmt, o)


# ---- e. the whole cube --------------------------------------------------------------------------------------------------------------
def test_the_whole_cube(csic, oracle):
    """All 2^24 (Y, Cb, Cr) as one 4096 x 4096 frame at 4:4:4, 8 / 8 / 8 -- the PLANAR and the BITS frame are the same bytes -- through
    k_recon and k_rbits to ARGB and YCC and through k_decode_gen to ARGB.  This is the check on the whole cube that the comment on
    finish_y (csic_kernel_ops.h) speaks of: the forward transform reaches under a quarter of these triples."""
    import torch
    N = csic._native
    bits = (8, 8, 8)
    planes = cube_planes(bits)
    with _plan(csic, 4096, 4096) as pl:
        lay = pl.planar_layout
        assert regions(pl, PLANAR) == regions(pl, BITS) and lay.frame_bytes == 3 << 24
        want = {o: ref_pixels(lay, *planes, o) for o in (ARGB, YCC)}
        rgb = want[ARGB].reshape(-1, 1).view(np.uint8)[:, 2::-1]                     # bytes B, G, R, A -> R, G, B
        assert hashlib.sha256(np.ascontiguousarray(rgb).tobytes()).hexdigest() == INVERSE_CUBE_DIGEST
        d_want = {o: _upload(w.view(np.int32).reshape(-1)) for o, w in want.items()}
        src = _upload(frame_of(pl, PLANAR, *planes, fill=0xFF))
        for o in (ARGB, YCC):
            assert pl.decode_kernel_name(PLANAR, o).startswith("k_recon<") and pl.decode_kernel_name(BITS, o).startswith("k_rbits<")
            assert torch.equal(_canaried_on_device(lambda d: pl.reconstruct_device(src, d, 1, o), 1 << 24), d_want[o]), ("k_recon", o)
            assert torch.equal(_canaried_on_device(lambda d: pl.reconstruct_bits_device(src, d, 1, o), 1 << 24), d_want[o]), ("k_rbits", o)
        pl.tune(N.TUNE_VARIANT, 9)
        for fmt in (PLANAR, BITS):
            assert pl.decode_kernel_name(fmt, ARGB).startswith("k_decode_gen<")
            assert torch.equal(_canaried_on_device(lambda d: pl.decode_device(src, fmt, d), 1 << 24), d_want[ARGB]), ("k_decode_gen", fmt)


# ---- f. bit offsets past 2^32 -------------------------------------------------------------------------------------------------------
def test_bit_offsets_past_2_32(csic, oracle):
    """4096 x 131073 at 4:4:4, factor 1, 8 / 8 / 8: 2^29 + 4096 positions, so the bit offset of a sample passes 2^32 in all three
    planes (BitPlanes::y_word multiplies in 64 bits and computes chroma indices in 64 bits on purpose).  The planes are random bytes
    made on the device -- n is a multiple of 256, so the three planes are the whole frame and there is nothing to fill -- and the
    expected stream Y | Cb << 8 | Cr << 16 and the counts are computed there too; the last 8192 positions and the 8192 around position
    2^29 are held against ref_pixels in ARGB on the host."""
    import torch
    W, H = 4096, 131073
    n = W * H
    assert n == (1 << 29) + 4096 and 8 * n > 1 << 32
    with _plan(csic, W, H) as pl:
        assert regions(pl, PLANAR) == regions(pl, BITS) == [(0, n, n, n, 0), (n, n, n, 2 * n, 0), (2 * n, n, n, 3 * n, 0)]
        g = torch.Generator(device="cuda:0")
        g.manual_seed(5600)
        src = torch.randint(0, 256, (3 * n,), dtype=torch.uint8, device="cuda:0", generator=g)
        y, cb, cr = src[:n], src[n:2 * n], src[2 * n:]
        want = cr.to(torch.int32)
        want <<= 8
        want |= cb
        want <<= 8
        want |= y
        for name, recon in (("k_rbits", pl.reconstruct_bits_device), ("k_recon", pl.reconstruct_device)):
            got = _canaried_on_device(lambda d: recon(src, d, 1, YCC), n)
            assert torch.equal(got, want), name
            del got
        del want
        spans = [(n - 8192, n), ((1 << 29) - 4096, (1 << 29) + 4096)]
        host = [[p[lo:hi].cpu().numpy() for p in (y, cb, cr)] for lo, hi in spans]
        for name, recon in (("k_rbits", pl.reconstruct_bits_device), ("k_recon", pl.reconstruct_device)):
            got = _canaried_on_device(lambda d: recon(src, d), n)
            for (lo, hi), planes in zip(spans, host):
                assert np.array_equal(got[lo:hi].cpu().numpy().view(np.uint32), ref_pixels(slice_layout(hi - lo), *planes, ARGB).reshape(-1)), (name, lo)
            del got
        want = torch.zeros((2, 3, 256), dtype=torch.int64, device="cuda:0")
        step = 1 << 26
        for p, c in enumerate((y, cb, cr)):
            for lo in range(0, n, step):
                part = c[lo:lo + step]
                want[0, p] += torch.bincount(part.to(torch.int32), minlength=256)
                prev = part[:1] * 0 if lo == 0 else c[lo - 1:lo]                    # e_0 = c_0; uint8 differences wrap mod 2^8
                want[1, p] += torch.bincount((part - torch.cat([prev, part[:-1]])).to(torch.int32), minlength=256)
        assert int(want.sum()) == 6 * n
        for fmt in (PLANAR, BITS):
            assert torch.equal(pl.code_stats_device(src, fmt)[0], want), fmt


def test_every_reader_family_was_seen(csic):
    """Across the module (this test runs last): the reconstruct kernels at factor 1, the fast decode, the general one."""
    assert {"k_recon", "k_rbits", "k_decode", "k_decode_gen"} <= SEEN, SEEN
