"""The AVG sampling extension on the GPU -- k_avg (tile body and the edge blocks of avg_edge_output), k_avg_generic, k_planar_avg_f1,
k_planar_avg_tile, k_planar_avg_gen and k_pbits_gen<avg> (csrc/csic_kernel_ops.h, csic_avg_tile.h, csic_planar.hip,
csic_planar_bits.hip) -- on frames built to order (tests/avg_frames.py; its numpy statement, its levers, the coverage of the built sets
and the faults they notice are proved on the CPU in tests/test_avg_frames_host.py).  Expected values come from the oracle
(process(form="avg"), oracle.planar(avg=True), the bit packing of tests/test_gpu_planar_bits.py); the cube and the palette are also held
to the closed form, the oracle's second opinion.  Every comparison is exact.  Packed outputs start as 0xEE with a canary tail; planar
and bit-packed frames are compared as whole buffers, so the bytes the format does not own keep 0xEE.  Each run asserts the kernel
it means to run (_run), and test_every_avg_kernel_was_seen (which runs last) holds the names seen to the list of what the selector
can produce.

  test_cube_*        all 2^24 colours through fwd_c_pk: k_avg<f1,h1,v1>, k_planar_avg_f1<h1,v1>, k_planar_avg_tile (CSIC_TUNE_VARIANT 12).
  test_palette       the corners of the chroma arithmetic, magnified to whole regions and with the last regions cut: every sink, 24
                     instantiations, both roundings, 8 / 8 / 8 and 5 / 6 / 3 bits.
  test_windows       saturated sums and both sides of every rounding tie, per channel: every sink.
  test_residues      every (W mod 8, H mod max(f, v)) with random and loud edges, frame by frame and as a batch of three (edge blocks
                     under blockIdx.z > 0): packed, planar (default, variants 12 and 9) and bit-packed.
  test_below_the_tile_minimum   W = 3 (7 at factor 8): the plans fall to the one-pixel-per-lane kernels.
Run with `-m gpu` on an MI355X."""
import re

import numpy as np
import pytest

import avg_frames as af
from test_gpu_planar_bits import _expected_frame

pytestmark = pytest.mark.gpu

CSQ = (3, 1, 2)
CANARY32 = -286331154                    # 0xEEEEEEEE as int32
FILL = 0xEE
TAIL = 64
FMT_PLANAR, FMT_BITS = 2, 3
ROUNDINGS = (af.FLOOR, af.TRUNC)
RN = ("floor", "trunc")
MF_IDS = [f"{a}{b}-f{f}" for a, b, f in af.MODE_FACTORS]
MIXED = (5, 6, 3)
SEEN = set()                             # normalised names (_norm) of every kernel a run of this module asserted and launched

PACKED_SINKS = ("argb", "ycc", "ycc_cached", "ycc_generic", "argb_generic")
PLANE_SINKS = ("planar", "planar12", "planar9", "bits")
ALL_SINKS = PACKED_SINKS + PLANE_SINKS
RESIDUE_SINKS = ("argb", "ycc", "planar", "planar12", "planar9", "bits")


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    assert csic_amd._native.lib().csic_device_count() >= 1
    return csic_amd


@pytest.fixture(scope="module")
def pal():
    """The palette image; building it builds the lever tables from the colour cube, once for the module."""
    return af.palette()


def _plan(csic, W, H, a, b, bits, f, rounding, fmt):
    cp = csic.make_c_params(W, H, a, b, *bits, f, CSQ, rounding=rounding, out_format=fmt, sampling=csic.Sampling.AVG)
    return csic.Plan(cp, 0)


def _op(orc, W, H, a=4, b=4, bits=(8, 8, 8), f=1, rounding=0, fmt=0):
    return orc.OracleParams(width=W, height=H, chroma_a=a, chroma_b=b, y_bits=bits[0], cb_bits=bits[1], cr_bits=bits[2], factor=f, op=CSQ,
                            rounding=rounding, out_format=fmt)


def _norm(name):
    """A kernel name without its rounding and format: what the coverage list is written in."""
    stem, args = name.rstrip(">").split("<")
    args = args.split(",")
    if stem == "k_avg":
        return (stem,) + tuple(args[2:])                       # f, h, v, nt / cached
    if stem == "k_planar_avg_tile":
        return (stem,) + tuple(args[1:4])                      # f, h, v
    if stem == "k_planar_avg_f1":
        return (stem,) + tuple(args[1:3])                      # h, v
    if stem == "k_pbits_gen":
        return (stem, args[1])                                 # avg
    return (stem,)


def _expected_name(sink, W, H, a, b, f, rounding, small):
    """The kernel a sink means to run, as a regular expression on the plan's kernel name.  small: a frame without a whole tile."""
    h, v = af.HV[a, b]
    rn = RN[rounding]
    if sink in ("argb", "ycc", "ycc_cached") and not small:
        return rf"k_avg<{rn},{sink[:4].rstrip('_')},f{f},h{h},v{v},{'cached' if sink == 'ycc_cached' else 'nt'}>"
    if sink in PACKED_SINKS:
        return rf"k_avg_generic<{rn},{sink[:4].rstrip('_')}>"
    if sink == "bits":
        return rf"k_pbits_gen<{rn},avg,h\d,v\d>"
    if sink == "planar9" or small:
        return rf"k_planar_avg_gen<{rn},h\d,v\d>"
    if sink == "planar" and f == 1 and W % 4 == 0 and H % v == 0:
        return rf"k_planar_avg_f1<{rn},h{h},v{v},nt>"
    return rf"k_planar_avg_tile<{rn},f{f},h{h},v{v},nt>"


def _claim(pl, sink, W, H, a, b, f, rounding, small):
    want = _expected_name(sink, W, H, a, b, f, rounding, small)
    assert re.fullmatch(want, pl.kernel_name), (sink, pl.kernel_name, want)
    SEEN.add(_norm(pl.kernel_name))


def _same(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = tuple(int(x) for x in np.argwhere(got != want)[0])
        raise AssertionError(f"{tag}: at {at} expected {int(want[at]):#x}, got {int(got[at]):#x}; {int((got != want).sum())} of {want.size} differ")


def _packed_on_device(pl, d_in, n):
    """The plan's packed output of n frames in a buffer that starts as 0xEE and keeps a canary tail -> the flat int32 device tensor."""
    import torch
    count = n * pl.out_width * pl.out_height
    buf = torch.full((count + TAIL,), CANARY32, dtype=torch.int32, device="cuda:0")
    pl.process_device(d_in, buf[:count], nframes=n)
    assert bool((buf[count:] == CANARY32).all()), "the canary behind the output was overwritten"
    return buf[:count]


def _planes_on_device(pl, d_in, n):
    """The plan's planar / bit-packed frames of n frames, the buffer pre-filled with 0xEE, tail included."""
    import torch
    buf = torch.full((n * pl.frame_bytes + 4 * TAIL,), FILL, dtype=torch.uint8, device="cuda:0")
    pl.process_device(d_in, buf[:n * pl.frame_bytes], nframes=n)
    return buf


def _planar_frame(lay, y, cb, cr):
    """The whole CSIC_FMT_PLANAR frame buffer, 0xEE in every byte the format does not own."""
    want = np.full(lay.frame_bytes, FILL, dtype=np.uint8)
    want[lay.y_offset:lay.y_offset + y.size] = y.reshape(-1)
    want[lay.cb_offset:lay.cb_offset + cb.size] = cb
    want[lay.cr_offset:lay.cr_offset + cr.size] = cr
    return want


def _run(csic, oracle, frames, a, b, f, rounding, bits, sinks, tag, closed=None, small=False):
    """Every sink of `sinks` on the batch `frames` (same shape), each on the kernel it names, against the oracle; closed: per
    format (ARGB, YCbCr) what the closed form says the packed outputs are, held to as well."""
    import torch
    N = csic._native
    n = len(frames)
    H, W = frames[0].shape
    d_in = torch.from_numpy(np.stack(frames).view(np.int32)).cuda()
    args = (W, H, a, b, f, rounding, small)
    want = {fmt: np.stack([oracle.process(_op(oracle, W, H, a, b, bits, f, rounding, fmt), fr, form="avg") for fr in frames]) for fmt in (af.ARGB, af.YCC)}
    if closed is not None:
        for fmt in (af.ARGB, af.YCC):
            _same(want[fmt], closed[fmt], tag + ("the oracle against the closed form", fmt))
    for fmt, names in ((af.ARGB, ("argb", "argb_generic")), (af.YCC, ("ycc", "ycc_cached", "ycc_generic"))):
        mine = [s for s in names if s in sinks]
        if not mine:
            continue
        with _plan(csic, W, H, a, b, bits, f, rounding, fmt) as pl:
            for sink in mine:
                pl.tune(N.TUNE_NONTEMPORAL, 0 if sink == "ycc_cached" else 1)
                pl.tune(N.TUNE_FORCE_GENERIC, 1 if sink.endswith("generic") else 0)
                _claim(pl, sink, *args)
                got = _packed_on_device(pl, d_in, n).cpu().numpy().view(np.uint32).reshape(want[fmt].shape)
                _same(got, want[fmt], tag + (pl.kernel_name,))
    if not set(sinks) & set(PLANE_SINKS):
        return
    planes = [oracle.planar(_op(oracle, W, H, a, b, bits, f, rounding), fr, avg=True)[1:] for fr in frames]
    tail = np.full(4 * TAIL, FILL, dtype=np.uint8)
    if {"planar", "planar12", "planar9"} & set(sinks):
        with _plan(csic, W, H, a, b, bits, f, rounding, FMT_PLANAR) as pl:
            whole = np.concatenate([_planar_frame(pl.planar_layout, *p) for p in planes] + [tail])
            for sink, variant in (("planar", 0), ("planar12", 12), ("planar9", 9)):
                if sink in sinks:
                    pl.tune(N.TUNE_VARIANT, variant)
                    _claim(pl, sink, *args)
                    _same(_planes_on_device(pl, d_in, n).cpu().numpy(), whole, tag + (pl.kernel_name,))
    if "bits" in sinks:
        with _plan(csic, W, H, a, b, bits, f, rounding, FMT_BITS) as pl:
            whole = np.concatenate([_expected_frame(pl.planar_bits_layout, *p) for p in planes] + [tail])
            _claim(pl, "bits", *args)
            _same(_planes_on_device(pl, d_in, n).cpu().numpy(), whole, tag + (pl.kernel_name,))


# ---- the cube ----------------------------------------------------------------------------------------
CUBE_PACKED = [(0, af.YCC), (1, af.YCC), (1, af.ARGB)]


@pytest.fixture(scope="module")
def cube_refs(oracle):
    """The oracle on the cube at 4:4:4, factor 1, 8 / 8 / 8, computed once for the module and left unchanged: {(rounding, format,
    form)} for the packed outputs, {(rounding, "planar")} = (Y, Cb, Cr) of oracle.planar(avg=True)."""
    refs = {(rounding, fmt, form): oracle.process(_op(oracle, 4096, 4096, rounding=rounding, fmt=fmt), af.cube(), form=form)
            for rounding, fmt in CUBE_PACKED for form in ("avg", "closed")}
    for rounding in ROUNDINGS:
        refs[rounding, "planar"] = oracle.planar(_op(oracle, 4096, 4096, rounding=rounding), af.cube(), avg=True)[1:]
    for v in refs.values():
        for x in (v if isinstance(v, tuple) else (v,)):
            x.setflags(write=False)
    return refs


def _cube_in():
    import torch
    return torch.from_numpy(af.cube().view(np.int32).reshape(-1)).cuda()


def _device(a):
    import torch
    return torch.from_numpy(np.array(a).reshape(-1).view(np.int32)).cuda()          # (a copy: the cached references are read-only)


@pytest.mark.parametrize("rounding,fmt", CUBE_PACKED, ids=["floor-ycc", "trunc-ycc", "trunc-argb"])
def test_cube_through_k_avg(csic, cube_refs, rounding, fmt):
    """fwd_c_pk on all 2^24 colours: the clamp (pure blue, pure red), every quotient of 255, both sides of the TRUNC threshold."""
    import torch
    want = cube_refs[rounding, fmt, "avg"]
    assert np.array_equal(want, cube_refs[rounding, fmt, "closed"])
    with _plan(csic, 4096, 4096, 4, 4, (8, 8, 8), 1, rounding, fmt) as pl:
        _claim(pl, "ycc" if fmt == af.YCC else "argb", 4096, 4096, 4, 4, 1, rounding, False)
        got = _packed_on_device(pl, _cube_in(), 1)
        assert torch.equal(got, _device(want)), pl.kernel_name


@pytest.mark.parametrize("rounding", ROUNDINGS, ids=RN)
@pytest.mark.parametrize("sink,variant", [("planar", 0), ("planar12", 12)])
def test_cube_through_the_planar_kernels(csic, cube_refs, rounding, sink, variant):
    """k_planar_avg_f1<h1,v1> and k_planar_avg_tile<f1,h1,v1> (CSIC_TUNE_VARIANT 12): the planes are the bytes of the packed YCbCr
    output, which is the closed form."""
    import torch
    y, cb, cr = cube_refs[rounding, "planar"]
    closed = cube_refs[rounding, af.YCC, "closed"]
    assert np.array_equal(y, closed & 255) and np.array_equal(cb, ((closed >> 8) & 255).reshape(-1)) and np.array_equal(cr, ((closed >> 16) & 255).reshape(-1))
    with _plan(csic, 4096, 4096, 4, 4, (8, 8, 8), 1, rounding, FMT_PLANAR) as pl:
        pl.tune(csic._native.TUNE_VARIANT, variant)
        _claim(pl, sink, 4096, 4096, 4, 4, 1, rounding, False)
        want = np.concatenate([_planar_frame(pl.planar_layout, y, cb, cr), np.full(4 * TAIL, FILL, dtype=np.uint8)])
        got = _planes_on_device(pl, _cube_in(), 1)
        assert torch.equal(got, torch.from_numpy(want).cuda()), pl.kernel_name


# ---- the palette -------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounding", ROUNDINGS, ids=RN)
@pytest.mark.parametrize("a,b,f", af.MODE_FACTORS, ids=MF_IDS)
def test_palette(csic, oracle, pal, a, b, f, rounding):
    """Both magnified forms through every sink; the oracle's outputs are themselves held to the closed form of the palette image."""
    h, v = af.HV[a, b]
    for bits in ((8, 8, 8), MIXED):
        base = {fmt: oracle.process(_op(oracle, pal.shape[1], pal.shape[0], bits=bits, rounding=rounding, fmt=fmt), pal, form="closed") for fmt in (af.ARGB, af.YCC)}
        for cut, frame in enumerate((af.magnified(pal, f, h, v), af.magnified_cut(pal, f, h, v))):
            closed = {fmt: af.magnified_expectation(base[fmt], f, h, v, bool(cut))[None] for fmt in base}
            _run(csic, oracle, [frame], a, b, f, rounding, bits, ALL_SINKS, ("palette", a, b, f, rounding, bits, "cut" if cut else "whole"), closed)


# ---- the windows -------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b,f", af.MODE_FACTORS, ids=MF_IDS)
def test_windows(csic, oracle, pal, a, b, f):
    """The mosaic of recipe windows (192 pixels wide: k_avg takes two tiles per lane at factors 1 and 2) through every sink."""
    for rounding in ROUNDINGS:
        frame, _ = af.windows_frame(a, b, f, rounding)
        for bits in ((8, 8, 8), MIXED):
            _run(csic, oracle, [frame], a, b, f, rounding, bits, ALL_SINKS, ("windows", a, b, f, rounding, bits))


# ---- the residues ------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(4), ids=["w16-17", "w18-19", "w20-21", "w22-23"])
@pytest.mark.parametrize("rounding", ROUNDINGS, ids=RN)
@pytest.mark.parametrize("a,b,f", af.MODE_FACTORS, ids=MF_IDS)
def test_residues(csic, oracle, a, b, f, rounding, part):
    """Every (W mod 8, H mod max(f, v)), every content: frame by frame through the packed kernels, the planar kernels and the bit
    packer, and the three contents as one batch (the edge blocks of frames 1 and 2 run under blockIdx.z > 0).  One id holds half of the
    widths."""
    assert part in range(4)
    shapes = [(W, H) for W, H in af.residue_shapes(a, b, f) if (W - 16) // 2 == part]
    assert len(shapes) == 2 * max(f, af.HV[a, b][1])
    for W, H in shapes:
        frames = [af.residue_frame(W, H, content) for content in af.RESIDUE_CONTENTS]
        for content, frame in zip(af.RESIDUE_CONTENTS, frames):
            _run(csic, oracle, [frame], a, b, f, rounding, (8, 8, 8), RESIDUE_SINKS, ("residues", a, b, f, rounding, W, H, content))
        _run(csic, oracle, frames, a, b, f, rounding, (8, 8, 8), RESIDUE_SINKS, ("residues", a, b, f, rounding, W, H, "batch"))


@pytest.mark.parametrize("a,b,f", af.MODE_FACTORS, ids=MF_IDS)
def test_below_the_tile_minimum(csic, oracle, a, b, f):
    """W = 3 (7 at factor 8): no whole tile, the plans fall to k_avg_generic / k_planar_avg_gen and are still exact."""
    W, H = af.small_shape(f)
    for rounding in ROUNDINGS:
        frames = [af.residue_frame(W, H, content) for content in af.RESIDUE_CONTENTS]
        _run(csic, oracle, frames, a, b, f, rounding, MIXED, ("argb", "ycc", "planar", "bits"), ("small", a, b, f, rounding, W, H), small=True)


# ---- coverage ------------------------------------------------------------------------------------------
def test_every_avg_kernel_was_seen(csic):
    """Across the module (this test runs last): every AVG kernel name the selector can produce -- k_avg at the 24 (f, h, v) with
    non-temporal and with cached accesses, k_avg_generic, k_planar_avg_f1 at its six (h, v), k_planar_avg_tile at the 24,
    k_planar_avg_gen, k_pbits_gen<avg>."""
    fhv = [(f"f{f}", f"h{h}", f"v{v}") for f in af.FACTORS for h, v in af.HV.values()]
    want = {("k_avg",) + x + (nt,) for x in fhv for nt in ("nt", "cached")} | {("k_planar_avg_tile",) + x for x in fhv}
    want |= {("k_planar_avg_f1", f"h{h}", f"v{v}") for h, v in af.HV.values()}
    want |= {("k_avg_generic",), ("k_planar_avg_gen",), ("k_pbits_gen", "avg")}
    assert len(want) == 48 + 24 + 6 + 3
    assert want <= SEEN, sorted(want - SEEN)
    assert SEEN <= want, sorted(SEEN - want)                   # and nothing this module does not know of
