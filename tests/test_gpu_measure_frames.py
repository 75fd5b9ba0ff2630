"""The measurement units -- k_dist_fast, k_dist_gen, k_ssim_fast, k_ssim_gen and k_sum_partials (csrc/csic_distortion.hip,
csrc/csic_ssim.hip, csrc/csic_measure.h) -- on frames built to order (tests/measure_frames.py; its levers, its q table and the
coverage of the built set are proved on the CPU in tests/test_measure_frames_host.py).  The units are fused, so a test steers the
(reference, output) pairs of their arithmetic only through the input frame: gray pixels dictate Y, YCbCr input dictates three planes,
a four-colour palette drives the chroma of the ARGB-only kernels.  Every sum and the whole SSIM map are compared EXACTLY with
sse_numpy / ssim_numpy on the oracle's outputs (measure_frames.reference); there are no tolerances.  Every call goes through
_ssim / _dist: the C entry points on sums, map and workspace pre-filled with 0xEE and followed by a tail that must keep its fill.

  test_built_mosaics          every kernel class (measure_frames.classes: fast<f1> / fast<f2> at h in {1, 2, 4} x v in {1, 2} x both
                              roundings, gen<hold> in both order classes at factors 2, 4, 8, gen<hold,ycc-in>, gen<avg>,
                              gen<avg,ycc-in>) x lever set x window layout (8 x 8, 248 x 8, 256 x 8, 264 x 8, 8 x 264, 40 x 104), every
                              recipe rotated through every window as the frames of one batch; both units; 16-byte loads and a d_in
                              offset by 4 bytes; the fast classes again under CSIC_TUNE_FORCE_GENERIC.  One case per class, lever
                              set and half of the layouts.
  test_distortion_shapes_of_the_general_kernel / _of_the_fast_kernel
                              128 x 128 and 136 x 120 at factor 8 (a full block of lanes at the maximal lane sum, 255 outputs), 13 x 11
                              at factors 2 and 8 (clamped edge blocks), 136 x 62 for the fast classes; SSIM on their cut windows too.
  test_batches                three frames with different recipes in the same windows: the batch, single calls, the reference.
  test_replay_pair            one pixel, the last chroma sample of the row above, decides a whole odd row of 4:2:0 / 4:4:0 / 4:1:0.
  test_fill_independence      the same numbers whatever the buffers held before.
Run with `-m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import measure_frames as mf

pytestmark = pytest.mark.gpu

FILL64 = int.from_bytes(b"\xEE" * 8, "little", signed=True)
FILL32 = int.from_bytes(b"\xEE" * 4, "little", signed=True)
TAIL = 16


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    assert csic_amd._native.lib().csic_device_count() >= 1
    return csic_amd


def _plan(csic, W, H, c):
    cp = csic.make_c_params(W, H, c["a"], c["b"], *c["bits"], c["f"], c["op"], rounding=c["rounding"], sampling=1 if c["avg"] else 0,
                            in_format=c["in_format"])
    return csic.Plan(cp, 0)


def _upload(frames, offset=False):
    """The frames on the device; offset: at an address that is 4 bytes past a 16-byte boundary."""
    import torch
    flat = torch.from_numpy(np.array(frames, dtype=np.uint32).reshape(-1).view(np.int32))
    if not offset:
        return flat.cuda()
    buf = torch.zeros(flat.numel() + 4, dtype=torch.int32, device="cuda")
    buf[1:1 + flat.numel()] = flat.cuda()
    d = buf[1:1 + flat.numel()]
    assert d.data_ptr() % 16 == 4
    return d


def _filled(count, dtype, fill):
    import torch
    return torch.full((count + TAIL,), fill, dtype=dtype, device="cuda")


def _tail_kept(buf, count, fill, what):
    assert bool((buf[count:] == fill).all()), f"the bytes behind {what} were overwritten"


def _ssim(csic, pl, d_in, n, fill=(FILL64, FILL32)):
    """csic_ssim_device with the map -> (sums (n, 6) int64, map (n, 6, wy, wx) int32) on the host."""
    import torch
    N = csic._native
    wy, wx = pl.ssim_windows
    need = pl.ssim_workspace_bytes(n)
    assert need % 8 == 0
    ws, sums, dmap = _filled(need // 8, torch.int64, fill[0]), _filled(n * 6, torch.int64, fill[0]), _filled(n * 6 * wy * wx, torch.int32, fill[1])
    N.check(N.lib().csic_ssim_device(pl._h, C.c_void_p(d_in.data_ptr()), n, C.c_void_p(sums.data_ptr()), C.c_void_p(dmap.data_ptr()),
                                     C.c_void_p(ws.data_ptr()), need, pl._stream()))
    torch.cuda.synchronize()
    _tail_kept(ws, need // 8, fill[0], "the SSIM workspace")
    _tail_kept(sums, n * 6, fill[0], "the SSIM sums")
    _tail_kept(dmap, n * 6 * wy * wx, fill[1], "the SSIM map")
    return sums[:n * 6].cpu().numpy().reshape(n, 6), dmap[:n * 6 * wy * wx].cpu().numpy().reshape(n, 6, wy, wx)


def _dist(csic, pl, d_in, n, fill=FILL64):
    """csic_distortion_device -> sums (n, 6) uint64 on the host."""
    import torch
    N = csic._native
    need = pl.distortion_workspace_bytes(n)
    assert need % 8 == 0
    ws, sse = _filled(need // 8, torch.int64, fill), _filled(n * 6, torch.int64, fill)
    N.check(N.lib().csic_distortion_device(pl._h, C.c_void_p(d_in.data_ptr()), n, C.c_void_p(sse.data_ptr()), C.c_void_p(ws.data_ptr()),
                                           need, pl._stream()))
    torch.cuda.synchronize()
    _tail_kept(ws, need // 8, fill, "the distortion workspace")
    _tail_kept(sse, n * 6, fill, "the distortion sums")
    return sse[:n * 6].cpu().numpy().reshape(n, 6).astype(np.uint64)


CHANNELS = ("R", "G", "B", "Y", "Cb", "Cr")


def _hold(got, want, what, where=None):
    """Exact equality; a difference is reported with its frame, channel and window, what the reference says and what the GPU gave."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    at = tuple(int(v) for v in np.argwhere(got != want)[0])
    names = ""
    if where is not None and len(at) == 4:
        wi = at[2] * want.shape[3] + at[3]
        names = [w[wi] if w is not None else None for w in where[at[0]]]
    raise AssertionError(f"{what}: frame {at[0]}, channel {CHANNELS[at[1]]}, at {at[2:]}, recipes (Y, Cb, Cr) {names}: "
                         f"expected {int(want[at])}, got {int(got[at])}; {int((got != want).sum())} of {want.size} differ")


def _check(csic, pl, frames, ref, what, offset=False, where=None):
    """Both units on a batch against ref = (sse, sums, map); sums or map None: a frame without a whole window, distortion only."""
    n = len(frames)
    d_in = _upload(frames, offset)
    _hold(_dist(csic, pl, d_in, n), ref[0], what + ("distortion sums",))
    if ref[1] is not None:
        sums, qmap = _ssim(csic, pl, d_in, n)
        _hold(qmap, ref[2], what + ("SSIM map",), where)
        _hold(sums, ref[1], what + ("SSIM sums",))


def _names(pl):
    return pl.distortion_kernel_name, pl.ssim_kernel_name


def _check_every_path(csic, pl, c, frames, ref, what, where=None, ssim_class=None):
    """A class's plan on its selected kernels (asserted), with 16-byte loads and with a d_in offset by 4 bytes, and the fast
    classes again under CSIC_TUNE_FORCE_GENERIC: the same numbers."""
    N = csic._native
    if c["force"]:
        pl.tune(N.TUNE_FORCE_GENERIC, 1)
    ssim_class = c["cls"] if ssim_class is None else ssim_class
    assert _names(pl) == ("k_dist_" + c["cls"], "k_ssim_" + ssim_class), what
    _check(csic, pl, frames, ref, what + _names(pl), where=where)
    _check(csic, pl, frames, ref, what + _names(pl) + ("d_in + 4",), offset=True, where=where)
    if c["cls"].startswith("fast"):
        pl.tune(N.TUNE_FORCE_GENERIC, 1)
        assert _names(pl) == ("k_dist_gen<hold>", "k_ssim_gen<hold>")
        _check(csic, pl, frames, ref, what + _names(pl), where=where)
        _check(csic, pl, frames, ref, what + _names(pl) + ("d_in + 4",), offset=True, where=where)
        pl.tune(N.TUNE_FORCE_GENERIC, 0)


# ---- every class x lever set x layout, every recipe through every window ------------------------------
LAYOUT_PARTS = {"rows": mf.LAYOUTS[:4], "grids": mf.LAYOUTS[4:]}             # 97 and 98 windows: two cases of equal cost
MOSAIC_SETS = [(c, lever, q, part) for c in mf.classes() for lever, q, _ in mf.levers_of(c) for part in LAYOUT_PARTS]


@pytest.mark.parametrize("c,lever,q,part", MOSAIC_SETS, ids=[f"{mf.class_id(c)}-{lever}{q}-{part}" for c, lever, q, part in MOSAIC_SETS])
def test_built_mosaics(csic, oracle, c, lever, q, part):
    mine = [case for case in mf.cases([c]) if (case["lever"], case["bits"][0]) == (lever, q) and (case["W"], case["H"]) in LAYOUT_PARTS[part]]
    assert [(case["W"], case["H"]) for case in mine] == list(LAYOUT_PARTS[part])
    for case in mine:
        ref = mf.reference(oracle, case)
        with _plan(csic, case["W"], case["H"], case) as pl:
            what = (mf.class_id(c), lever, case["bits"], case["W"], case["H"])
            _check_every_path(csic, pl, case, ref["frames"], (ref["sse"], ref["sums"], ref["map"]), what, ref["where"])


def test_every_case_of_the_built_set_is_run():
    assert sum(len(LAYOUT_PARTS[part]) for _, _, _, part in MOSAIC_SETS) == len(mf.cases())
    assert sum(LAYOUT_PARTS.values(), ()) == mf.LAYOUTS


# ---- shapes of the distortion kernels ------------------------------------------------------------------
def _shape_reference(oracle, c, lever, names, W, H, count):
    frames, _ = mf.build_frames(lever, names, c["f"], W, H)
    frames = frames[:count]
    m = [mf.measure(oracle, fr, W, H, c) for fr in frames]
    sse = np.array([x[0] for x in m], dtype=np.uint64)
    if m[0][1] is None:
        return frames, (sse, None, None)
    return frames, (sse, np.array([x[1] for x in m], dtype=np.int64), np.stack([x[2] for x in m]).astype(np.int32))


GEN_SHAPES = [(128, 128, 8), (136, 120, 8), (13, 11, 2), (13, 11, 8)]
GEN_PLANS = [(mf.CSQ, mf.ARGB, False, (2, 0)), (mf.SCQ, mf.ARGB, False, (1, 0)), (mf.SCQ, mf.YCC, False, (4, 0)), (mf.CSQ, mf.ARGB, True, (2, 0)),
             (mf.CSQ, mf.YCC, True, (1, 1))]


@pytest.mark.parametrize("op,in_format,avg,ab", GEN_PLANS, ids=["hold-312", "hold-132", "hold-132-ycc", "avg", "avg-ycc"])
@pytest.mark.parametrize("W,H,f", GEN_SHAPES, ids=[f"{W}x{H}-f{f}" for W, H, f in GEN_SHAPES])
def test_distortion_shapes_of_the_general_kernel(csic, oracle, W, H, f, op, in_format, avg, ab):
    """128 x 128 at factor 8: 256 output pixels, one full block of k_dist_gen, and on the held_white frame every lane holds
    63 * 255^2 in R, G, B and Y, a wave 64 times that (262 180 800, the sum its 32-bit reduction is said to hold); 136 x 120: 255
    outputs; 13 x 11: the f x f blocks clamped at the right and bottom edge.  Both order classes, YCbCr input and AVG; the
    SSIM unit runs on the same frames (13 x 11 has one whole window and cut ones)."""
    a, b = ab
    name = "gen<" + ("avg" if avg else "hold") + (",ycc-in>" if in_format == mf.YCC else ">")
    c = dict(mf._cls(name, a, b, f, op, avg=avg, in_format=in_format, force=(f == 2 and op == mf.CSQ and not avg and in_format == mf.ARGB)),
             bits=(8, 8, 8))
    lever = "ycc" if in_format == mf.YCC else "gray"
    for names in (("held_white",), mf.RECIPE_SETS[8]):
        frames, ref = _shape_reference(oracle, c, lever, names, W, H, 3)
        if names == ("held_white",) and not avg and (W, H, f) == (128, 128, 8):
            assert ref[0][0].tolist()[3] == 256 * 63 * 65025
        with _plan(csic, W, H, c) as pl:
            _check_every_path(csic, pl, c, frames, ref, (name, op, a, b, W, H, f, names[0]))


@pytest.mark.parametrize("ab,rounding", list(zip(mf.CHROMA, (0, 1, 0, 1, 1, 0))), ids=[f"{a}{b}" for a, b in mf.CHROMA])
@pytest.mark.parametrize("f", [1, 2])
def test_distortion_shapes_of_the_fast_kernel(csic, oracle, f, ab, rounding):
    """136 x 62: rows of 34 units, 2108 (1054 at factor 2) units in three (two) blocks, the last one partial; the height is no
    multiple of 8, so the SSIM unit takes its general kernel on the same frames (7 whole window rows, the last rows cut)."""
    W, H = 136, 62
    a, b = ab
    c = dict(mf._cls(f"fast<f{f}>", a, b, f, mf.CSQ, rounding), bits=(8, 8, 8))
    for lever, names in (("gray", mf.RECIPE_SETS[8]), ("palette", mf.PALETTE_SET)):
        frames, ref = _shape_reference(oracle, c, lever, names, W, H, 4)
        with _plan(csic, W, H, c) as pl:
            _check_every_path(csic, pl, c, frames, ref, (c["cls"], a, b, rounding, lever), ssim_class="gen<hold>")


# ---- batches -----------------------------------------------------------------------------------------
BATCH_CLASSES = [c for c in mf.classes() if (c["cls"], c["f"], c["a"], c["b"], c["rounding"]) in
                 {("fast<f1>", 1, 2, 0, 0), ("fast<f2>", 2, 1, 0, 1), ("gen<hold>", 4, 2, 2, 0), ("gen<hold,ycc-in>", 2, 1, 0, 0), ("gen<avg>", 2, 4, 4, 1)}]


@pytest.mark.parametrize("c", BATCH_CLASSES, ids=mf.class_id)
def test_batches(csic, oracle, c):
    """Three frames that hold different recipes in the same windows, so that frame z's map and sums cannot be another frame's:
    the batch against the reference, and every frame alone against its row of the batch."""
    assert len(BATCH_CLASSES) == 5
    lever = "ycc" if c["in_format"] == mf.YCC else "gray"
    for W, H in ((264, 8), (40, 104)):
        case = dict(c, lever=lever, bits=(8, 8, 8), names=mf.RECIPE_SETS[8], W=W, H=H)
        ref = mf.reference(oracle, case)
        frames = ref["frames"][:3]
        for z in range(3):
            assert all(ref["where"][z][0][wi] != ref["where"][(z + 1) % 3][0][wi] for wi in range(len(ref["where"][z][0])))
        assert len({ref["map"][z].tobytes() for z in range(3)}) == 3
        with _plan(csic, W, H, case) as pl:
            d_in = _upload(frames)
            sums, qmap = _ssim(csic, pl, d_in, 3)
            sse = _dist(csic, pl, d_in, 3)
            _hold(qmap, ref["map"][:3], (mf.class_id(c), W, H, "batch map"), ref["where"])
            _hold(sums, ref["sums"][:3], (mf.class_id(c), W, H, "batch sums"))
            _hold(sse, ref["sse"][:3], (mf.class_id(c), W, H, "batch sse"))
            for z in range(3):
                d_one = _upload(frames[z])
                s1, m1 = _ssim(csic, pl, d_one, 1)
                assert np.array_equal(s1[0], sums[z]) and np.array_equal(m1[0], qmap[z]) and np.array_equal(_dist(csic, pl, d_one, 1)[0], sse[z])


# ---- the 4:x:0 replay row ------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(2, 0), (4, 0), (1, 0)])
def test_replay_pair(csic, oracle, a, b):
    """Factor 1, neutral chroma everywhere but in one column of the even rows.  Frame 0: the column is the last sample column, and
    that one pixel decides the chroma of the whole odd row below it, in every window of the row pair; frame 1: one column to the
    left, and the odd rows measure as neutral (tests/test_measure_frames_host.py shows both on the oracle).  A kernel that replays
    another column gives frame 1's numbers for frame 0.  fast<f1> and gen<hold> on the palette, gen<hold,ycc-in> on YCbCr input;
    40 x 16 (whole windows), 264 x 16 (a second block) and 43 x 19 (the sample column beyond the last whole window)."""
    h = mf.HOLD[a, b][0]
    for W, H in ((40, 16), (264, 16), (43, 19)):
        for rounding in (0, 1):
            for name, lever, in_format, force in (("fast<f1>", "palette", mf.ARGB, False), ("gen<hold>", "palette", mf.ARGB, True),
                                                  ("gen<hold,ycc-in>", "ycc", mf.YCC, False)):
                if W % 8:
                    if name == "fast<f1>":
                        continue
                    force = False                                                 # cut windows: the SSIM unit's general kernel by itself
                c = dict(mf._cls(name, a, b, 1, mf.CSQ, rounding, in_format=in_format, force=force), bits=(8, 8, 8))
                frames = np.stack([mf.replay_frames(W, H, h, lever, shift) for shift in (0, 1)])
                m = [mf.measure(oracle, fr, W, H, c) for fr in frames]
                ref = (np.array([x[0] for x in m], dtype=np.uint64), np.array([x[1] for x in m], dtype=np.int64), np.stack([x[2] for x in m]).astype(np.int32))
                assert (ref[0][0][4:] > ref[0][1][4:]).all() and not np.array_equal(ref[2][0][4:], ref[2][1][4:])
                with _plan(csic, W, H, c) as pl:
                    if W % 8 and name == "gen<hold>":                             # W % 4 != 0: both units take the general kernel by themselves
                        assert _names(pl) == ("k_dist_gen<hold>", "k_ssim_gen<hold>")
                    _check_every_path(csic, pl, c, frames, ref, (name, a, b, W, H, rounding))


# ---- fill independence -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", BATCH_CLASSES, ids=mf.class_id)
def test_fill_independence(csic, oracle, c):
    """Sums, map and workspace pre-filled with 0xEE, with zeros and with 0x55: the same results, and the bytes behind every
    extent keep their fill (_ssim / _dist)."""
    lever = "ycc" if c["in_format"] == mf.YCC else "gray"
    W, H = 264, 8
    case = dict(c, lever=lever, bits=(8, 8, 8), names=mf.RECIPE_SETS[8], W=W, H=H)
    ref = mf.reference(oracle, case)
    n = len(ref["frames"])
    with _plan(csic, W, H, case) as pl:
        d_in = _upload(ref["frames"])
        for f64, f32 in ((FILL64, FILL32), (0, 0), (0x5555555555555555, 0x55555555)):
            sums, qmap = _ssim(csic, pl, d_in, n, (f64, f32))
            _hold(qmap, ref["map"], (mf.class_id(c), hex(f32), "map"), ref["where"])
            _hold(sums, ref["sums"], (mf.class_id(c), hex(f32), "sums"))
            _hold(_dist(csic, pl, d_in, n, f64), ref["sse"], (mf.class_id(c), hex(f32), "sse"))
