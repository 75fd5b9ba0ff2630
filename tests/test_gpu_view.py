"""csic_decode_view_* on the GPU (k_view, k_view_gen of csic_decode.hip): a window of the decoded frame reduced by an s x s box.
Expected frames come from tests/view_ref.py -- the definition in numpy over the oracle's replicated packed output -- on inputs
that tests/test_view_ref.py shows to tell six wrong rules from the right one.  Every output buffer is followed by a canary and every
comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import view_ref as R
from conftest import GOLDEN, load_png_rgb

pytestmark = pytest.mark.gpu

CANARY = -286331154                      # 0xEEEEEEEE as int32
ARGB, YCC, PLANAR, BITS = R.ARGB, R.YCC, R.PLANAR, R.BITS
PAIRS = [(s, o) for s in (BITS, PLANAR, YCC, ARGB) for o in (ARGB, YCC) if (s, o) != (ARGB, YCC)]


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    assert csic_amd._native.lib().csic_device_count() >= 1
    return csic_amd


def _plan(csic, c, fmt=ARGB):
    cp = csic.make_c_params(c.W, c.H, c.a, c.b, *c.bits, c.f, c.op, rounding=0, out_format=fmt,
                            sampling=csic.Sampling.AVG if c.avg else csic.Sampling.HOLD_DECIMATE)
    return csic.Plan(cp, 0)


def _source(csic, c, fmt, argb=None, nframes=1):
    """The compressed frame(s) of a case in `fmt`, produced by the forward path of the same parameters."""
    import torch
    d_in = torch.from_numpy((R.frame(c) if argb is None else argb).view(np.int32)).cuda()
    with _plan(csic, c, fmt) as pl:
        return pl.process_device(d_in, nframes=nframes)


def _view_checked(pl, src, s, v, o=ARGB, nframes=1, offset=0):
    """decode_view_device into a buffer with canaries around the output; returns uint32 (nframes, height, width)."""
    import torch
    n = nframes * v.width * v.height
    buf = torch.full((offset + n + 64,), CANARY, dtype=torch.int32, device="cuda:0")
    pl.decode_view_device(src, v, s, buf[offset:offset + n], nframes=nframes, out_format=o)
    host = buf.cpu().numpy()
    assert (host[:offset] == CANARY).all() and (host[offset + n:] == CANARY).all(), "a canary around the output was overwritten"
    return host[offset:offset + n].view(np.uint32).reshape(nframes, v.height, v.width)


def _family(v, general=False):
    return "k_view<s%d," % v.scale if v.width % 4 == 0 and not general else "k_view_gen<"


@pytest.mark.parametrize("f", R.FACTORS)
def test_view_sweep_vs_the_definition(csic, oracle, f):
    """Every scale x this factor (s < f, s = f, s > f) x chroma mode x order class x sampling on 64 x 48, 37 x 35 and 130 x 70: the
    whole frame, views flush with the right and bottom edges, odd origins, widths 1, 4, 5 and 8; the default kernels and the
    general one (variant 9), and which one ran; the whole frame at scale 1 equals decode_device."""
    N = csic._native
    seen = set()
    for c in [c for c in R.sweep_cases() + R.DISCRIMINATING if c.f == f]:
        src = _source(csic, c, BITS)
        with _plan(csic, c) as pl:
            for s in R.SCALES:
                for v in R.views_of(c.W, c.H, s):
                    want = R.view(oracle, c, v)
                    for variant in (0, 9):
                        pl.tune(N.TUNE_VARIANT, variant)
                        name = pl.decode_view_kernel_name(BITS, v)
                        assert name.startswith(_family(v, variant == 9)), (name, v, variant)
                        seen.add(name.split(",")[0])
                        got = _view_checked(pl, src, BITS, v)[0]
                        assert np.array_equal(got, want), (name, c, v, variant)
            pl.tune(N.TUNE_VARIANT, 0)
            whole = R.View(0, 0, c.W, c.H, 1)
            assert np.array_equal(_view_checked(pl, src, BITS, whole)[0], pl.decode_device(src, BITS).cpu().numpy().view(np.uint32)), c
    assert {"k_view_gen<bits"} | {"k_view<s%d" % s for s in R.SCALES} <= seen, seen


@pytest.mark.parametrize("bits", [(8, 8, 8), (6, 5, 5), (3, 3, 2), (1, 1, 1)])
def test_view_sources_outputs_and_bit_sets(csic, oracle, bits):
    """The four sources x two outputs minus the refused pair, at one bit set, on 37 x 35 at factor 2 under 4:2:0 and on 64 x 48 at
    factor 4 in the other order class."""
    N = csic._native
    for c in (R.Case(37, 35, 2, 0, bits, 2, R.CSQ, False, "noise"), R.Case(64, 48, 2, 0, bits, 4, R.SCQ, False, "noise")):
        srcs = {s: _source(csic, c, s) for s in (BITS, PLANAR, YCC, ARGB)}
        with _plan(csic, c) as pl:
            for s in (1, 2, 8):
                for v in R.views_of(c.W, c.H, s)[:4]:
                    for variant in (0, 9):
                        pl.tune(N.TUNE_VARIANT, variant)
                        for src, o in PAIRS:
                            assert np.array_equal(_view_checked(pl, srcs[src], src, v, o)[0], R.view(oracle, c, v, o)), (c, v, src, o, variant)
            assert pl.decode_view_kernel_name(ARGB, R.View(0, 0, 4, 4, 1), YCC) == ""
            # scale 1, whole frame: decode_device, for every pair
            pl.tune(N.TUNE_VARIANT, 0)
            for src, o in PAIRS:
                assert np.array_equal(_view_checked(pl, srcs[src], src, R.View(0, 0, c.W, c.H, 1), o)[0],
                                      pl.decode_device(srcs[src], src, out_format=o).cpu().numpy().view(np.uint32)), (c, src, o)


def test_view_batch_of_three_odd_frames_and_an_offset_output(csic, oracle):
    """nframes = 3 on 37 x 35: frames 1 and 2 of a 5-wide view start at addresses that are only 4-byte aligned; and an output that
    starts 4 bytes into its buffer."""
    c = R.Case(37, 35, 2, 0, (6, 5, 5), 2, R.CSQ, False, "noise")
    rng = np.random.default_rng(7100)
    argb = rng.integers(0, 1 << 32, 3 * c.W * c.H, dtype=np.uint32)
    frames = argb.reshape(3, -1)
    for fmt in (BITS, YCC):
        src = _source(csic, c, fmt, argb, nframes=3)
        with _plan(csic, c) as pl:
            for v in (R.View(1, 3, 5, 3, 4), R.View(0, 0, 8, 8, 4), R.View(3, 5, 4, 3, 2), R.View(0, 0, 37, 35, 1)):
                for offset in (0, 1):
                    got = _view_checked(pl, src, fmt, v, nframes=3, offset=offset)
                    for k in range(3):
                        assert np.array_equal(got[k], R.view(oracle, c, v, argb=frames[k])), (fmt, v, offset, k)


def test_view_tuning_knobs(csic, oracle):
    """NO_VECTOR and FORCE_GENERIC select the general kernel; NONTEMPORAL 0 and every BLOCK_THREADS give the same pixels."""
    N = csic._native
    c = R.Case(130, 70, 2, 0, (6, 5, 5), 2, R.CSQ, False, "noise")
    src = _source(csic, c, BITS)
    v = R.View(1, 3, 16, 8, 8)
    want = R.view(oracle, c, v)
    for knob, value, family in ((N.TUNE_NO_VECTOR, 1, "k_view_gen<"), (N.TUNE_FORCE_GENERIC, 1, "k_view_gen<"), (N.TUNE_NONTEMPORAL, 0, "k_view<s8,"),
                                (N.TUNE_BLOCK_THREADS, 64, "k_view<s8,"), (N.TUNE_BLOCK_THREADS, 128, "k_view<s8,"), (N.TUNE_BLOCK_THREADS, 256, "k_view<s8,")):
        with _plan(csic, c) as pl:
            pl.tune(knob, value)
            name = pl.decode_view_kernel_name(BITS, v)
            assert name.startswith(family), (knob, value, name)
            if family != "k_view_gen<":
                assert ("cached" in name) == (knob == N.TUNE_NONTEMPORAL), name
            assert np.array_equal(_view_checked(pl, src, BITS, v)[0], want), (knob, value)


def test_view_graph_capture_and_replay(csic, oracle):
    import torch
    c = R.Case(64, 48, 2, 0, (6, 5, 5), 2, R.CSQ, False, "noise")
    v = R.View(1, 3, 12, 8, 4)
    rng = np.random.default_rng(7200)
    frames = [rng.integers(0, 1 << 32, c.W * c.H, dtype=np.uint32) for _ in range(2)]
    with _plan(csic, c, BITS) as pl:
        d_in = torch.from_numpy(frames[0].view(np.int32)).cuda()
        d_bits = pl.process_device(d_in)
        d_out = torch.zeros((v.height, v.width), dtype=torch.int32, device="cuda:0")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            pl.decode_view_device(d_bits, v, d_out=d_out)             # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            pl.process_device(d_in, d_bits)
            pl.decode_view_device(d_bits, v, d_out=d_out)
        for fr in frames[::-1]:
            d_in.copy_(torch.from_numpy(fr.view(np.int32)))
            d_out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(d_out.cpu().numpy().view(np.uint32), R.view(oracle, c, v, argb=fr))


def test_view_host_path(csic, oracle):
    c = R.Case(37, 35, 1, 0, (3, 3, 2), 2, R.CSQ, False, "noise")
    rng = np.random.default_rng(7300)
    argb = rng.integers(0, 1 << 32, 2 * c.W * c.H, dtype=np.uint32)
    h_bits = _source(csic, c, BITS, argb, nframes=2).cpu().numpy()
    h_ycc = _source(csic, c, YCC, argb, nframes=2).cpu().numpy()
    N = csic._native
    with _plan(csic, c, BITS) as pl:
        for v in (R.View(1, 1, 5, 3, 4), R.View(0, 0, 4, 4, 8)):
            want = np.stack([R.view(oracle, c, v, argb=argb.reshape(2, -1)[k]) for k in range(2)])
            got = pl.decode_view_host(h_bits, v, nframes=2)
            assert got.dtype == np.uint32 and got.shape == (2, v.height, v.width) and np.array_equal(got, want), v
            assert np.array_equal(pl.decode_view_host(h_ycc, v, YCC, nframes=2), want), v
        with pytest.raises(csic.IllegalArgumentException) as ei:
            pl.decode_view_host(h_bits.reshape(-1)[:-1], R.View(0, 0, 4, 4, 8), nframes=2)
        assert ei.value.status == N.EINVAL_SIZE
    top = csic.ImageCompressorTop(c.W, c.H, c.a, c.b, *c.bits, c.f, *[csic.ProcessingStep(x) for x in c.op])
    fr = argb[:c.W * c.H].reshape(c.H, c.W)
    v = csic.View(3, 5, 4, 3, 2)
    assert np.array_equal(top.decodeView(top.processPlanarBits(fr), v), R.view(oracle, c, R.View(*v), argb=fr.reshape(-1)))
    top.close()


def test_view_refusals(csic):
    import torch
    N = csic._native
    lib = N.lib()
    W, H = 64, 48
    c = R.Case(W, H, 2, 0, (6, 5, 5), 2, R.CSQ, False, "noise")
    with _plan(csic, c, BITS) as pl:
        lay = pl.planar_bits_layout
        src = torch.zeros(lay.frame_bytes + 256, dtype=torch.uint8, device="cuda:0")
        packed = torch.zeros(pl.out_width * pl.out_height, dtype=torch.int32, device="cuda:0")
        out = torch.zeros(W * H, dtype=torch.int32, device="cuda:0")
        ps, pp, po = C.c_void_p(src.data_ptr()), C.c_void_p(packed.data_ptr()), C.c_void_p(out.data_ptr())

        def call(view, s=ps, fmt=BITS, o=po, ofmt=ARGB, nf=1, plan=pl._h):
            return lib.csic_decode_view_device(plan, s, fmt, C.byref(N.CsicView(*view)) if view is not None else None, o, ofmt, nf, None)

        good = (8, 4, 12, 10, 4)                                            # 8 + 48 <= 64, 4 + 40 <= 48
        assert call(good) == N.OK
        # one pixel outside the frame on each side
        for bad in ((-1, 4, 12, 10, 4), (8, -1, 12, 10, 4), (17, 4, 12, 10, 4), (8, 9, 12, 10, 4), (0, 0, 65, 1, 1),
                    (0, 0, 1, 49, 1), (0, 0, 5, 1, 16), (0, 0, 1, 4, 16)):
            assert call(bad) == N.EINVAL_SIZE, bad
            assert "inside" in lib.csic_last_error().decode()
            assert pl.decode_view_kernel_name(BITS, bad) == ""
        for flush in ((16, 8, 12, 10, 4), (0, 0, 64, 48, 1), (0, 0, 4, 3, 16)):
            assert call(flush) == N.OK, flush
        assert call((0, 0, 2 ** 31 - 1, 2, 16)) == N.EINVAL_SIZE            # 64-bit arithmetic
        for zero in ((0, 0, 0, 4, 1), (0, 0, 4, 0, 1), (0, 0, -4, 4, 1)):
            assert call(zero) == N.EINVAL_SIZE, zero
        for scale in (3, 0, -2, 32, 5):
            assert call((0, 0, 1, 1, scale)) == N.EINVAL_SIZE, scale
            assert "scale" in lib.csic_last_error().decode()
        assert call(good, plan=None) == N.EINVAL_NULL and call(None) == N.EINVAL_NULL
        assert call(good, s=None) == N.EINVAL_NULL and call(good, o=None) == N.EINVAL_NULL
        for nf in (0, -3):
            assert call(good, nf=nf) == N.EINVAL_SIZE
        assert call(good, s=pp, fmt=ARGB, ofmt=YCC) == N.EINVAL_FORMAT
        assert "inverse" in lib.csic_last_error().decode()
        assert call(good, fmt=4) == N.EINVAL_FORMAT and call(good, ofmt=BITS) == N.EINVAL_FORMAT
        for s in (BITS, PLANAR):                                            # a misaligned planar source
            assert call(good, s=C.c_void_p(src.data_ptr() + 128), fmt=s) == N.EINVAL_SIZE
        assert call(good, s=C.c_void_p(packed.data_ptr() + 2), fmt=YCC) == N.EINVAL_SIZE
        assert call(good, s=pp, fmt=YCC, o=C.c_void_p(out.data_ptr() + 2)) == N.EINVAL_SIZE
        torch.cuda.synchronize()
        hs, ho = np.zeros(lay.frame_bytes, dtype=np.uint8), np.zeros(120, dtype=np.uint32)
        phs, pho, hv = hs.ctypes.data_as(C.c_void_p), ho.ctypes.data_as(C.c_void_p), C.byref(N.CsicView(*good))
        assert lib.csic_decode_view_host(pl._h, phs, hs.size, BITS, hv, pho, 120, ARGB, 1) == N.OK
        assert lib.csic_decode_view_host(pl._h, None, hs.size, BITS, hv, pho, 120, ARGB, 1) == N.EINVAL_NULL
        assert lib.csic_decode_view_host(pl._h, phs, hs.size, BITS, None, pho, 120, ARGB, 1) == N.EINVAL_NULL
        assert lib.csic_decode_view_host(pl._h, phs, hs.size - 1, BITS, hv, pho, 120, ARGB, 1) == N.EINVAL_SIZE
        assert lib.csic_decode_view_host(pl._h, phs, hs.size, BITS, hv, pho, 121, ARGB, 1) == N.EINVAL_SIZE
        assert lib.csic_decode_view_host(pl._h, phs, hs.size, ARGB, hv, pho, 120, YCC, 1) == N.EINVAL_FORMAT
        # the Python layer
        with pytest.raises(csic.IllegalArgumentException):
            pl.decode_view_device(src[:lay.frame_bytes - 1], good)
        with pytest.raises(csic.IllegalArgumentException):
            pl.decode_view_device(src[:lay.frame_bytes], good, d_out=out[:119])
        with pytest.raises(csic.IllegalArgumentException) as ei:
            pl.decode_view_device(src[:lay.frame_bytes], (0, 0, 4, 4, 3))
        assert ei.value.status == N.EINVAL_SIZE


def test_view_thumbnail_of_the_golden_input(csic, oracle, input_images):
    """in512.png at 4:2:0, 6/5/5, factor 2: the whole frame at scale 8, a 64 x 64 thumbnail, on the fast kernel."""
    rgb = input_images["in512"]
    argb = oracle.rgb_to_argb(rgb).reshape(-1)
    c = R.Case(512, 512, 2, 0, (6, 5, 5), 2, R.CSQ, False, "golden")
    v = R.View(0, 0, 64, 64, 8)
    src = _source(csic, c, BITS, argb)
    with _plan(csic, c) as pl:
        assert pl.decode_view_kernel_name(BITS, v).startswith("k_view<s8,bits,argb,nt>")
        assert np.array_equal(_view_checked(pl, src, BITS, v)[0], R.view(oracle, c, v, argb=argb))


def test_decompress_window_and_scale(csic, oracle, input_images, tmp_path):
    """compress -> decompress --window 100,60,256,128 --scale 4 gives a 64 x 32 PNG equal to the definition; --frame and
    --output-pattern on a three-frame version-5 file."""
    from csic_amd.app import main
    src = os.path.join(GOLDEN, "inputs", "in512.png")
    packed, back = str(tmp_path / "in512.csic"), str(tmp_path / "view.png")
    args = ["--a", "2", "--b", "0", "--yq", "6", "--cbq", "5", "--crq", "5", "--sf", "2", "--op1", "chroma", "--op2", "spatial", "--op3", "color"]
    assert main(["compress", "--input", src, "--output", packed] + args) == 0
    assert main(["decompress", "--input", packed, "--output", back, "--window", "100,60,256,128", "--scale", "4"]) == 0
    argb = oracle.rgb_to_argb(input_images["in512"]).reshape(-1)
    c = R.Case(512, 512, 2, 0, (6, 5, 5), 2, R.CSQ, False, "golden")
    got = load_png_rgb(back)
    assert got.shape == (32, 64, 3) and np.array_equal(got, oracle.argb_to_rgb(R.view(oracle, c, R.View(100, 60, 64, 32, 4), argb=argb)))
    # the remainder of a window that is no multiple of the scale is dropped; the default window is the whole frame
    assert main(["decompress", "--input", packed, "--output", back, "--window", "1,3,103,50", "--scale", "8"]) == 0
    assert np.array_equal(load_png_rgb(back), oracle.argb_to_rgb(R.view(oracle, c, R.View(1, 3, 12, 6, 8), argb=argb)))
    assert main(["decompress", "--input", packed, "--output", back, "--scale", "16"]) == 0
    assert np.array_equal(load_png_rgb(back), oracle.argb_to_rgb(R.view(oracle, c, R.View(0, 0, 32, 32, 16), argb=argb)))
    # refusals: outside the frame, smaller than one box
    assert main(["decompress", "--input", packed, "--output", back, "--window", "400,0,113,64"]) == 1
    assert main(["decompress", "--input", packed, "--output", back, "--window", "0,0,7,64", "--scale", "8"]) == 1
    # a sequence: three frames, temporal delta coding (container version 5)
    from PIL import Image
    paths = []
    for k in range(3):
        paths.append(str(tmp_path / f"f{k}.png"))
        Image.fromarray(np.roll(input_images["in512"][:96, :128], 3 * k, axis=1)).save(paths[-1])
    seq = str(tmp_path / "seq.csic")
    assert main(["compress", "--inputs", ",".join(paths), "--gop", "3", "--output", seq, "--coding", "groups"] + args) == 0
    assert csic.container_info(seq).version == 5
    c = R.Case(128, 96, 2, 0, (6, 5, 5), 2, R.CSQ, False, "golden")
    assert main(["decompress", "--input", seq, "--output-pattern", str(tmp_path / "v_%d.png"), "--window", "4,2,96,64", "--scale", "2"]) == 0
    assert main(["decompress", "--input", seq, "--output", back, "--frame", "2", "--window", "4,2,96,64", "--scale", "2"]) == 0
    for k in range(3):
        fr = oracle.rgb_to_argb(load_png_rgb(paths[k])).reshape(-1)
        want = oracle.argb_to_rgb(R.view(oracle, c, R.View(4, 2, 48, 32, 2), argb=fr))
        assert np.array_equal(load_png_rgb(str(tmp_path / f"v_{k}.png")), want), k
        if k == 2:
            assert np.array_equal(load_png_rgb(back), want)
