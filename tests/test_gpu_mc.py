"""The device codec of the motion-compensated temporal layer (csic_mc.hip: k_mc_search, k_mc_table, k_mc_delta, k_mc_undelta) against the
numpy statement of tests/mc_ref.py, on code planes built to order as W x H, 4:4:4, factor 1 -- every plane has W H samples in rows of W;
the PLANAR_BITS frames are built on the host and uploaded.  The shapes are the smallest at which the kernels can go wrong:

    1 x 1, 31 x 1, 33 x 1     everything clamps; ragged groups
    8 x 5                     rows shorter than a group
    16 x 16, 16 x 18          G = 8 and 9: a nibble dword that is exactly full, and one nibble into the next
    32 x 4                    rows equal to a group
    100 x 21                  a second wave
    128 x 64                  exactly one block
    2731 x 3                  one lane into a second block, with dy reaching across blocks
    200 x 100                 three blocks, windows across block edges

each at every q = 1 .. 8 as (q, q, q) and the mixed triples (6, 5, 5), (5, 5, 3), (3, 3, 2), with six contents (tests/test_mc_host.py:
random, identical, the wrap, a whole-plane shift, two halves with different vectors, 20 stripes with 20 vectors), a range of 0, 1, 2
and -- on the small shapes -- 7, and (nframes, gop) of (1, 1), (2, 2), (5, 3), (5, 7).  A delta frame depends on its own and the previous
frame only, so the reference computes every frame once as a delta frame and a (nframes, gop) case picks.  Per case: tables, nibbles and
difference frames byte for byte, 0xEE outside the payload ranges and behind map_bytes, the source only read, undelta restores it.  Then
undelta on maps built to order (any nibble, any displacement), the cached instantiations, frames from the forward path through
mc_delta -> Rice -> a version-6 file -> read -> decode, one linear graph capture of mc_delta -> Rice pack -> unpack -> mc_undelta, and
the refusals, in place included.  Run with `-m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from delta_ref import frame_buffers, map_buffers
from mc_ref import map_bytes_of, ref_mc_delta, ref_mc_layout, ref_mc_undelta
from test_container import MODES
from test_gpu_pack import EE, _filled, _plan, _source
from test_mc_host import CONTENTS, LARGE, MOST, SMALL, TRIPLES, check_layout, sequence

pytestmark = pytest.mark.gpu

CASES = [(1, 1), (2, 2), (5, 3), (5, 7)]


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    assert csic_amd._native.lib().csic_device_count() >= 1
    return csic_amd


def _reference(lay, stride, frames, bits, W, R):
    """-> (src, as_delta, maps_delta): the frame buffers (0xEE outside the payload: a key frame's difference frame is its source buffer),
    every frame's difference frame as a delta frame, and its map; row 0 of the latter two is not used."""
    src = frame_buffers(lay, frames, bits, EE)
    diffs, maps, _ = ref_mc_delta(frames, bits, [W] * 3, len(frames) + 1, R)
    return src, frame_buffers(lay, diffs, bits, EE), map_buffers(maps, stride, EE)


def _want(ref, nframes, gop, map_bytes):
    src, as_delta, maps_delta = ref
    key = np.arange(nframes) % gop == 0
    want_m = maps_delta[:nframes].copy()
    want_m[key, :map_bytes] = 0
    return np.where(key[:, None], src[:nframes], as_delta[:nframes]), want_m


def _run(pl, d_src, nframes, gop, R):
    """mc_delta then mc_undelta on the device, every destination pre-filled with 0xEE.  -> (diff, maps, back) on the device."""
    fb, ms = pl.frame_bytes, pl.mc_layout.map_stride
    diff, maps = pl.mc_delta_device(d_src[:nframes], nframes, gop, R, _filled((nframes, fb)), _filled((nframes, ms)))
    back = pl.mc_undelta_device(diff, maps, nframes, gop, _filled((nframes, fb)))
    return diff, maps, back


def _check_all(csic, bits, shapes, ranges, cases, contents=CONTENTS, cached=False):
    import torch
    N = csic._native
    rng = np.random.default_rng(18500 + 100 * bits[0] + 10 * bits[1] + bits[2])
    for i, (W, H) in enumerate(shapes):
        with _plan(csic, W, H, 4, 4, bits) as pl:
            mb, stride = check_layout(pl.mc_layout, [W * H] * 3, [W] * 3)
            assert pl.mc_kernel_name == "k_mc_delta<q%d,%d,%d,nt>" % bits
            if cached:
                pl.tune(N.TUNE_NONTEMPORAL, 0)
                assert pl.mc_kernel_name == "k_mc_delta<q%d,%d,%d,cached>" % bits
            for j, content in enumerate(contents):
                R = ranges[(i + j) % len(ranges)]
                ref = _reference(pl.planar_bits_layout, stride, sequence(content, W, H, bits, R, rng), bits, W, R)
                d_src = torch.from_numpy(ref[0]).cuda()
                for nframes, gop in cases:
                    tag = (bits, W, H, content, R, nframes, gop, cached)
                    want_d, want_m = _want(ref, nframes, gop, mb)
                    diff, maps, back = _run(pl, d_src, nframes, gop, R)
                    assert torch.equal(maps, torch.from_numpy(want_m).cuda()), tag        # tables and nibbles, 0xEE behind map_bytes
                    assert torch.equal(diff, torch.from_numpy(want_d).cuda()), tag        # byte for byte, 0xEE outside the payload ranges
                    assert torch.equal(back, d_src[:nframes]), tag                        # undelta restores the source, 0xEE kept
                assert np.array_equal(d_src.cpu().numpy(), ref[0]), (bits, W, H, content)  # the source is only read


@pytest.mark.parametrize("bits", TRIPLES)
def test_small_shapes_every_content_range_frame_count_and_gop(csic, bits):
    _check_all(csic, bits, SMALL, (0, 1, 2, 1, 2, 7, 2), CASES)


@pytest.mark.parametrize("bits", TRIPLES)
def test_block_edges_every_content_and_range(csic, bits):
    _check_all(csic, bits, LARGE, (2, 1, 0, 2), [(2, 2), (5, 3)])


@pytest.mark.parametrize("bits", TRIPLES)
def test_cached_variants(csic, bits):
    _check_all(csic, bits, ((33, 1), (100, 21), (2731, 3)), (2, 1), [(5, 2), (5, 7)], contents=("halves", "stripes"), cached=True)


@pytest.mark.parametrize("bits", [(1, 1, 1), (8, 8, 8), (6, 5, 5), (3, 3, 2)])
def test_undelta_on_maps_built_to_order(csic, bits):
    """Any nibble reads one of the 16 words and any word clamps: tables of any T with displacements up to INT32_MIN and INT32_MAX, nibbles
    up to 15 whatever T says."""
    import torch
    rng = np.random.default_rng(18600 + bits[0])
    for W, H in ((33, 1), (16, 18), (100, 21), (2731, 3)):
        n, nframes, gop = W * H, 4, 3
        with _plan(csic, W, H, 4, 4, bits) as pl:
            lay, ml = pl.planar_bits_layout, pl.mc_layout
            diffs = [[rng.integers(0, 1 << q, n) for q in bits] for _ in range(nframes)]
            maps = []
            for k in range(nframes):
                tables = []
                for p in range(3):
                    words = rng.integers(-3 * W, 3 * W + 1, 16)
                    words[rng.integers(1, 16, 4)] = (-2 ** 31, 2 ** 31 - 1, n, -n)
                    words[0] = rng.integers(0, 16)
                    tables.append(words.tolist())
                maps.append(map_bytes_of(tables, [rng.integers(0, 16, (n + 31) // 32) for _ in range(3)]))
            want = frame_buffers(lay, ref_mc_undelta(diffs, maps, bits, gop), bits, EE)
            d_diff = torch.from_numpy(frame_buffers(lay, diffs, bits, EE)).cuda()
            d_maps = torch.from_numpy(map_buffers(maps, ml.map_stride, EE)).cuda()
            back = pl.mc_undelta_device(d_diff, d_maps, nframes, gop, _filled((nframes, pl.frame_bytes)))
            assert np.array_equal(back.cpu().numpy(), want), (bits, W, H)


def _payload_mask(lay):
    keep = np.zeros(lay.frame_bytes, dtype=bool)
    for o, nb in ((lay.y_offset, lay.y_bytes), (lay.cb_offset, lay.cb_bytes), (lay.cr_offset, lay.cr_bytes)):
        keep[o:o + nb] = True
    return keep


FORWARD = [(W, H, a, b, f, False) for W, H in ((201, 27), (128, 64)) for a, b in MODES for f in (1, 2)] + [(201, 27, 2, 0, 2, True)]


@pytest.mark.parametrize("W,H,a,b,f,avg", FORWARD)
def test_frames_from_the_forward_path_through_a_version_6_file(csic, tmp_path, W, H, a, b, f, avg):
    """process -> mc_delta -> rice_pack_device -> write_container_coded(maps=..., motion=R) -> read_container gives the processed frames,
    the file is the host writer's, and the decode of what was read is the decode of the originals."""
    import torch
    bits, nframes, gop, R = (6, 5, 5), 4, 3, 2
    rng = np.random.default_rng(18800 + W + 7 * a + b + f)
    big = rng.integers(0, 1 << 32, (H + 8, W + 8), dtype=np.uint32)
    frames = [np.ascontiguousarray(big[k:k + H, 2 * k:2 * k + W]).reshape(-1) for k in range(nframes)]   # a pan of (1, 2) per frame
    with _plan(csic, W, H, a, b, bits, f, avg=avg) as pl:
        buf = _source(pl, np.stack(frames), nframes)
        diff, maps = pl.mc_delta_device(buf, nframes, gop, R)
        coded, sizes = pl.rice_pack_device(diff, nframes)
        torch.cuda.synchronize()
        path = str(tmp_path / "seq.csic")
        csic.write_container_coded(path, pl.c_params, coded.cpu().numpy(), sizes.cpu().numpy(), coding="rice", maps=maps.cpu().numpy(), gop=gop, motion=R)
        host = str(tmp_path / "host.csic")
        csic.write_container(host, pl.c_params, buf.cpu().numpy(), coding="rice", gop=gop, motion=R)
        assert open(path, "rb").read() == open(host, "rb").read()              # the host writer's file
        info = csic.container_info(path)
        assert (info.version, info.nframes, info.gop, info.motion) == (6, nframes, gop, R)
        inter = csic.container_inter_groups(path)
        assert inter[0].sum() == 0 and inter[3].sum() == 0 and inter[1].sum() > 0
        _, n, back = csic.read_container(path)
        want = buf.cpu().numpy().copy()
        want[:, ~_payload_mask(pl.planar_bits_layout)] = 0
        assert n == nframes and np.array_equal(back, want)
        assert torch.equal(pl.decode_device(torch.from_numpy(back).cuda(), nframes=nframes), pl.decode_device(buf, nframes=nframes))


def test_capture_and_replay_in_a_graph(csic):
    """One linear capture of mc_delta -> Rice pack -> unpack -> mc_undelta, replayed on new contents."""
    import torch
    W, H, bits, nframes, gop, R = 200, 41, (6, 5, 5), 5, 3, 2
    rng = np.random.default_rng(18700)
    with _plan(csic, W, H, 4, 4, bits) as pl:
        lay, ml = pl.planar_bits_layout, pl.mc_layout
        refs = [_reference(lay, ml.map_stride, sequence(c, W, H, bits, R, rng), bits, W, R) for c in ("random", "halves", "stripes")]
        src = torch.from_numpy(refs[0][0]).cuda()
        fb, ms, bound = pl.frame_bytes, ml.map_stride, pl.rice_layout.bound_bytes
        diff, maps, coded, undone, back = _filled((nframes, fb)), _filled((nframes, ms)), _filled((nframes, bound)), _filled((nframes, fb)), _filled((nframes, fb))
        ws = _filled((nframes * ml.workspace_frame_bytes,))

        def chain():
            pl.mc_delta_device(src, nframes, gop, R, diff, maps, ws)
            _, sizes = pl.rice_pack_device(diff, nframes, coded)
            pl.rice_unpack_device(coded, nframes, undone)
            pl.mc_undelta_device(undone, maps, nframes, gop, back)
            return sizes
        chain()                                             # the warm-up
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                chain()
        torch.cuda.current_stream().wait_stream(s)
        for ref in refs[1:]:
            src.copy_(torch.from_numpy(ref[0]).cuda())
            g.replay()
            torch.cuda.synchronize()
            want_d, want_m = _want(ref, nframes, gop, ml.map_bytes)
            assert np.array_equal(maps.cpu().numpy(), want_m) and np.array_equal(diff.cpu().numpy(), want_d)
            assert torch.equal(undone, diff) and torch.equal(back, src)


def test_refusals(csic):
    """All before any device is touched."""
    import torch
    L, N = csic._native.lib(), csic._native
    with _plan(csic, 64, 16, 2, 0, (6, 5, 5)) as pl:
        fb, ml = pl.frame_bytes, pl.mc_layout
        ms, wsb = ml.map_stride, 3 * ml.workspace_frame_bytes
        frames = torch.zeros(4 * fb + 256, dtype=torch.uint8, device="cuda")
        diff = torch.zeros(4 * fb + 256, dtype=torch.uint8, device="cuda")
        maps = torch.zeros(3 * ms + 256, dtype=torch.uint8, device="cuda")
        work = torch.zeros(wsb + 256, dtype=torch.uint8, device="cuda")
        s = pl._stream()
        ptr = lambda t, o=0: C.c_void_p(t.data_ptr() + o)

        def delta(n=3, gop=2, R=2, f=ptr(frames), d=ptr(diff), m=ptr(maps), plan=pl._h, w=ptr(work), wb=wsb):
            return L.csic_mc_delta_device(plan, f, n, gop, R, d, m, w, wb, s)

        def undelta(n=3, gop=2, f=ptr(frames), d=ptr(diff), m=ptr(maps), plan=pl._h):
            return L.csic_mc_undelta_device(plan, d, m, n, gop, f, s)
        nul = C.c_void_p(None)
        for call in (delta, undelta):
            assert call(plan=None) == N.EINVAL_NULL and call(f=nul) == N.EINVAL_NULL and call(d=nul) == N.EINVAL_NULL and call(m=nul) == N.EINVAL_NULL
            assert call(n=0) == N.EINVAL_SIZE and call(n=65536) == N.EINVAL_SIZE and call(gop=0) == N.EINVAL_SIZE and call(gop=-1) == N.EINVAL_SIZE
            assert call(f=ptr(frames, 64)) == N.EINVAL_SIZE and call(d=ptr(diff, 128)) == N.EINVAL_SIZE and call(m=ptr(maps, 4)) == N.EINVAL_SIZE
            assert call(d=ptr(frames)) == N.EINVAL_SIZE                        # in place is not allowed
            assert call(d=ptr(frames, fb)) == N.EINVAL_SIZE                    # a partial overlap (frame_bytes is a multiple of 256)
            assert call(m=ptr(frames, 256)) == N.EINVAL_SIZE                   # the maps inside the frames
            assert L.csic_last_error().decode() != ""
            assert call() == N.OK and call(gop=100000) == N.OK                 # apart; one key frame
        assert delta(R=-1) == N.EINVAL_SIZE and delta(R=8) == N.EINVAL_SIZE and delta(R=0) == N.OK and delta(R=7) == N.OK
        assert delta(w=nul) == N.EINVAL_NULL and delta(wb=wsb - 1) == N.EINVAL_SIZE and delta(w=ptr(work, 4)) == N.EINVAL_SIZE
        torch.cuda.synchronize()
        want = np.zeros((3, ms), dtype=np.uint8)                               # zeros: constant frames, every group a tie; the last call's
        want[1, 0:129:64] = 1                                                  # delta frame has tables of the zero vector alone
        assert not frames.any() and not diff.any() and np.array_equal(maps[:3 * ms].cpu().numpy().reshape(3, ms), want)
        assert L.csic_mc_kernel_name(None) == b""
        with pytest.raises(csic.IllegalArgumentException):
            pl.mc_delta_device(frames[:fb + 1])
        with pytest.raises(csic.IllegalArgumentException):
            pl.mc_undelta_device(diff[:2 * fb].reshape(2, fb), None, 2, 2)
    # parameters the container does not take: a plan whose input is YCbCr
    cp = csic.make_c_params(64, 16, 2, 0, 6, 5, 5, 1, (3, 1, 2), in_format=N.FMT_YCBCR888X)
    with csic.Plan(cp, 0) as pl:
        z = torch.zeros(8192, dtype=torch.uint8, device="cuda")
        assert L.csic_mc_delta_device(pl._h, C.c_void_p(z.data_ptr()), 1, 1, 1, C.c_void_p(z.data_ptr() + 2048), C.c_void_p(z.data_ptr() + 4096),
                                      C.c_void_p(z.data_ptr() + 6144), 2048, pl._stream()) == N.EINVAL_FORMAT
