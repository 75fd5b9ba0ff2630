"""The device codec of the temporal layer (csic_delta.hip: k_delta, k_undelta) against the numpy statement of tests/delta_ref.py, on code
planes built to order (n x 1, 4:4:4, factor 1: every plane has exactly n samples; the PLANAR_BITS frames are built on the host and
uploaded, as tests/test_gpu_codec_planes.py does).  The sizes are the smallest at which the kernels can go wrong:

    n = 1, 31, 33     ragged groups, G = 1, 2
    n = 1000, 1025    G = 32, 33: a map dword that is exactly full, and one bit into the next
    n = 2053          G = 65: both halves of a ballot and a second wave
    n = 8192, 8193    exactly one block, and a second block of one lane
    n = 20 000        three blocks

each at every q = 1 .. 8 as (q, q, q) and the mixed triples (6, 5, 5), (5, 5, 3), (3, 3, 2), with 1, 2 and 5 frames, gop 1, 2, 3 and 7,
and four contents: random frames, identical frames, groups that are identical and random in turn, and the wrap.  A delta frame depends
on its own and the previous frame only, so the reference computes every frame once as a key frame and once as a delta frame and a
(nframes, gop) case picks.  Per case: difference frames and maps byte for byte, 0xEE outside the payload ranges and behind map_bytes,
the source only read, undelta restores it.  Then the in-place form, the cached instantiations, frames from the forward path through
delta -> Rice -> a version-5 file -> read -> decode, one linear graph capture of delta -> pack -> unpack -> undelta, and the refusals.
Run with `-m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from delta_ref import frame_buffers, map_buffers, ref_delta, ref_map_layout
from test_container import MODES
from test_gpu_pack import EE, _filled, _plan, _source

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 33, 1000, 1025, 2053, 8192, 8193, 20000)
TRIPLES = [(q, q, q) for q in range(1, 9)] + [(6, 5, 5), (5, 5, 3), (3, 3, 2)]
FRAMES, GOPS, MOST = (1, 2, 5), (1, 2, 3, 7), 5
CONTENTS = ("random", "identical", "alternating", "wrap")


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    assert csic_amd._native.lib().csic_device_count() >= 1
    return csic_amd


def _sequence(content, n, bits, rng):
    """MOST frames of three planes of n codes."""
    if content == "random":
        return [[rng.integers(0, 1 << q, n) for q in bits] for _ in range(MOST)]
    if content == "identical":
        one = [np.cumsum(rng.integers(-1, 2, n)) % (1 << q) for q in bits]
        return [one] * MOST
    if content == "alternating":                            # every other group is the previous frame's, the rest is redrawn
        frames = [[rng.integers(0, 1 << q, n) for q in bits]]
        for k in range(1, MOST):
            keep = (np.arange(n) // 32 + k) % 2 == 0
            frames.append([np.where(keep, c, rng.integers(0, 1 << q, n)) for c, q in zip(frames[-1], bits)])
        return frames
    even = np.arange(n) % 2 == 0                            # the wrap: 0 over 2^q - 1 in every other sample, and back
    tops = [(1 << q) - 1 for q in bits]
    r = [np.where(even, t, max(t - 1, 0)).astype(np.int64) for t in tops]
    c = [np.where(even, 0, t).astype(np.int64) for t in tops]
    return [r, c, r, c, r]


def _reference(lay, stride, frames, bits):
    """-> (src, as_delta, maps_delta): the frame buffers (0xEE outside the payload: a key frame's difference frame is its source buffer),
    every frame's difference frame as a delta frame, and its map; row 0 of the latter two is not used."""
    src = frame_buffers(lay, frames, bits, EE)
    diffs, maps, _ = ref_delta(frames, bits, len(frames) + 1)
    return src, frame_buffers(lay, diffs, bits, EE), map_buffers(maps, stride, EE)


def _want(ref, nframes, gop, map_bytes):
    src, as_delta, maps_delta = ref
    key = np.arange(nframes) % gop == 0
    want_m = maps_delta[:nframes].copy()
    want_m[key, :map_bytes] = 0
    return np.where(key[:, None], src[:nframes], as_delta[:nframes]), want_m


def _run(pl, d_src, nframes, gop, in_place=False):
    """delta then undelta on the device, every destination pre-filled with 0xEE.  -> (diff, maps, back) on the device."""
    fb, ms = pl.frame_bytes, pl.delta_layout.map_stride
    if in_place:
        work = d_src[:nframes].clone()
        diff, maps = pl.delta_device(work, nframes, gop, work, _filled((nframes, ms)))
        keep = diff.clone()
        back = pl.undelta_device(work, maps, nframes, gop, work)
        return keep, maps, back
    diff, maps = pl.delta_device(d_src[:nframes], nframes, gop, _filled((nframes, fb)), _filled((nframes, ms)))
    back = pl.undelta_device(diff, maps, nframes, gop, _filled((nframes, fb)))
    return diff, maps, back


def _check_all(csic, bits, sizes, contents, cases, in_place=False, cached=False):
    import torch
    N = csic._native
    rng = np.random.default_rng(16500 + 100 * bits[0] + 10 * bits[1] + bits[2])
    for n in sizes:
        with _plan(csic, n, 1, 4, 4, bits) as pl:
            ml = pl.delta_layout
            G, off, mb, stride = ref_map_layout([n] * 3)
            assert (list(ml.groups), list(ml.map_offset), ml.map_bytes, ml.map_stride) == (G, off, mb, stride)
            assert pl.delta_kernel_name == "k_delta<q%d,%d,%d,nt>" % bits
            if cached:
                pl.tune(N.TUNE_NONTEMPORAL, 0)
                assert pl.delta_kernel_name == "k_delta<q%d,%d,%d,cached>" % bits
            for content in contents:
                ref = _reference(pl.planar_bits_layout, stride, _sequence(content, n, bits, rng), bits)
                d_src = torch.from_numpy(ref[0]).cuda()
                for nframes, gop in cases:
                    tag = (bits, n, content, nframes, gop, in_place, cached)
                    want_d, want_m = _want(ref, nframes, gop, mb)
                    diff, maps, back = _run(pl, d_src, nframes, gop, in_place)
                    assert torch.equal(diff, torch.from_numpy(want_d).cuda()), tag        # byte for byte, 0xEE outside the payload ranges
                    assert torch.equal(maps, torch.from_numpy(want_m).cuda()), tag        # byte for byte, 0xEE behind map_bytes
                    assert torch.equal(back, d_src[:nframes]), tag                        # undelta restores the source, 0xEE kept
                assert np.array_equal(d_src.cpu().numpy(), ref[0]), (bits, n, content)    # the source is only read


@pytest.mark.parametrize("bits", TRIPLES)
def test_every_size_content_frame_count_and_gop(csic, bits):
    _check_all(csic, bits, SIZES, CONTENTS, [(nf, gop) for nf in FRAMES for gop in GOPS])


@pytest.mark.parametrize("bits", [(1, 1, 1), (8, 8, 8), (6, 5, 5), (3, 3, 2)])
def test_in_place_in_both_directions(csic, bits):
    _check_all(csic, bits, (33, 1025, 8193), ("alternating", "wrap"), [(5, 1), (5, 3), (2, 7)], in_place=True)


@pytest.mark.parametrize("bits", TRIPLES)
def test_cached_variants(csic, bits):
    _check_all(csic, bits, (33, 2053, 8193), ("alternating",), [(5, 2), (5, 7)], cached=True)


def _payload_mask(lay):
    keep = np.zeros(lay.frame_bytes, dtype=bool)
    for o, nb in ((lay.y_offset, lay.y_bytes), (lay.cb_offset, lay.cb_bytes), (lay.cr_offset, lay.cr_bytes)):
        keep[o:o + nb] = True
    return keep


FORWARD = [(W, H, a, b, f, False) for W, H in ((201, 27), (128, 64)) for a, b in MODES for f in (1, 2)] + [(201, 27, 2, 0, 2, True)]


@pytest.mark.parametrize("W,H,a,b,f,avg", FORWARD)
def test_frames_from_the_forward_path_through_a_version_5_file(csic, tmp_path, W, H, a, b, f, avg):
    """process -> delta -> rice_pack_device -> write_container_coded(maps=...) -> read_container gives the processed frames, and the
    decode of what was read is the decode of the originals."""
    import torch
    bits, nframes, gop = (6, 5, 5), 4, 3
    rng = np.random.default_rng(16600 + W + 7 * a + b + f)
    frames = [rng.integers(0, 1 << 32, W * H, dtype=np.uint32)]
    for k in range(1, nframes):                             # the upper part stays, the rest is redrawn
        nxt = frames[-1].copy()
        nxt[W * H // 2:] = rng.integers(0, 1 << 32, W * H - W * H // 2, dtype=np.uint32)
        frames.append(nxt)
    with _plan(csic, W, H, a, b, bits, f, avg=avg) as pl:
        buf = _source(pl, np.stack(frames), nframes)
        diff, maps = pl.delta_device(buf, nframes, gop)
        coded, sizes = pl.rice_pack_device(diff, nframes)
        torch.cuda.synchronize()
        path = str(tmp_path / "seq.csic")
        csic.write_container_coded(path, pl.c_params, coded.cpu().numpy(), sizes.cpu().numpy(), coding="rice", maps=maps.cpu().numpy(), gop=gop)
        host = str(tmp_path / "host.csic")
        csic.write_container(host, pl.c_params, buf.cpu().numpy(), coding="rice", gop=gop)
        assert open(path, "rb").read() == open(host, "rb").read()              # the host writer's file
        info = csic.container_info(path)
        assert (info.version, info.nframes, info.gop) == (5, nframes, gop)
        inter = csic.container_inter_groups(path)
        assert inter[0].sum() == 0 and inter[3].sum() == 0 and inter[1].sum() > 0
        _, n, back = csic.read_container(path)
        want = buf.cpu().numpy().copy()
        want[:, ~_payload_mask(pl.planar_bits_layout)] = 0
        assert n == nframes and np.array_equal(back, want)
        assert torch.equal(pl.decode_device(torch.from_numpy(back).cuda(), nframes=nframes), pl.decode_device(buf, nframes=nframes))


def test_capture_and_replay_in_a_graph(csic):
    """One linear capture of delta -> pack -> unpack -> undelta, replayed on new contents."""
    import torch
    n, bits, nframes, gop = 8193, (6, 5, 5), 5, 3
    rng = np.random.default_rng(16700)
    with _plan(csic, n, 1, 4, 4, bits) as pl:
        lay, ml = pl.planar_bits_layout, pl.delta_layout
        refs = [_reference(lay, ml.map_stride, _sequence(c, n, bits, rng), bits) for c in ("random", "alternating", "wrap")]
        src = torch.from_numpy(refs[0][0]).cuda()
        fb, ms, bound = pl.frame_bytes, ml.map_stride, pl.rice_layout.bound_bytes
        diff, maps, coded, undone, back = _filled((nframes, fb)), _filled((nframes, ms)), _filled((nframes, bound)), _filled((nframes, fb)), _filled((nframes, fb))

        def chain():
            pl.delta_device(src, nframes, gop, diff, maps)
            _, sizes = pl.rice_pack_device(diff, nframes, coded)
            pl.rice_unpack_device(coded, nframes, undone)
            pl.undelta_device(undone, maps, nframes, gop, back)
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
            assert np.array_equal(diff.cpu().numpy(), want_d) and np.array_equal(maps.cpu().numpy(), want_m)
            assert torch.equal(undone, diff) and torch.equal(back, src)


def test_refusals(csic):
    """All before any device is touched."""
    import torch
    L, N = csic._native.lib(), csic._native
    with _plan(csic, 64, 16, 2, 0, (6, 5, 5)) as pl:
        fb, ms = pl.frame_bytes, pl.delta_layout.map_stride
        frames = torch.zeros(4 * fb + 256, dtype=torch.uint8, device="cuda")
        diff = torch.zeros(3 * fb + 256, dtype=torch.uint8, device="cuda")
        maps = torch.zeros(3 * ms + 256, dtype=torch.uint8, device="cuda")
        s = pl._stream()
        ptr = lambda t, o=0: C.c_void_p(t.data_ptr() + o)

        def delta(n=3, gop=2, f=ptr(frames), d=ptr(diff), m=ptr(maps), plan=pl._h):
            return L.csic_delta_device(plan, f, n, gop, d, m, s)

        def undelta(n=3, gop=2, f=ptr(frames), d=ptr(diff), m=ptr(maps), plan=pl._h):
            return L.csic_undelta_device(plan, d, m, n, gop, f, s)
        nul = C.c_void_p(None)
        for call in (delta, undelta):
            assert call(plan=None) == N.EINVAL_NULL and call(f=nul) == N.EINVAL_NULL and call(d=nul) == N.EINVAL_NULL and call(m=nul) == N.EINVAL_NULL
            assert call(n=0) == N.EINVAL_SIZE and call(n=65536) == N.EINVAL_SIZE and call(gop=0) == N.EINVAL_SIZE and call(gop=-1) == N.EINVAL_SIZE
            assert call(f=ptr(frames, 64)) == N.EINVAL_SIZE and call(d=ptr(diff, 128)) == N.EINVAL_SIZE and call(m=ptr(maps, 4)) == N.EINVAL_SIZE
            assert call(d=ptr(frames, fb)) == N.EINVAL_SIZE                    # a partial overlap (frame_bytes is a multiple of 256)
            assert call(m=ptr(frames, 256)) == N.EINVAL_SIZE                   # the maps inside the frames
            assert L.csic_last_error().decode() != ""
            assert call() == N.OK and call(d=ptr(frames)) == N.OK and call(gop=100000) == N.OK      # apart; exactly in place; one key frame
        torch.cuda.synchronize()
        assert not frames.any() and not diff.any() and not maps.any()           # zeros: constant frames, every group a tie
        assert L.csic_delta_kernel_name(None) == b""
        with pytest.raises(csic.IllegalArgumentException):
            pl.delta_device(frames[:fb + 1])
        with pytest.raises(csic.IllegalArgumentException):
            pl.undelta_device(diff[:2 * fb].reshape(2, fb), None, 2, 2)
    # parameters the container does not take: a plan whose input is YCbCr
    cp = csic.make_c_params(64, 16, 2, 0, 6, 5, 5, 1, (3, 1, 2), in_format=N.FMT_YCBCR888X)
    with csic.Plan(cp, 0) as pl:
        z = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        assert L.csic_delta_device(pl._h, C.c_void_p(z.data_ptr()), 1, 1, C.c_void_p(z.data_ptr()), C.c_void_p(z.data_ptr() + 2048), pl._stream()) == N.EINVAL_FORMAT
