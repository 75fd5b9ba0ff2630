"""The group coding on the GPU (csic_pack_device, csic_unpack_device): every coded byte and every size equal to the numpy statement of
the format (tests/test_pack_host.py) on the oracle's planes, nothing written behind a frame's coded_bytes or outside the payload
ranges of a PLANAR_BITS frame; the smallest shapes that can go wrong, the block edge, a frame with more blocks than the scan has
threads, batches, graph capture, the host codec in both directions, the container and the CLI.  Source frames come from the library's
own PLANAR_BITS output into a buffer pre-filled with 0xEE, as are all destinations.  Planes built to order instead -- every width
w = 0 .. q of every q as the Y and as a chroma plane, whole blocks of one width and shuffled ones, all-zero blocks between full ones
(k_pack_emit, k_unpack_emit, pk_store_sections), groups stored wider than necessary into k_unpack_emit, and the cached instantiations
k_pack<.., cached> -- are uploaded by tests/test_gpu_codec_planes.py, which shares _compare below.  Run with `-m gpu` on an MI355X."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_container import CSQ, _frame_buffer, _random_sets
from test_pack_host import codes_of, plane_bytes, ref_encode, ref_groups

pytestmark = pytest.mark.gpu

EE = 0xEE
BITS = 3


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    assert csic_amd._native.lib().csic_device_count() >= 1
    return csic_amd


def _plan(csic, W, H, a=4, b=4, bits=(8, 8, 8), f=1, op=CSQ, rounding=0, avg=False):
    cp = csic.make_c_params(W, H, a, b, *bits, f, op, rounding=rounding, out_format=BITS, sampling=1 if avg else 0)
    return csic.Plan(cp, 0)


def _filled(shape):
    import torch
    return torch.full(shape, EE, dtype=torch.uint8, device="cuda:0")


def _source(pl, frames, nframes=1):
    """The library's PLANAR_BITS output of `frames` in a buffer pre-filled with 0xEE: uint8 (nframes, frame_bytes)."""
    import torch
    d_in = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint32).reshape(-1).view(np.int32)).cuda()
    return pl.process_device(d_in, _filled((nframes * pl.frame_bytes,)), nframes).reshape(nframes, pl.frame_bytes)


def _roundtrip(pl, buf, nframes=1):
    """pack then unpack on the device, every destination pre-filled: -> (coded, sizes, back) as numpy arrays."""
    import torch
    bound = pl.pack_layout.bound_bytes
    coded, sizes = pl.pack_device(buf, nframes, _filled((nframes, bound)))
    back = pl.unpack_device(coded, nframes, _filled((nframes, pl.frame_bytes)))
    torch.cuda.synchronize()
    return coded.cpu().numpy(), sizes.cpu().numpy(), back.cpu().numpy().reshape(nframes, -1)


def _compare(tag, lay, bits, planes, src, coded, sizes, back, bound, wants):
    """The comparison of both device codecs' tests (this module's, test_gpu_rice.py's and test_gpu_codec_planes.py's): frame k's source
    buffer src[k] holds planes[k] and 0xEE elsewhere, its coded row, size and the unpacked frame are the reference's, wants[k]."""
    for k, want in enumerate(wants):
        # the source itself: the planes in the payload ranges, 0xEE elsewhere
        assert np.array_equal(src[k], _frame_buffer(lay, [plane_bytes(c, q) for c, q in zip(planes[k], bits)], EE)), tag
        assert int(sizes[k]) == len(want), (tag, k, int(sizes[k]), len(want))
        assert coded[k, :len(want)].tobytes() == want, (tag, k)
        assert np.all(coded[k, len(want):] == EE), (tag, k)                # nothing behind coded_bytes, up to the next frame
        assert len(want) <= bound
    assert len(wants) == len(src) and np.array_equal(back, src), tag        # payload ranges restored, 0xEE everywhere else


def _check(csic, oracle, frames, W, H, a, b, bits, f=1, op=CSQ, rounding=0, avg=False):
    """`frames` (nframes, W * H) through the device codec against numpy.  Returns (the planes' codes per frame, the coded sizes)."""
    frames = np.ascontiguousarray(frames, dtype=np.uint32).reshape(-1, W * H)
    nframes = frames.shape[0]
    tag = (W, H, a, b, bits, f, op, rounding, avg)
    with _plan(csic, W, H, a, b, bits, f, op, rounding, avg) as pl:
        lay, bound = pl.planar_bits_layout, pl.pack_layout.bound_bytes
        buf = _source(pl, frames, nframes)
        coded, sizes, back = _roundtrip(pl, buf, nframes)
        src = buf.cpu().numpy()
        planes = [codes_of(oracle, W, H, a, b, bits, f, op, rounding, avg, fr) for fr in frames]
        _compare(tag, lay, bits, planes, src, coded, sizes, back, bound, [ref_encode(p, bits) for p in planes])
    return planes, sizes


def _mixed(rng, W, H):
    """Noise in the upper half, a slow ramp below: widths from 0 to q within one frame."""
    fr = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
    lo = (W * H) // 2
    ramp = (np.arange(W * H - lo, dtype=np.uint32) // 5) & np.uint32(0xFF)
    fr[lo:] = ramp * np.uint32(0x010101) | np.uint32(0xFF000000)
    return fr


# ---- random parameters -----------------------------------------------------------------------------
def test_random_sets_vs_numpy(csic, oracle):
    seen_q, seen_w = set(), set()
    for (W, H, a, b, bits, f, op, rounding, avg, nframes, rng) in _random_sets(40, 9600):
        frames = np.stack([_mixed(rng, W, H) if k % 2 else rng.integers(0, 1 << 32, W * H, dtype=np.uint32) for k in range(nframes)])
        planes, _ = _check(csic, oracle, frames, W, H, a, b, bits, f, op, rounding, avg)
        seen_q |= set(bits)
        for fr in planes:
            for c, q in zip(fr, bits):
                seen_w |= set(ref_groups(c, q)[0].tolist())
    assert seen_q == set(range(1, 9)) and seen_w >= set(range(1, 9))


# ---- the smallest shapes that can go wrong --------------------------------------------------------------
@pytest.mark.parametrize("W,H,a,b,f,op", [
    (1, 1, 4, 4, 1, CSQ),
    (4, 1, 1, 0, 1, CSQ),            # 4:1:0: one chroma sample
    (31, 1, 4, 4, 1, CSQ), (32, 1, 4, 4, 1, CSQ), (33, 1, 4, 4, 1, CSQ),
    (8160, 1, 4, 4, 1, CSQ), (8192, 1, 4, 4, 1, CSQ), (8224, 1, 4, 4, 1, CSQ),     # 255, 256, 257 groups: the block edge
    (13, 9, 2, 0, 1, CSQ),
    (30, 34, 2, 0, 4, (1, 3, 2)),    # spatial before chroma: the last chroma row is partial
])
def test_small_shapes_and_the_block_edge(csic, oracle, W, H, a, b, f, op):
    rng = np.random.default_rng(W * 100 + H + a)
    for bits in ((8, 8, 8), (6, 5, 5), (3, 3, 2), (1, 7, 4)):
        _check(csic, oracle, np.stack([rng.integers(0, 1 << 32, W * H, dtype=np.uint32), _mixed(rng, W, H)]), W, H, a, b, bits, f, op)
    if (W, H) == (30, 34):
        with _plan(csic, W, H, a, b, (6, 5, 5), f, op) as pl:
            g = pl.planar_layout
            assert g.chroma_samples < g.chroma_width * g.chroma_height
    if W in (8160, 8192, 8224):
        with _plan(csic, W, H, a, b) as pl:
            assert list(pl.pack_layout.groups) == [W // 32] * 3


def test_more_blocks_than_the_scan_has_threads(csic, oracle):
    """2048 x 1056 at 4:4:4, 8/8/8: 264 blocks of 256 groups per plane, 792 per frame -- the scan kernel loops."""
    W, H = 2048, 1056
    rng = np.random.default_rng(9700)
    with _plan(csic, W, H) as pl:
        assert pl.pack_workspace_bytes(1) == 4 * 3 * 264 and pl.pack_kernel_name == "k_pack<q8,8,8,nt>"
    _, sizes = _check(csic, oracle, _mixed(rng, W, H), W, H, 4, 4, (8, 8, 8))
    assert sizes[0] < 3 * W * H


def test_constant_and_noise_frames(csic, oracle):
    W, H = 300, 70
    rng = np.random.default_rng(9800)
    for bits in ((8, 8, 8), (6, 5, 5)):
        with _plan(csic, W, H, 2, 0, bits) as pl:
            fixed, bound = pl.pack_layout.fixed_bytes, pl.pack_layout.bound_bytes
        _, sizes = _check(csic, oracle, np.full(W * H, 0xFF4080C0, dtype=np.uint32), W, H, 2, 0, bits)
        assert sizes[0] == fixed                                            # every width 0
        _, sizes = _check(csic, oracle, rng.integers(0, 1 << 32, W * H, dtype=np.uint32), W, H, 2, 0, bits)
        assert fixed < sizes[0] <= bound


def test_batch_of_three_different_frames(csic, oracle):
    W, H, bits, f = 200, 72, (6, 5, 5), 2
    rng = np.random.default_rng(9900)
    frames = np.stack([np.full(W * H, 0xFF336699, dtype=np.uint32), _mixed(rng, W, H), rng.integers(0, 1 << 32, W * H, dtype=np.uint32)])
    _, sizes = _check(csic, oracle, frames, W, H, 2, 0, bits, f)             # frame k sits at k * bound_bytes: rows of `coded`
    assert sizes[0] < sizes[1] < sizes[2]


def test_capture_and_replay_in_a_graph(csic, oracle):
    import torch
    W, H, bits = 320, 240, (6, 5, 5)
    rng = np.random.default_rng(10000)
    frames = [_mixed(rng, W, H), rng.integers(0, 1 << 32, W * H, dtype=np.uint32), np.full(W * H, 0xFF102030, dtype=np.uint32)]
    wants = [ref_encode(codes_of(oracle, W, H, 2, 0, bits, 1, CSQ, 0, False, fr), bits) for fr in frames]
    with _plan(csic, W, H, 2, 0, bits) as pl:
        bufs = [_source(pl, fr) for fr in frames]
        src = bufs[0].clone()
        coded, back = _filled((1, pl.pack_layout.bound_bytes)), _filled((1, pl.frame_bytes))
        pl.unpack_device(pl.pack_device(src, 1, coded)[0], 1, back)              # the warm-up
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                _, sizes = pl.pack_device(src, 1, coded)
                pl.unpack_device(coded, 1, back)
        torch.cuda.current_stream().wait_stream(s)
        for k in (1, 2):                                                    # two replays, the input changed each time
            src.copy_(bufs[k])
            g.replay()
            torch.cuda.synchronize()
            assert int(sizes[0]) == len(wants[k])
            assert coded.cpu().numpy()[0, :len(wants[k])].tobytes() == wants[k]
            assert torch.equal(back, bufs[k])


# ---- device <-> host, the container, the CLI -------------------------------------------------------------
def test_device_and_host_codecs_read_each_other(csic, oracle):
    import torch
    W, H, bits = 150, 37, (7, 4, 2)
    rng = np.random.default_rng(10100)
    frame = _mixed(rng, W, H)
    with _plan(csic, W, H, 2, 2, bits) as pl:
        buf = _source(pl, frame)
        src = buf.cpu().numpy()[0]
        coded, sizes = pl.pack_device(buf)
        torch.cuda.synchronize()
        dev = coded.cpu().numpy()[0, :int(sizes[0])]
        host = pl.pack(src)
        assert np.array_equal(dev, host)
        # host unpack of the device's bytes: the planes, into a pre-filled buffer
        out = np.full(pl.frame_bytes, EE, dtype=np.uint8)
        assert np.array_equal(pl.unpack(dev, out), src)
        # device unpack of the host's bytes
        padded = np.full(pl.pack_layout.bound_bytes, EE, dtype=np.uint8)
        padded[:host.size] = host
        back = pl.unpack_device(torch.from_numpy(padded).cuda().reshape(1, -1), 1, _filled((1, pl.frame_bytes)))
        torch.cuda.synchronize()
        assert np.array_equal(back.cpu().numpy()[0], src)


def test_container_from_device_output_is_the_host_writers_file(csic, oracle, tmp_path):
    import torch
    W, H, bits = 96, 50, (6, 5, 5)
    rng = np.random.default_rng(10200)
    frames = np.stack([_mixed(rng, W, H), rng.integers(0, 1 << 32, W * H, dtype=np.uint32)])
    with _plan(csic, W, H, 2, 0, bits) as pl:
        buf = _source(pl, frames, 2)
        coded, sizes = pl.pack_device(buf, 2)
        torch.cuda.synchronize()
        a, b = str(tmp_path / "device.csic"), str(tmp_path / "host.csic")
        csic.write_container_coded(a, pl.c_params, coded.cpu().numpy(), sizes.cpu().numpy())
        csic.write_container(b, pl.c_params, buf.cpu().numpy(), coding="groups")
        assert open(a, "rb").read() == open(b, "rb").read()
        assert csic.container_coded_sizes(a).tolist() == [int(x) for x in sizes]
        _, n, back = csic.read_container(a)
        src = buf.cpu().numpy().copy()
        lay = pl.planar_bits_layout
        keep = np.zeros(lay.frame_bytes, dtype=bool)
        for off, nb in ((lay.y_offset, lay.y_bytes), (lay.cb_offset, lay.cb_bytes), (lay.cr_offset, lay.cr_bytes)):
            keep[off:off + nb] = True
        src[:, ~keep] = 0
        assert n == 2 and np.array_equal(back, src)


def test_cli_groups_coding(csic, tmp_path, capsys):
    png = os.path.join(GOLDEN, "inputs", "in512.png")
    common = ["--a", "2", "--b", "0", "--yq", "6", "--cbq", "5", "--crq", "5", "--sf", "1", "--op1", "chroma", "--op2", "spatial", "--op3", "color"]
    raw, grp = str(tmp_path / "raw.csic"), str(tmp_path / "groups.csic")
    assert csic.app.main(["compress", "--input", png, "--output", raw] + common) == 0
    assert csic.app.main(["compress", "--input", png, "--output", grp, "--coding", "groups"] + common) == 0
    assert csic.container_info(raw).version == 1 and csic.container_info(grp).version == 3
    assert os.path.getsize(grp) < os.path.getsize(raw)
    assert csic.app.main(["decompress", "--input", raw, "--output", str(tmp_path / "raw.png")]) == 0
    assert csic.app.main(["decompress", "--input", grp, "--output", str(tmp_path / "groups.png")]) == 0
    assert open(tmp_path / "raw.png", "rb").read() == open(tmp_path / "groups.png", "rb").read()
    capsys.readouterr()
    assert csic.app.main(["inspect", "--input", grp]) == 0
    text = capsys.readouterr().out
    assert "version 3" in text and "coding: groups" in text and f"{int(csic.container_coded_sizes(grp)[0])} bytes" in text


# ---- refusals (all before any device is touched) -----------------------------------------------------------
def test_refusals(csic):
    import torch
    L, N = csic._native.lib(), csic._native
    with _plan(csic, 64, 16, 2, 0, (6, 5, 5)) as pl:
        fb, bound, wsb = pl.frame_bytes, pl.pack_layout.bound_bytes, pl.pack_workspace_bytes(2)
        bits = torch.zeros(2 * fb + 256, dtype=torch.uint8, device="cuda")
        coded = torch.zeros(2 * bound + 256, dtype=torch.uint8, device="cuda")
        sizes = torch.zeros(4, dtype=torch.int64, device="cuda")
        ws = torch.zeros(wsb + 16, dtype=torch.uint8, device="cuda")
        s = pl._stream()

        def pack(n=2, b=0, c=0, z=0, w=0, wb=wsb, plan=pl._h):
            return L.csic_pack_device(plan, C.c_void_p(bits.data_ptr() + b), n, C.c_void_p(coded.data_ptr() + c), C.c_void_p(sizes.data_ptr() + z),
                                      C.c_void_p(ws.data_ptr() + w), wb, s)

        def unpack(n=2, b=0, c=0, w=0, wb=wsb, plan=pl._h):
            return L.csic_unpack_device(plan, C.c_void_p(coded.data_ptr() + c), n, C.c_void_p(bits.data_ptr() + b), C.c_void_p(ws.data_ptr() + w), wb, s)
        for call in (pack, unpack):
            assert call(n=0) == N.EINVAL_SIZE and call(n=65536) == N.EINVAL_SIZE
            assert call(b=64) == N.EINVAL_SIZE and call(c=128) == N.EINVAL_SIZE and call(w=4) == N.EINVAL_SIZE
            assert call(wb=wsb - 8) == N.EINVAL_SIZE
            assert call(plan=None) == N.EINVAL_NULL
        assert pack(z=4) == N.EINVAL_SIZE
        nul = C.c_void_p(None)
        assert L.csic_pack_device(pl._h, nul, 2, C.c_void_p(coded.data_ptr()), C.c_void_p(sizes.data_ptr()), C.c_void_p(ws.data_ptr()), wsb, s) == N.EINVAL_NULL
        assert L.csic_pack_device(pl._h, C.c_void_p(bits.data_ptr()), 2, nul, C.c_void_p(sizes.data_ptr()), C.c_void_p(ws.data_ptr()), wsb, s) == N.EINVAL_NULL
        assert L.csic_pack_device(pl._h, C.c_void_p(bits.data_ptr()), 2, C.c_void_p(coded.data_ptr()), nul, C.c_void_p(ws.data_ptr()), wsb, s) == N.EINVAL_NULL
        assert L.csic_pack_device(pl._h, C.c_void_p(bits.data_ptr()), 2, C.c_void_p(coded.data_ptr()), C.c_void_p(sizes.data_ptr()), nul, wsb, s) == N.EINVAL_NULL
        assert L.csic_unpack_device(pl._h, nul, 2, C.c_void_p(bits.data_ptr()), C.c_void_p(ws.data_ptr()), wsb, s) == N.EINVAL_NULL
        assert L.csic_unpack_device(pl._h, C.c_void_p(coded.data_ptr()), 2, nul, C.c_void_p(ws.data_ptr()), wsb, s) == N.EINVAL_NULL
        assert L.csic_pack_workspace_bytes(pl._h, 0, C.byref(C.c_size_t())) == N.EINVAL_SIZE
        assert L.csic_pack_workspace_bytes(None, 1, C.byref(C.c_size_t())) == N.EINVAL_NULL
        assert L.csic_pack_kernel_name(None) == b"" and pl.pack_kernel_name == "k_pack<q6,5,5,nt>"
        pl.tune(N.TUNE_NONTEMPORAL, 0)
        assert pl.pack_kernel_name == "k_pack<q6,5,5,cached>"
        pl.tune(N.TUNE_NONTEMPORAL, 1)
        assert pack() == N.OK and unpack(w=8, wb=wsb) == N.OK             # zeros: a constant frame, every width 0
        torch.cuda.synchronize()
        assert sizes[:2].tolist() == [pl.pack_layout.fixed_bytes] * 2
        with pytest.raises(csic.IllegalArgumentException):
            pl.pack_device(bits[:fb + 1])
        with pytest.raises(csic.IllegalArgumentException):
            pl.unpack_device(coded[:bound - 1])
