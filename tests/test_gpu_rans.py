"""The rANS coding on the GPU (csic_rans_pack_device, csic_rans_unpack_device): every coded byte and every size equal to the numpy
statement of the format (tests/test_rans_host.py) and to the host codec, nothing written behind a frame's coded_bytes or outside the
payload ranges of a PLANAR_BITS frame, unpack restores the source, and each codec reads the other's output.  The PLANAR_BITS frames are
built on the host from planes of codes and uploaded, so what the kernels see does not depend on the colour transform: the group, lane
and block edges (1, 63 .. 65, 1023 .. 1025 groups), every bit width, a frame with more blocks than the scan has threads, the planes
built to order of tests/rans_planes.py, batches, graph capture, the container and the CLI.  Sources and destinations are pre-filled
with 0xEE.  No invalid stream is fed to the device (the clamping is shown on the host: tests/test_cpp_rans.py).  Run with `-m gpu` on
an MI355X."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from rans_planes import built_planes
from test_container import _frame_buffer
from test_gpu_pack import EE, _filled, _plan
from test_pack_host import plane_bytes
from test_rans_host import BLOCK, ref_encode_rans

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    assert csic_amd._native.lib().csic_device_count() >= 1
    return csic_amd


def _upload(pl, frames, bits):
    """Frames of three planes of codes each -> their PLANAR_BITS buffers on the device, 0xEE between the planes: (nframes, frame_bytes)."""
    import torch
    lay = pl.planar_bits_layout
    host = np.stack([_frame_buffer(lay, [plane_bytes(c, q) for c, q in zip(planes, bits)], EE) for planes in frames])
    return torch.from_numpy(host).cuda(), host


def _check(csic, frames, n, bits, wants=None, W=None, H=1):
    """`frames` -- three planes of n codes each per frame, an n x 1 plan at 4:4:4 (or W x H = n) -- through the device codec against the
    numpy statement and the host codec, in both directions.  -> the coded sizes."""
    import torch
    wants = [ref_encode_rans(planes, bits) for planes in frames] if wants is None else wants
    nframes = len(frames)
    with _plan(csic, n if W is None else W, H, 4, 4, bits) as pl:
        bound = pl.rans_layout.bound_bytes
        buf, src = _upload(pl, frames, bits)
        coded, sizes = pl.rans_pack_device(buf, nframes, _filled((nframes, bound)))
        back = pl.rans_unpack_device(coded, nframes, _filled((nframes, pl.frame_bytes)))
        torch.cuda.synchronize()
        coded, sizes, back = coded.cpu().numpy(), sizes.cpu().numpy(), back.cpu().numpy().reshape(nframes, -1)
        for k, want in enumerate(wants):
            assert int(sizes[k]) == len(want) <= bound, (n, bits, k, int(sizes[k]), len(want))
            assert coded[k, :len(want)].tobytes() == want, (n, bits, k)
            assert np.all(coded[k, len(want):] == EE), (n, bits, k)       # nothing behind coded_bytes, up to the next frame
            assert pl.rans_pack(src[k]).tobytes() == want                   # the host codec writes the same bytes
            out = np.full(pl.frame_bytes, EE, dtype=np.uint8)
            assert np.array_equal(pl.rans_unpack(coded[k, :len(want)], out), src[k])      # and reads the device's
        assert np.array_equal(back, src), (n, bits)                         # payload ranges restored, 0xEE everywhere else
    return sizes


def _walk(rng, n, q, step=1):
    return (np.cumsum(rng.integers(-step, step + 1, n)) % (1 << q)).astype(np.int64)


def _two_frames(rng, n, bits):
    """noise, and a slow walk with a stretch of noise: skewed tables, rANS and raw chunks"""
    noise = [rng.integers(0, 1 << q, n).astype(np.int64) for q in bits]
    walk = [_walk(rng, n, q) for q in bits]
    for c, q in zip(walk, bits):
        c[n // 2:n // 2 + n // 7] = rng.integers(0, 1 << q, n // 7)
    return [noise, walk]


# ---- the group, lane and block edges ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 32 * 63, 32 * 63 + 1, 32 * 65 - 9, 32 * 1023, 32 * 1024, 32 * 1024 + 1, 32 * 1025 + 17])
def test_group_lane_and_block_edges(csic, n):
    rng = np.random.default_rng(22000 + n)
    for bits in ((8, 8, 8), (6, 5, 5), (1, 7, 4)):
        _check(csic, _two_frames(rng, n, bits), n, bits)
    with _plan(csic, n, 1, 4, 4, (6, 5, 5)) as pl:
        groups = (n + 31) // 32
        assert list(pl.rans_layout.groups) == [groups] * 3 and list(pl.rans_layout.blocks) == [(groups + BLOCK - 1) // BLOCK] * 3


@pytest.mark.parametrize("q", range(1, 9))
def test_every_bit_width(csic, q):
    rng = np.random.default_rng(22100 + q)
    n = 32 * 1100 - 5                                                       # two blocks per plane, the last group ragged
    _check(csic, _two_frames(rng, n, (q, q, q)) + [[_walk(rng, n, q, 3) for _ in range(3)]], n, (q, q, q))


def test_more_blocks_than_the_scan_has_threads(csic):
    """8192 x 1025 at 4:4:4, 2/2/2: 257 blocks of 1024 groups per plane, 771 per frame -- the scan kernel loops, the directory spans them."""
    W, H, bits = 8192, 1025, (2, 2, 2)
    rng = np.random.default_rng(22200)
    plane = np.where(rng.random(W * H) < 0.1, 1, 0).cumsum() % 4
    plane[W * 300:W * 301] = rng.integers(0, 4, W)                         # some raw blocks in between
    with _plan(csic, W, H, 4, 4, bits) as pl:
        assert list(pl.rans_layout.blocks) == [257] * 3 and pl.rans_kernel_name == "k_rans<q2,2,2,nt>"
        assert pl.rans_workspace_bytes(1) == 4 * (2 * 771 + 768)
    want = ref_encode_rans([plane] * 3, bits)
    sizes = _check(csic, [[plane] * 3], W * H, bits, [want], W, H)
    assert sizes[0] < 3 * W * H // 8


# ---- planes built to order -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(built_planes()))
def test_built_planes(csic, name):
    """Each plane of tests/rans_planes.py (conditions: tests/test_rans_planes_host.py) as the Y plane, as a chroma plane and in all three."""
    q, codes = built_planes()[name]
    rng = np.random.default_rng(22300 + q)
    qo = 4 if q == 3 else 3
    other = rng.integers(0, 1 << qo, codes.size).astype(np.int64)
    _check(csic, [[codes, other, other]], codes.size, (q, qo, qo))
    _check(csic, [[other, codes, codes]], codes.size, (qo, q, q))
    _check(csic, [[codes] * 3], codes.size, (q, q, q))


# ---- launch forms ----------------------------------------------------------------------------------------------
def test_batch_of_three_different_frames(csic):
    n, bits = 32 * 1040 + 3, (6, 5, 5)
    rng = np.random.default_rng(22400)
    frames = [[np.full(n, 3, dtype=np.int64)] * 3] + _two_frames(rng, n, bits)[::-1]
    sizes = _check(csic, frames, n, bits)                                   # frame k sits at k * bound_bytes: rows of `coded`
    assert sizes[0] < sizes[1] < sizes[2]


def test_capture_and_replay_in_a_graph(csic):
    import torch
    n, bits = 32 * 1040 + 3, (6, 5, 5)
    rng = np.random.default_rng(22500)
    frames = _two_frames(rng, n, bits) + [[np.full(n, 1, dtype=np.int64)] * 3]
    wants = [ref_encode_rans(planes, bits) for planes in frames]
    with _plan(csic, n, 1, 4, 4, bits) as pl:
        bufs, _ = _upload(pl, frames, bits)
        src = bufs[0:1].clone()
        coded, back = _filled((1, pl.rans_layout.bound_bytes)), _filled((1, pl.frame_bytes))
        pl.rans_unpack_device(pl.rans_pack_device(src, 1, coded)[0], 1, back)    # the warm-up
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                _, sizes = pl.rans_pack_device(src, 1, coded)
                pl.rans_unpack_device(coded, 1, back)
        torch.cuda.current_stream().wait_stream(s)
        for k in (1, 2):                                                    # two replays, the input changed each time
            src.copy_(bufs[k:k + 1])
            g.replay()
            torch.cuda.synchronize()
            assert int(sizes[0]) == len(wants[k])
            assert coded.cpu().numpy()[0, :len(wants[k])].tobytes() == wants[k]
            assert torch.equal(back, bufs[k:k + 1])


# ---- device <-> host, the other coders ------------------------------------------------------------------------
def test_device_reads_the_host_codecs_output(csic):
    import torch
    n, bits = 32 * 1030 - 11, (7, 4, 2)
    rng = np.random.default_rng(22600)
    with _plan(csic, n, 1, 4, 4, bits) as pl:
        buf, src = _upload(pl, _two_frames(rng, n, bits)[1:], bits)
        host = pl.rans_pack(src[0])
        padded = np.full(pl.rans_layout.bound_bytes, EE, dtype=np.uint8)
        padded[:host.size] = host
        back = pl.rans_unpack_device(torch.from_numpy(padded).cuda().reshape(1, -1), 1, _filled((1, pl.frame_bytes)))
        torch.cuda.synchronize()
        assert np.array_equal(back.cpu().numpy()[0], src[0])


@pytest.mark.parametrize("bits", [(6, 5, 5), (1, 7, 4)])
@pytest.mark.parametrize("n", [33, 8224])
def test_all_three_device_codecs_store_the_same_anchors(csic, n, bits):
    """One random frame through the three device codecs: the anchors sections are the same bytes."""
    import torch
    rng = np.random.default_rng(22650 + n + bits[0])
    with _plan(csic, n, 1, 4, 4, bits) as pl:
        buf, src = _upload(pl, [[rng.integers(0, 1 << q, n).astype(np.int64) for q in bits]], bits)
        g, gs = pl.pack_device(buf, 1, _filled((1, pl.pack_layout.bound_bytes)))
        r, rs = pl.rice_pack_device(buf, 1, _filled((1, pl.rice_layout.bound_bytes)))
        x, xs = pl.rans_pack_device(buf, 1, _filled((1, pl.rans_layout.bound_bytes)))
        torch.cuda.synchronize()
        g, r, x = g.cpu().numpy()[0], r.cpu().numpy()[0], x.cpu().numpy()[0]
        pk, rl, xl = pl.pack_layout, pl.rice_layout, pl.rans_layout
        anchors = g[pk.anchors_offset[0]:pk.fixed_bytes].tobytes()
        assert r[rl.anchors_offset[0]:rl.directory_offset].tobytes() == anchors
        assert x[xl.anchors_offset[0]:xl.directory_offset].tobytes() == anchors
        assert np.array_equal(x[:int(xs[0])], pl.rans_pack(src[0]))


# ---- the container, the CLI --------------------------------------------------------------------------------
def test_container_from_device_output_is_the_host_writers_file(csic, tmp_path):
    import torch
    n, bits = 32 * 1030 - 11, (6, 5, 5)
    rng = np.random.default_rng(22700)
    with _plan(csic, n, 1, 4, 4, bits) as pl:
        buf, src = _upload(pl, _two_frames(rng, n, bits), bits)
        coded, sizes = pl.rans_pack_device(buf, 2)
        torch.cuda.synchronize()
        a, b = str(tmp_path / "device.csic"), str(tmp_path / "host.csic")
        csic.write_container_coded(a, pl.c_params, coded.cpu().numpy(), sizes.cpu().numpy(), coding="rans")
        csic.write_container(b, pl.c_params, src, coding="rans")
        assert open(a, "rb").read() == open(b, "rb").read()
        assert csic.container_info(a).version == 7 and csic.container_coded_sizes(a).tolist() == [int(x) for x in sizes]
        _, nframes, back = csic.read_container(a)
        lay = pl.planar_bits_layout
        keep = np.zeros(lay.frame_bytes, dtype=bool)
        for off, nb in ((lay.y_offset, lay.y_bytes), (lay.cb_offset, lay.cb_bytes), (lay.cr_offset, lay.cr_bytes)):
            keep[off:off + nb] = True
        want = src.copy()
        want[:, ~keep] = 0
        assert nframes == 2 and np.array_equal(back, want)


COMMON = ["--a", "2", "--b", "0", "--yq", "6", "--cbq", "5", "--crq", "5", "--sf", "1", "--op1", "chroma", "--op2", "spatial", "--op3", "color"]


def test_cli_rans_coding(csic, tmp_path, capsys):
    png = os.path.join(GOLDEN, "inputs", "in512.png")
    raw, rice, rans = (str(tmp_path / n) for n in ("raw.csic", "rice.csic", "rans.csic"))
    assert csic.app.main(["compress", "--input", png, "--output", raw] + COMMON) == 0
    assert csic.app.main(["compress", "--input", png, "--output", rice, "--coding", "rice"] + COMMON) == 0
    assert csic.app.main(["compress", "--input", png, "--output", rans, "--coding", "rans"] + COMMON) == 0
    assert csic.container_info(rans).version == 7
    assert os.path.getsize(rans) < os.path.getsize(rice) < os.path.getsize(raw)
    assert csic.app.main(["decompress", "--input", raw, "--output", str(tmp_path / "raw.png")]) == 0
    assert csic.app.main(["decompress", "--input", rans, "--output", str(tmp_path / "rans.png")]) == 0
    assert open(tmp_path / "raw.png", "rb").read() == open(tmp_path / "rans.png", "rb").read()
    capsys.readouterr()
    assert csic.app.main(["inspect", "--input", rans]) == 0
    text = capsys.readouterr().out
    assert "version 7" in text and "coding: rans" in text and f"{int(csic.container_coded_sizes(rans)[0])} bytes" in text
    assert "frame 0, Y: 0 of 8 blocks raw" in text


@pytest.mark.parametrize("motion", [None, 2])
def test_cli_rans_sequence(csic, tmp_path, motion):
    """compress --inputs ... --gop 3 [--motion 2] --coding rans writes the host writer's file; decompress --frame gives, for every frame,
    the PNG of the single-frame path."""
    from PIL import Image
    from conftest import load_png_rgb
    rgb = load_png_rgb(os.path.join(GOLDEN, "inputs", "in512.png"))
    pngs = []
    for k in range(3):
        pngs.append(str(tmp_path / f"in{k}.png"))
        Image.fromarray(np.roll(rgb, (k, 2 * k), axis=(0, 1))).save(pngs[-1])
    layer = ["--gop", "3"] + ([] if motion is None else ["--motion", str(motion)])
    seq = str(tmp_path / "seq.csic")
    assert csic.app.main(["compress", "--inputs", ",".join(pngs), "--coding", "rans", "--output", seq] + layer + COMMON) == 0
    info = csic.container_info(seq)
    assert (info.version, info.nframes, info.gop, info.motion) == (7, 3, 3, -1 if motion is None else motion)
    host = str(tmp_path / "host.csic")
    csic.write_container(host, info.params, csic.read_container(seq)[2], coding="rans", gop=3, motion=motion)
    assert open(host, "rb").read() == open(seq, "rb").read()                   # the device's file is the host writer's
    singles = 0
    for k, png in enumerate(pngs):
        one, out, single = str(tmp_path / "one.csic"), str(tmp_path / "frame.png"), str(tmp_path / "single.png")
        assert csic.app.main(["compress", "--input", png, "--output", one, "--coding", "rans"] + COMMON) == 0
        assert csic.app.main(["decompress", "--input", one, "--output", single]) == 0
        singles += os.path.getsize(one)
        assert csic.app.main(["decompress", "--input", seq, "--output", out, "--frame", str(k)]) == 0
        assert open(out, "rb").read() == open(single, "rb").read()
    if motion is not None:
        assert os.path.getsize(seq) < singles                                  # a pan: the motion layer finds it


# ---- refusals (all before any device is touched) -----------------------------------------------------------
def test_refusals(csic):
    import torch
    L, N = csic._native.lib(), csic._native
    with _plan(csic, 64, 16, 2, 0, (6, 5, 5)) as pl:
        fb, bound, wsb = pl.frame_bytes, pl.rans_layout.bound_bytes, pl.rans_workspace_bytes(2)
        bits = torch.zeros(2 * fb + 256, dtype=torch.uint8, device="cuda")
        coded = torch.zeros(2 * bound + 256, dtype=torch.uint8, device="cuda")
        sizes = torch.zeros(4, dtype=torch.int64, device="cuda")
        ws = torch.zeros(wsb + 16, dtype=torch.uint8, device="cuda")
        s = pl._stream()

        def pack(n=2, b=0, c=0, z=0, w=0, wb=wsb, plan=pl._h):
            return L.csic_rans_pack_device(plan, C.c_void_p(bits.data_ptr() + b), n, C.c_void_p(coded.data_ptr() + c), C.c_void_p(sizes.data_ptr() + z),
                                           C.c_void_p(ws.data_ptr() + w), wb, s)

        def unpack(n=2, b=0, c=0, plan=pl._h):
            return L.csic_rans_unpack_device(plan, C.c_void_p(coded.data_ptr() + c), n, C.c_void_p(bits.data_ptr() + b), s)
        for call in (pack, unpack):
            assert call(n=0) == N.EINVAL_SIZE and call(n=65536) == N.EINVAL_SIZE
            assert call(b=64) == N.EINVAL_SIZE and call(c=128) == N.EINVAL_SIZE
            assert call(plan=None) == N.EINVAL_NULL
        assert pack(w=4) == N.EINVAL_SIZE and pack(wb=wsb - 8) == N.EINVAL_SIZE and pack(z=4) == N.EINVAL_SIZE
        nul = C.c_void_p(None)
        assert L.csic_rans_pack_device(pl._h, nul, 2, C.c_void_p(coded.data_ptr()), C.c_void_p(sizes.data_ptr()), C.c_void_p(ws.data_ptr()), wsb, s) == N.EINVAL_NULL
        assert L.csic_rans_pack_device(pl._h, C.c_void_p(bits.data_ptr()), 2, nul, C.c_void_p(sizes.data_ptr()), C.c_void_p(ws.data_ptr()), wsb, s) == N.EINVAL_NULL
        assert L.csic_rans_pack_device(pl._h, C.c_void_p(bits.data_ptr()), 2, C.c_void_p(coded.data_ptr()), nul, C.c_void_p(ws.data_ptr()), wsb, s) == N.EINVAL_NULL
        assert L.csic_rans_pack_device(pl._h, C.c_void_p(bits.data_ptr()), 2, C.c_void_p(coded.data_ptr()), C.c_void_p(sizes.data_ptr()), nul, wsb, s) == N.EINVAL_NULL
        assert L.csic_rans_unpack_device(pl._h, nul, 2, C.c_void_p(bits.data_ptr()), s) == N.EINVAL_NULL
        assert L.csic_rans_unpack_device(pl._h, C.c_void_p(coded.data_ptr()), 2, nul, s) == N.EINVAL_NULL
        assert L.csic_rans_workspace_bytes(pl._h, 0, C.byref(C.c_size_t())) == N.EINVAL_SIZE
        assert L.csic_rans_workspace_bytes(None, 1, C.byref(C.c_size_t())) == N.EINVAL_NULL
        assert L.csic_rans_kernel_name(None) == b"" and pl.rans_kernel_name == "k_rans<q6,5,5,nt>"
        pl.tune(N.TUNE_NONTEMPORAL, 0)
        assert pl.rans_kernel_name == "k_rans<q6,5,5,cached>"
        assert pack() == N.OK                                              # zeros: a constant frame, the cached instantiations
        pl.tune(N.TUNE_NONTEMPORAL, 1)
        assert unpack() == N.OK
        torch.cuda.synchronize()
        rl = pl.rans_layout
        assert sizes[:2].tolist() == [rl.fixed_bytes + 4 * sum(min(g, 64) for g in rl.groups)] * 2       # a chunk is its states
        with pytest.raises(csic.IllegalArgumentException):
            pl.rans_pack_device(bits[:fb + 1])
        with pytest.raises(csic.IllegalArgumentException):
            pl.rans_unpack_device(coded[:bound - 1])
