"""The Rice coding on the GPU (csic_rice_pack_device, csic_rice_unpack_device): every coded byte and every size equal to the numpy
statement of the format (tests/test_rice_host.py) on the oracle's planes, nothing written behind a frame's coded_bytes or outside the
payload ranges of a PLANAR_BITS frame, unpack restores the source; the shapes of tests/test_gpu_pack.py, a block in which zero, raw and
Rice groups interleave, a frame with more blocks than the scan has threads, batches, graph capture, the host codec in both directions,
the container and the CLI; random parameter sets (AVG sampling, rounding, f = 8, the six stage orders) on three kinds of content.
Sources and destinations are pre-filled with 0xEE.  No invalid stream is fed to the device (the clamping is shown on the host:
tests/test_cpp_rice.py).  Every source here is process_device's output, so which modes and runs the kernels meet follows from the colour
transform and the quantiser; tests/test_gpu_codec_planes.py uploads planes built to order instead, and is where to look for: every
(q, mode) pair in whole blocks and shuffled, with three different widths per frame (test_runs_and_shuffled_frames: the bit offsets
of RcWriter and its shared dwords); unary runs of 62 zeros and a dword of U without a terminator (test_long_unary_runs: the loop of
RcWriter::unary, the plateau of s_cum); chunks of exactly 248 q + 1 dwords around an empty one (test_full_and_empty_chunks: the last
element of s_chunk and s_cum); valid streams of another encoder -- mode q - 1, runs of up to 255 zeros -- into k_rice_unpack
(test_foreign_streams_unpack); the cached instantiations (test_cached_variants).  Run with `-m gpu` on an MI355X."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_container import CSQ, ORDERS, _random_sets
from test_gpu_pack import EE, _compare, _filled, _mixed, _plan, _source
from test_pack_host import codes_of, ref_groups
from test_rice_host import ref_encode_rice, ref_modes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    assert csic_amd._native.lib().csic_device_count() >= 1
    return csic_amd


def _roundtrip(pl, buf, nframes=1):
    """pack then unpack on the device, every destination pre-filled: -> (coded, sizes, back) as numpy arrays."""
    import torch
    bound = pl.rice_layout.bound_bytes
    coded, sizes = pl.rice_pack_device(buf, nframes, _filled((nframes, bound)))
    back = pl.rice_unpack_device(coded, nframes, _filled((nframes, pl.frame_bytes)))
    torch.cuda.synchronize()
    return coded.cpu().numpy(), sizes.cpu().numpy(), back.cpu().numpy().reshape(nframes, -1)


def _check(csic, oracle, frames, W, H, a, b, bits, f=1, op=CSQ, rounding=0, avg=False):
    """`frames` (nframes, W * H) through the device codec against numpy.  Returns (the planes' codes per frame, the coded sizes)."""
    frames = np.ascontiguousarray(frames, dtype=np.uint32).reshape(-1, W * H)
    nframes = frames.shape[0]
    tag = (W, H, a, b, bits, f, op, rounding, avg)
    with _plan(csic, W, H, a, b, bits, f, op, rounding, avg) as pl:
        lay, bound = pl.planar_bits_layout, pl.rice_layout.bound_bytes
        buf = _source(pl, frames, nframes)
        coded, sizes, back = _roundtrip(pl, buf, nframes)
        src = buf.cpu().numpy()
        planes = [codes_of(oracle, W, H, a, b, bits, f, op, rounding, avg, fr) for fr in frames]
        _compare(tag, lay, bits, planes, src, coded, sizes, back, bound, [ref_encode_rice(p, bits) for p in planes])
    return planes, sizes


# ---- random parameters -----------------------------------------------------------------------------
RANDOM_SEED = 12050


def _random_frames(seed=RANDOM_SEED, count=40):
    """The parameter sets of test_random_sets_vs_numpy with their frames: the three kinds of content of
    test_rice_host.test_random_sets_match_the_reference_byte_for_byte, in turn over the sets and over a batch's frames."""
    for i, (W, H, a, b, bits, f, op, rounding, avg, nframes, rng) in enumerate(_random_sets(count, seed)):
        frames = []
        for k in range(nframes):
            argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
            if (i + k) % 3 == 1:                              # smooth content: zero groups and small k
                argb = (np.arange(W * H, dtype=np.uint32) // 3 * np.uint32(0x010101)) | np.uint32(0xFF000000)
            elif (i + k) % 3 == 2:                            # a ramp with a few outliers: every k in between
                argb = (np.arange(W * H, dtype=np.uint32) // 2 * np.uint32(0x010101)) | np.uint32(0xFF000000)
                hit = rng.random(W * H) < 0.08
                argb[hit] = rng.integers(0, 1 << 32, int(hit.sum()), dtype=np.uint32)
            frames.append(argb)
        yield (W, H, a, b, bits, f, op, rounding, avg), np.stack(frames)


def test_random_sets_vs_numpy(csic, oracle):
    """40 random parameter sets -- the six modes of subsampling, f = 1, 2, 4, 8, the six stage orders, both roundings, AVG sampling,
    batches of 1 and 3 -- on noise, a smooth ramp and a ramp with 8 % outliers: every width and every mode that an encoder can emit."""
    seen_bits, seen_modes, seen = set(), set(), set()
    for (W, H, a, b, bits, f, op, rounding, avg), frames in _random_frames():
        planes, _ = _check(csic, oracle, frames, W, H, a, b, bits, f, op, rounding, avg)
        seen_bits |= set(bits)
        seen |= {("f", f), ("avg", avg), ("rounding", rounding), ("op", op), ("n", len(frames))}
        for fr in planes:
            for c, q in zip(fr, bits):
                seen_modes |= {(q, int(m)) for m in ref_modes(ref_groups(c, q)[2], q)}
    assert seen_bits == set(range(1, 9))
    assert {m for _, m in seen_modes} == set(range(0, 9)) | {15}
    assert seen_modes == {(q, m) for q in range(1, 9) for m in [15] + [k for k in range(q + 1) if k != q - 1]}      # with seed 12050: all
    assert seen >= {("f", 8), ("avg", True), ("rounding", 1), ("n", 1), ("n", 3)} | {("op", o) for o in ORDERS}


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
    if W in (8160, 8192, 8224):
        with _plan(csic, W, H, a, b) as pl:
            assert list(pl.rice_layout.groups) == [W // 32] * 3 and list(pl.rice_layout.blocks) == [(W // 32 + 255) // 256] * 3


def test_zero_raw_and_rice_groups_interleave_in_one_block(csic, oracle):
    """8192 x 2 at 4:4:4: two blocks per plane in which every even group is constant, every odd one noise or a slow ramp -- the unary
    groups before a group are not its lane number, so its terminator index is not 31 x lane."""
    W, H = 8192, 2
    rng = np.random.default_rng(12100)
    fr = np.zeros(W * H, dtype=np.uint32)
    for g in range(W * H // 32):
        if g % 2 == 0:
            fr[32 * g:32 * g + 32] = 0xFF000000 | (0x010101 * int(rng.integers(0, 256)))
        elif g % 4 == 1:
            fr[32 * g:32 * g + 32] = rng.integers(0, 1 << 32, 32, dtype=np.uint32)
        else:
            fr[32 * g:32 * g + 32] = 0xFF000000 | (np.uint32(0x010101) * ((int(rng.integers(0, 200)) + np.arange(32, dtype=np.uint32) // 3) & np.uint32(0xFF)))
    for bits in ((8, 8, 8), (6, 5, 5)):
        planes, _ = _check(csic, oracle, fr, W, H, 4, 4, bits)
        m = ref_modes(ref_groups(planes[0][0], bits[0])[2], bits[0])[:256]
        assert np.all(m[0::2] == 15) and {bits[0]} < set(m[1::2].tolist()) and 15 not in m[1::2].tolist()     # zero, raw and Rice groups


def test_more_blocks_than_the_scan_has_threads(csic, oracle):
    """2048 x 1056 at 4:4:4, 8/8/8: 264 blocks of 256 groups per plane, 792 per frame -- the scan kernel loops, the directory spans them."""
    W, H = 2048, 1056
    rng = np.random.default_rng(12200)
    with _plan(csic, W, H) as pl:
        assert pl.rice_workspace_bytes(1) == 4 * 3 * 264 and pl.rice_kernel_name == "k_rice<q8,8,8,nt>"
        assert list(pl.rice_layout.blocks) == [264] * 3
    _, sizes = _check(csic, oracle, _mixed(rng, W, H), W, H, 4, 4, (8, 8, 8))
    assert sizes[0] < 3 * W * H


def test_constant_and_noise_frames(csic, oracle):
    W, H = 300, 70
    rng = np.random.default_rng(12300)
    for bits in ((8, 8, 8), (6, 5, 5)):
        with _plan(csic, W, H, 2, 0, bits) as pl:
            rl = pl.rice_layout
            fixed, top = rl.fixed_bytes, rl.fixed_bytes + 4 * sum(b * (248 * q + 1) for b, q in zip(rl.blocks, bits))
        _, sizes = _check(csic, oracle, np.full(W * H, 0xFF4080C0, dtype=np.uint32), W, H, 2, 0, bits)
        assert sizes[0] == fixed                                            # every group in zero mode
        _, sizes = _check(csic, oracle, rng.integers(0, 1 << 32, W * H, dtype=np.uint32), W, H, 2, 0, bits)
        assert fixed < sizes[0] <= top


def test_batch_of_three_different_frames(csic, oracle):
    W, H, bits, f = 200, 72, (6, 5, 5), 2
    rng = np.random.default_rng(12400)
    frames = np.stack([np.full(W * H, 0xFF336699, dtype=np.uint32), _mixed(rng, W, H), rng.integers(0, 1 << 32, W * H, dtype=np.uint32)])
    _, sizes = _check(csic, oracle, frames, W, H, 2, 0, bits, f)             # frame k sits at k * bound_bytes: rows of `coded`
    assert sizes[0] < sizes[1] < sizes[2]


def test_capture_and_replay_in_a_graph(csic, oracle):
    import torch
    W, H, bits = 320, 240, (6, 5, 5)
    rng = np.random.default_rng(12500)
    frames = [_mixed(rng, W, H), rng.integers(0, 1 << 32, W * H, dtype=np.uint32), np.full(W * H, 0xFF102030, dtype=np.uint32)]
    wants = [ref_encode_rice(codes_of(oracle, W, H, 2, 0, bits, 1, CSQ, 0, False, fr), bits) for fr in frames]
    with _plan(csic, W, H, 2, 0, bits) as pl:
        bufs = [_source(pl, fr) for fr in frames]
        src = bufs[0].clone()
        coded, back = _filled((1, pl.rice_layout.bound_bytes)), _filled((1, pl.frame_bytes))
        pl.rice_unpack_device(pl.rice_pack_device(src, 1, coded)[0], 1, back)    # the warm-up
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                _, sizes = pl.rice_pack_device(src, 1, coded)
                pl.rice_unpack_device(coded, 1, back)
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
    rng = np.random.default_rng(12600)
    frame = _mixed(rng, W, H)
    with _plan(csic, W, H, 2, 2, bits) as pl:
        buf = _source(pl, frame)
        src = buf.cpu().numpy()[0]
        coded, sizes = pl.rice_pack_device(buf)
        torch.cuda.synchronize()
        dev = coded.cpu().numpy()[0, :int(sizes[0])]
        host = pl.rice_pack(src)
        assert np.array_equal(dev, host)
        out = np.full(pl.frame_bytes, EE, dtype=np.uint8)                  # host unpack of the device's bytes, into a pre-filled buffer
        assert np.array_equal(pl.rice_unpack(dev, out), src)
        padded = np.full(pl.rice_layout.bound_bytes, EE, dtype=np.uint8)   # device unpack of the host's bytes
        padded[:host.size] = host
        back = pl.rice_unpack_device(torch.from_numpy(padded).cuda().reshape(1, -1), 1, _filled((1, pl.frame_bytes)))
        torch.cuda.synchronize()
        assert np.array_equal(back.cpu().numpy()[0], src)


@pytest.mark.parametrize("bits", [(6, 5, 5), (1, 7, 4)])
@pytest.mark.parametrize("W", [33, 8224])
def test_both_device_codecs_store_the_same_anchors(csic, W, bits):
    """One random frame through both device codecs, which store a block's nibble and anchors sections with the same code: the nibble
    sections have the same extents, the anchors sections are the same bytes, and each coded frame is its host codec's."""
    import torch
    frame = np.random.default_rng(12650 + W + bits[0]).integers(0, 1 << 32, W, dtype=np.uint32)
    with _plan(csic, W, 1, 4, 4, bits) as pl:
        buf = _source(pl, frame)
        g, gs = pl.pack_device(buf, 1, _filled((1, pl.pack_layout.bound_bytes)))
        r, rs = pl.rice_pack_device(buf, 1, _filled((1, pl.rice_layout.bound_bytes)))
        torch.cuda.synchronize()
        src = buf.cpu().numpy()[0]
        g, r = g.cpu().numpy()[0, :int(gs[0])], r.cpu().numpy()[0, :int(rs[0])]
        pk, rl = pl.pack_layout, pl.rice_layout
        assert list(pk.widths_offset) + [pk.anchors_offset[0]] == list(rl.modes_offset) + [rl.anchors_offset[0]]
        assert list(pk.anchors_offset) + [pk.fixed_bytes] == list(rl.anchors_offset) + [rl.directory_offset]
        assert g[pk.anchors_offset[0]:pk.fixed_bytes].tobytes() == r[rl.anchors_offset[0]:rl.directory_offset].tobytes()
        assert np.array_equal(g, pl.pack(src)) and np.array_equal(r, pl.rice_pack(src))


def test_container_from_device_output_is_the_host_writers_file(csic, oracle, tmp_path):
    import torch
    W, H, bits = 96, 50, (6, 5, 5)
    rng = np.random.default_rng(12700)
    frames = np.stack([_mixed(rng, W, H), rng.integers(0, 1 << 32, W * H, dtype=np.uint32)])
    with _plan(csic, W, H, 2, 0, bits) as pl:
        buf = _source(pl, frames, 2)
        coded, sizes = pl.rice_pack_device(buf, 2)
        torch.cuda.synchronize()
        a, b = str(tmp_path / "device.csic"), str(tmp_path / "host.csic")
        csic.write_container_coded(a, pl.c_params, coded.cpu().numpy(), sizes.cpu().numpy(), coding="rice")
        csic.write_container(b, pl.c_params, buf.cpu().numpy(), coding="rice")
        assert open(a, "rb").read() == open(b, "rb").read()
        assert csic.container_info(a).version == 4 and csic.container_coded_sizes(a).tolist() == [int(x) for x in sizes]
        _, n, back = csic.read_container(a)
        src = buf.cpu().numpy().copy()
        lay = pl.planar_bits_layout
        keep = np.zeros(lay.frame_bytes, dtype=bool)
        for off, nb in ((lay.y_offset, lay.y_bytes), (lay.cb_offset, lay.cb_bytes), (lay.cr_offset, lay.cr_bytes)):
            keep[off:off + nb] = True
        src[:, ~keep] = 0
        assert n == 2 and np.array_equal(back, src)


def test_cli_rice_coding(csic, tmp_path, capsys):
    png = os.path.join(GOLDEN, "inputs", "in512.png")
    common = ["--a", "2", "--b", "0", "--yq", "6", "--cbq", "5", "--crq", "5", "--sf", "1", "--op1", "chroma", "--op2", "spatial", "--op3", "color"]
    raw, grp, rice = (str(tmp_path / n) for n in ("raw.csic", "groups.csic", "rice.csic"))
    assert csic.app.main(["compress", "--input", png, "--output", raw] + common) == 0
    assert csic.app.main(["compress", "--input", png, "--output", grp, "--coding", "groups"] + common) == 0
    assert csic.app.main(["compress", "--input", png, "--output", rice, "--coding", "rice"] + common) == 0
    assert csic.container_info(rice).version == 4
    assert os.path.getsize(rice) < os.path.getsize(grp) < os.path.getsize(raw)
    assert csic.app.main(["decompress", "--input", raw, "--output", str(tmp_path / "raw.png")]) == 0
    assert csic.app.main(["decompress", "--input", rice, "--output", str(tmp_path / "rice.png")]) == 0
    assert open(tmp_path / "raw.png", "rb").read() == open(tmp_path / "rice.png", "rb").read()
    capsys.readouterr()
    assert csic.app.main(["inspect", "--input", rice]) == 0
    text = capsys.readouterr().out
    assert "version 4" in text and "coding: rice" in text and f"{int(csic.container_coded_sizes(rice)[0])} bytes" in text


# ---- refusals (all before any device is touched) -----------------------------------------------------------
def test_refusals(csic):
    import torch
    L, N = csic._native.lib(), csic._native
    with _plan(csic, 64, 16, 2, 0, (6, 5, 5)) as pl:
        fb, bound, wsb = pl.frame_bytes, pl.rice_layout.bound_bytes, pl.rice_workspace_bytes(2)
        bits = torch.zeros(2 * fb + 256, dtype=torch.uint8, device="cuda")
        coded = torch.zeros(2 * bound + 256, dtype=torch.uint8, device="cuda")
        sizes = torch.zeros(4, dtype=torch.int64, device="cuda")
        ws = torch.zeros(wsb + 16, dtype=torch.uint8, device="cuda")
        s = pl._stream()

        def pack(n=2, b=0, c=0, z=0, w=0, wb=wsb, plan=pl._h):
            return L.csic_rice_pack_device(plan, C.c_void_p(bits.data_ptr() + b), n, C.c_void_p(coded.data_ptr() + c), C.c_void_p(sizes.data_ptr() + z),
                                           C.c_void_p(ws.data_ptr() + w), wb, s)

        def unpack(n=2, b=0, c=0, plan=pl._h):
            return L.csic_rice_unpack_device(plan, C.c_void_p(coded.data_ptr() + c), n, C.c_void_p(bits.data_ptr() + b), s)
        for call in (pack, unpack):
            assert call(n=0) == N.EINVAL_SIZE and call(n=65536) == N.EINVAL_SIZE
            assert call(b=64) == N.EINVAL_SIZE and call(c=128) == N.EINVAL_SIZE
            assert call(plan=None) == N.EINVAL_NULL
        assert pack(w=4) == N.EINVAL_SIZE and pack(wb=wsb - 8) == N.EINVAL_SIZE and pack(z=4) == N.EINVAL_SIZE
        nul = C.c_void_p(None)
        assert L.csic_rice_pack_device(pl._h, nul, 2, C.c_void_p(coded.data_ptr()), C.c_void_p(sizes.data_ptr()), C.c_void_p(ws.data_ptr()), wsb, s) == N.EINVAL_NULL
        assert L.csic_rice_pack_device(pl._h, C.c_void_p(bits.data_ptr()), 2, nul, C.c_void_p(sizes.data_ptr()), C.c_void_p(ws.data_ptr()), wsb, s) == N.EINVAL_NULL
        assert L.csic_rice_pack_device(pl._h, C.c_void_p(bits.data_ptr()), 2, C.c_void_p(coded.data_ptr()), nul, C.c_void_p(ws.data_ptr()), wsb, s) == N.EINVAL_NULL
        assert L.csic_rice_pack_device(pl._h, C.c_void_p(bits.data_ptr()), 2, C.c_void_p(coded.data_ptr()), C.c_void_p(sizes.data_ptr()), nul, wsb, s) == N.EINVAL_NULL
        assert L.csic_rice_unpack_device(pl._h, nul, 2, C.c_void_p(bits.data_ptr()), s) == N.EINVAL_NULL
        assert L.csic_rice_unpack_device(pl._h, C.c_void_p(coded.data_ptr()), 2, nul, s) == N.EINVAL_NULL
        assert L.csic_rice_workspace_bytes(pl._h, 0, C.byref(C.c_size_t())) == N.EINVAL_SIZE
        assert L.csic_rice_workspace_bytes(None, 1, C.byref(C.c_size_t())) == N.EINVAL_NULL
        assert L.csic_rice_kernel_name(None) == b"" and pl.rice_kernel_name == "k_rice<q6,5,5,nt>"
        pl.tune(N.TUNE_NONTEMPORAL, 0)
        assert pl.rice_kernel_name == "k_rice<q6,5,5,cached>"
        pl.tune(N.TUNE_NONTEMPORAL, 1)
        assert pack() == N.OK                                              # zeros: a constant frame, every group in zero mode
        assert unpack() == N.OK
        torch.cuda.synchronize()
        assert sizes[:2].tolist() == [pl.rice_layout.fixed_bytes] * 2
        with pytest.raises(csic.IllegalArgumentException):
            pl.rice_pack_device(bits[:fb + 1])
        with pytest.raises(csic.IllegalArgumentException):
            pl.rice_unpack_device(coded[:bound - 1])
