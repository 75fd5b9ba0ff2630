"""Code statistics on the GPU (csic_code_stats_*): every count equal, exactly, to the numpy statement of the definition
(tests/test_code_stats_host.py) on the oracle's planes, from the library's own PLANAR and PLANAR_BITS output of the same frame; the
fast kernels against the general one; the smallest shapes that can go wrong, block boundaries, a constant frame, batches, graph
capture, the host paths, the reference's images and the refusals.  Run with `-m gpu` on an MI355X."""
import ctypes as C
import itertools

import numpy as np
import pytest

from test_code_stats_host import oracle_code_stats, plane_hists
from plane_frames import _frame_from_codes, pack_codes

pytestmark = pytest.mark.gpu

ORDERS = list(itertools.permutations((1, 2, 3)))
CSQ = (3, 1, 2)
CHROMA = [(4, 4), (2, 2), (2, 0), (1, 1), (4, 0), (1, 0)]
PLANAR, BITS = 2, 3


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    assert csic_amd._native.lib().csic_device_count() >= 1
    return csic_amd


def _plan(csic, W, H, a=4, b=4, bits=(8, 8, 8), f=1, op=CSQ, rounding=0, avg=False, fmt=BITS):
    cp = csic.make_c_params(W, H, a, b, *bits, f, op, rounding=rounding, out_format=fmt, sampling=1 if avg else 0)
    return csic.Plan(cp, 0)


def _to_device(frames):
    import torch
    return torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint32).reshape(-1).view(np.int32)).cuda()


def _stats(pl, d_src, fmt=None, nframes=1):
    """counts of nframes compressed frames on the device -> uint64 (nframes, 2, 3, 256)"""
    import torch
    out = pl.code_stats_device(d_src, fmt, nframes)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


def _fast_and_general(csic, pl, d_src, fmt=None, nframes=1):
    """The plan's own kernel, then the general one on the same buffer: ((name, counts), (name, counts))."""
    N = csic._native
    fast = (pl.code_stats_kernel_name(fmt), _stats(pl, d_src, fmt, nframes))
    pl.tune(N.TUNE_FORCE_GENERIC, 1)
    gen = (pl.code_stats_kernel_name(fmt), _stats(pl, d_src, fmt, nframes))
    pl.tune(N.TUNE_FORCE_GENERIC, 0)
    assert gen[0].startswith("k_cstat_gen") and not fast[0].startswith("k_cstat_gen")
    return fast, gen


def _check_frame(csic, oracle, frame, W, H, a, b, bits, f, op, rounding, avg, fill=None):
    """Compresses `frame` to both formats on the device and holds every kernel's counts against numpy.  Returns the kernel names."""
    import torch
    want = oracle_code_stats(oracle, frame, W, H, a, b, bits, f, op, rounding, avg)
    d_in = _to_device(frame)
    names = set()
    for fmt in (PLANAR, BITS):
        with _plan(csic, W, H, a, b, bits, f, op, rounding, avg, fmt) as pl:
            d_out = None if fill is None else torch.full((pl.frame_bytes,), fill, dtype=torch.uint8, device="cuda:0")
            buf = pl.process_device(d_in, d_out)
            for name, got in _fast_and_general(csic, pl, buf):
                names.add(name.split("<")[0])
                assert np.array_equal(got[0], want), (name, W, H, a, b, bits, f, op, rounding, avg)
    return names


# ---- random parameters, all three kernels, against numpy-from-oracle ---------------------------
@pytest.mark.parametrize("seed", range(3))
def test_random_shapes_vs_numpy(csic, oracle, seed):
    rng = np.random.default_rng(9500 + seed)
    names, seen_bits, seen_f = set(), set(), set()
    for i in range(40):
        W, H = int(rng.integers(4, 91)), int(rng.integers(1, 41))
        a, b = CHROMA[i % 6]
        bits = tuple(int(x) for x in rng.integers(1, 9, 3))
        f = int(rng.choice([1, 2, 4, 8]))
        avg = rng.random() < 0.3
        op = CSQ if avg else ORDERS[int(rng.integers(0, 6))]
        rounding = int(rng.integers(0, 2))
        frame = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        names |= _check_frame(csic, oracle, frame, W, H, a, b, bits, f, op, rounding, avg)
        seen_bits |= set(bits)
        seen_f.add(f)
    assert names == {"k_cstat_bytes", "k_cstat_bits", "k_cstat_gen"}
    assert seen_bits == set(range(1, 9)) and seen_f == {1, 2, 4, 8}


# ---- the smallest shapes that can go wrong -----------------------------------------------------
@pytest.mark.parametrize("W,H,a,b,f,op", [
    (13, 9, 2, 0, 1, CSQ),          # every plane shorter than a lane's 16 samples or no multiple of 16 / 32
    (13, 9, 4, 4, 1, CSQ),
    (1, 1, 4, 4, 1, CSQ),
    (4, 1, 1, 0, 1, CSQ),           # 4:1:0: one chroma sample
    (33, 1, 2, 2, 1, CSQ),          # one sample past a whole group
])
def test_small_shapes(csic, oracle, W, H, a, b, f, op):
    rng = np.random.default_rng(W * 100 + H + a)
    for bits in ((8, 8, 8), (6, 5, 5), (3, 3, 2), (1, 7, 4)):
        _check_frame(csic, oracle, rng.integers(0, 1 << 32, W * H, dtype=np.uint32), W, H, a, b, bits, f, op, 0, False)


@pytest.mark.parametrize("W,H,a,b,partial", [(30, 14, 2, 0, False), (30, 34, 2, 0, True), (30, 14, 2, 2, True)])
def test_unwritten_tail_of_a_partial_chroma_row_is_not_counted(csic, oracle, W, H, a, b, partial):
    """Factor 4, spatial before chroma: the chroma counters wrap at the full width, so the last chroma row can be partial
    (chroma_samples < chroma_width * chroma_height) and what lies behind it in the plane is never written: 0xFF here, as is every
    other byte the format does not own.  30 x 14 at 4:2:0 ends in a row without samples (8 x 4 = 32 positions: 30 in chroma row 0,
    2 in the odd row 1), so its planes are whole; 30 x 34 at 4:2:0 (72 positions: 12 in the even row 2, 21 samples of 30) and
    30 x 14 at 4:2:2 (16 samples of 30) do end in a partial one."""
    f, op = 4, (1, 3, 2)
    rng = np.random.default_rng(3000 + H + a + b)
    with _plan(csic, W, H, a, b, (6, 5, 5), f, op) as pl:
        g = pl.planar_layout
        assert (g.chroma_samples < g.chroma_width * g.chroma_height) == partial
    for bits in ((8, 8, 8), (6, 5, 5), (7, 3, 1)):
        _check_frame(csic, oracle, rng.integers(0, 1 << 32, W * H, dtype=np.uint32), W, H, a, b, bits, f, op, 0, False, fill=0xFF)


@pytest.mark.parametrize("q", range(1, 9))
def test_every_bit_width_on_a_ragged_plane(csic, oracle, q):
    """67 x 5 = 335 samples in bits form: 10 whole groups of 32 and a ragged one, codes straddling dwords for every q that does not
    divide 32; the chroma planes take two other widths."""
    W, H = 67, 5
    rng = np.random.default_rng(670 + q)
    bits = (q, q % 8 + 1, (q + 3) % 8 + 1)
    _check_frame(csic, oracle, rng.integers(0, 1 << 32, W * H, dtype=np.uint32), W, H, 4, 4, bits, 1, CSQ, 0, False)


# ---- block boundaries: the predecessor across lanes, waves and blocks --------------------------------
@pytest.mark.parametrize("fmt", [PLANAR, BITS])
@pytest.mark.parametrize("bits", [(8, 8, 8), (6, 5, 5), (3, 7, 1)])
def test_block_boundaries(csic, oracle, fmt, bits):
    """A Y plane of 3 * block_samples + 37 samples (335 x 587 at the shipped block size): three whole blocks of the straight-line body
    and a ragged fourth.  A ramp c_i = i mod 2^q has a single residual bin apart from e_0 -- one wrong predecessor anywhere moves a
    count -- and random content is held against numpy; both as hand-made frames and as the library's own output."""
    import torch
    with _plan(csic, 16, 16, fmt=fmt) as probe:
        block = probe.code_stats_block_samples(fmt)
    n = 3 * block + 37
    W = next(w for w in range(300, 2000) if n % w == 0)
    H = n // W
    rng = np.random.default_rng(sum(bits) + fmt)
    with _plan(csic, W, H, 4, 4, bits, fmt=fmt) as pl:
        assert pl.planar_layout.y_width * pl.planar_layout.y_height == n and pl.planar_layout.chroma_samples == n
        i = np.arange(n, dtype=np.int64)
        ramp = [i % (1 << q) for q in bits]
        noise = [rng.integers(0, 1 << q, n) for q in bits]
        for planes in (ramp, noise):
            want = np.stack([np.stack(x) for x in zip(*[plane_hists(c, q) for c, q in zip(planes, bits)])])
            d_src = torch.from_numpy(_frame_from_codes(csic, pl, fmt, planes, bits)).cuda()
            for name, got in _fast_and_general(csic, pl, d_src, fmt):
                assert np.array_equal(got[0], want), name
        for p, q in enumerate(bits):                                  # the ramp: e_0 = 0, every other residual 1
            h1 = plane_hists(ramp[p], q)[1]
            assert h1[0] == 1 and h1[1] == n - 1
        frame = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        want = oracle_code_stats(oracle, frame, W, H, 4, 4, bits)
        buf = pl.process_device(_to_device(frame))
        for name, got in _fast_and_general(csic, pl, buf):
            assert np.array_equal(got[0], want), name


def test_constant_frame(csic, oracle):
    """Every count in one bin -- all 64 lanes of every LDS atomic on one address -- and still exact: h0 = {c: n}, h1 = {c: 1, 0: n - 1}."""
    W, H, bits = 512, 300, (8, 7, 5)                                   # 153 600 samples: two whole blocks and a part
    frame = np.full(W * H, 0xFF4080C0, dtype=np.uint32)
    want = oracle_code_stats(oracle, frame, W, H, 2, 0, bits)
    for p, n in enumerate((W * H, W * H // 4, W * H // 4)):
        c = int(np.flatnonzero(want[0, p])[0])
        assert c != 0 and want[0, p, c] == n and want[1, p, c] == 1 and want[1, p, 0] == n - 1
        assert np.count_nonzero(want[0, p]) == 1 and np.count_nonzero(want[1, p]) == 2
    for fmt in (PLANAR, BITS):
        with _plan(csic, W, H, 2, 0, bits, fmt=fmt) as pl:
            buf = pl.process_device(_to_device(frame))
            for name, got in _fast_and_general(csic, pl, buf):
                assert np.array_equal(got[0], want), name


# ---- batches, graph capture, the host paths ------------------------------------------------------
@pytest.mark.parametrize("fmt", [PLANAR, BITS])
def test_batch_of_three_different_frames(csic, oracle, fmt):
    W, H, bits, f = 100, 36, (6, 5, 5), 2
    rng = np.random.default_rng(1003)
    frames = np.stack([rng.integers(0, 1 << 32, W * H, dtype=np.uint32), np.full(W * H, 0xFF336699, dtype=np.uint32),
                       (np.arange(W * H, dtype=np.uint32) * np.uint32(2654435761)) | np.uint32(0xFF000000)])
    want = np.stack([oracle_code_stats(oracle, fr, W, H, 2, 0, bits, f) for fr in frames])
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[0], want[2])
    with _plan(csic, W, H, 2, 0, bits, f, fmt=fmt) as pl:
        buf = pl.process_device(_to_device(frames), nframes=3)
        assert buf.shape == (3, pl.frame_bytes)
        for name, got in _fast_and_general(csic, pl, buf, nframes=3):
            assert np.array_equal(got, want), name
        for k in range(3):
            assert np.array_equal(_stats(pl, buf[k])[0], want[k])
        host = pl.code_stats_host(buf.cpu().numpy(), nframes=3)
        assert host.dtype == np.uint64 and np.array_equal(host, want)
        ss = pl.code_stats(buf, nframes=3)
        g = pl.planar_layout
        assert [s.samples for s in ss] == [(g.y_width * g.y_height, g.chroma_samples, g.chroma_samples)] * 3
        assert ss[1].bits_per_pixel("best") == 0.0 and ss[0].bits_per_pixel("best") > 1.0
        assert all(np.array_equal(s.hist, w) for s, w in zip(ss, want))


def test_capture_and_replay_in_a_graph(csic, oracle):
    """The memset that clears d_hist is part of the capture: a replay gives the counts again, not twice the counts."""
    import torch
    W, H, bits = 320, 240, (6, 5, 5)
    rng = np.random.default_rng(77)
    frames = rng.integers(0, 1 << 32, (2, W * H), dtype=np.uint32)
    want = np.stack([oracle_code_stats(oracle, fr, W, H, 2, 0, bits) for fr in frames])
    with _plan(csic, W, H, 2, 0, bits) as pl:
        buf = pl.process_device(_to_device(frames), nframes=2)
        assert np.array_equal(_stats(pl, buf, nframes=2), want)          # the warm-up
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                out = pl.code_stats_device(buf, nframes=2)
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(2):
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint64), want)


def test_host_and_python_paths_agree_with_the_device(csic, oracle):
    W, H, bits, f = 100, 60, (6, 5, 5), 2
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 1 << 32, (H, W), dtype=np.uint32)
    want = oracle_code_stats(oracle, frame, W, H, 2, 0, bits, f)
    top = csic.ImageCompressorTop(W, H, 2, 0, *bits, f, csic.ProcessingStep.ChromaSubsampling, csic.ProcessingStep.SpatialSampling,
                                  csic.ProcessingStep.ColorQuantization)
    try:
        pl = top.plan(csic.PixelFormat.PLANAR_BITS)
        buf = pl.process_device(_to_device(frame))                    # the two-step path
        dev = _stats(pl, buf)[0]
        assert np.array_equal(dev, want)
        assert np.array_equal(pl.code_stats_host(buf.cpu().numpy())[0], dev)
        two_step = pl.code_stats(buf)
        s = top.codeStats(_to_device(frame).reshape(H, W))             # compress and measure on the device
        assert isinstance(s, csic.CodeStats) and s == two_step and np.array_equal(s.hist, want)
        assert top.codeStats(frame) == s                               # numpy in: the host entry points
        g = pl.planar_layout
        assert s.samples == (50 * 30, g.chroma_samples, g.chroma_samples) and s.bits == bits and s.pixels == W * H
        assert s.raw_bits_per_pixel == (1500 * 6 + g.chroma_samples * 10) / 6000
        # a PLANAR frame of the same parameters gives the same counts through a plan of any out_format
        with _plan(csic, W, H, 2, 0, bits, f, fmt=PLANAR) as pp:
            assert np.array_equal(_stats(pl, pp.process_device(_to_device(frame)), PLANAR)[0], want)
    finally:
        top.close()


# ---- the reference's images --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["in16", "in128", "in512"])
@pytest.mark.parametrize("bits", [(6, 5, 5), (3, 3, 2)], ids=["Q16bit", "Q8bit"])
def test_golden_inputs(csic, oracle, input_images, name, bits):
    rgb = input_images[name]
    H, W = rgb.shape[:2]
    frame = oracle.rgb_to_argb(rgb).reshape(-1)
    names = _check_frame(csic, oracle, frame, W, H, 2, 0, bits, 1, CSQ, 0, False)
    assert names == {"k_cstat_bytes", "k_cstat_bits", "k_cstat_gen"}


def test_headline_plan_kernel_names(csic):
    """8192 x 8192 at 4:2:0: names only, no launch."""
    N = csic._native
    with _plan(csic, 8192, 8192, 2, 0, (6, 5, 5), fmt=0) as pl:
        assert pl.code_stats_kernel_name(PLANAR) == "k_cstat_bytes<nt>"
        assert pl.code_stats_kernel_name(BITS) == "k_cstat_bits<q6,5,5,nt>"
        assert pl.code_stats_block_samples(PLANAR) == pl.code_stats_block_samples(BITS) > 0
        pl.tune(N.TUNE_NONTEMPORAL, 0)
        assert pl.code_stats_kernel_name(PLANAR) == "k_cstat_bytes<cached>"
        pl.tune(N.TUNE_NONTEMPORAL, 1)
        pl.tune(N.TUNE_VARIANT, 9)
        assert pl.code_stats_kernel_name(PLANAR) == "k_cstat_gen<planar>" and pl.code_stats_kernel_name(BITS) == "k_cstat_gen<bits>"
        pl.tune(N.TUNE_VARIANT, 0)
        pl.tune(N.TUNE_NO_VECTOR, 1)
        assert pl.code_stats_kernel_name(PLANAR) == "k_cstat_gen<planar>" and pl.code_stats_kernel_name(BITS).startswith("k_cstat_bits<q6")
        with pytest.raises(csic.IllegalArgumentException):
            pl.code_stats_kernel_name(0)                            # the plan's own format is packed ARGB
    with _plan(csic, 8192, 8192, 2, 0, (8, 8, 8), fmt=BITS) as pl:
        assert pl.code_stats_kernel_name() == "k_cstat_bits<q8,8,8,nt>"


# ---- refusals ----------------------------------------------------------------------------------
def test_refusals(csic):
    import torch
    L, N = csic._native.lib(), csic._native
    W, H = 64, 16
    with _plan(csic, W, H, 2, 0, (6, 5, 5)) as pl:
        fb = pl.frame_bytes
        src = torch.zeros(2 * fb + 256, dtype=torch.uint8, device="cuda")
        hist = torch.zeros(2 * 1536 + 2, dtype=torch.int64, device="cuda")
        s = pl._stream()

        def call(fmt=BITS, n=2, src_off=0, hist_off=0):
            return L.csic_code_stats_device(pl._h, C.c_void_p(src.data_ptr() + src_off), fmt, n, C.c_void_p(hist.data_ptr() + hist_off), s)
        assert src.data_ptr() % 256 == 0
        assert call(n=0) == N.EINVAL_SIZE and call(n=65536) == N.EINVAL_SIZE
        assert call(src_off=64) == N.EINVAL_SIZE and call(hist_off=4) == N.EINVAL_SIZE
        assert call(fmt=0) == N.EINVAL_FORMAT and call(fmt=1) == N.EINVAL_FORMAT and call(fmt=4) == N.EINVAL_FORMAT
        assert L.csic_code_stats_device(pl._h, None, BITS, 2, C.c_void_p(hist.data_ptr()), s) == N.EINVAL_NULL
        assert L.csic_code_stats_device(pl._h, C.c_void_p(src.data_ptr()), BITS, 2, None, s) == N.EINVAL_NULL
        assert call() == N.OK and call(hist_off=8) == N.OK
        torch.cuda.synchronize()
        assert int(hist[1:1 + 256].sum()) == W * H                   # zeros are code 0 of every sample
        with pytest.raises(csic.IllegalArgumentException) as ei:
            pl.code_stats_host(np.zeros(fb + 1, dtype=np.uint8))
        assert ei.value.status == N.EINVAL_SIZE
        with pytest.raises(csic.IllegalArgumentException):
            pl.code_stats_device(src[:fb + 1])
        with pytest.raises(csic.IllegalArgumentException) as ei:
            pl.code_stats_device(src[:fb], 1)
        assert ei.value.status == N.EINVAL_FORMAT
