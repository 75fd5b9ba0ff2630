"""The quantiser sweep on the GPU (csic_qsweep_*): every sum equal, exactly, to csic_distortion_device of the plan with that width
(identity A) and every histogram to kind 1 of csic_code_stats_device on that plan's PLANAR output (identity B), and both equal to a
numpy closed form on the oracle's 8/8/8 outputs, so that a mistake the units share cannot hide; the histogram kernel alone on planes
built to order; batches, graph capture, the host paths, the refusals; and `compress --target-bytes` end to end against the procedure
run in numpy.  Run with `-m gpu` on an MI355X."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import measure_frames as mf
import plane_frames as pf
from conftest import GOLDEN
from test_code_stats_host import oracle_planes, plane_hists
from test_distortion_host import forward, oracle_params, unpack
from test_qsweep_host import rank_numpy

pytestmark = pytest.mark.gpu

ORDERS = list(itertools.permutations((1, 2, 3)))
CSQ, SCQ = (3, 1, 2), (1, 3, 2)
CHROMA4 = [(4, 4), (2, 2), (2, 0), (1, 1)]
CHROMA6 = CHROMA4 + [(4, 0), (1, 0)]
PLANAR = 2
WORDS = 24 + 24 * 256
CANARY = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    assert csic_amd._native.lib().csic_device_count() >= 1
    return csic_amd


def _plan(csic, W, H, a=4, b=4, bits=(6, 5, 5), f=1, op=CSQ, rounding=0, avg=False, fmt=0):
    return csic.Plan(csic.make_c_params(W, H, a, b, *bits, f, op, rounding=rounding, out_format=fmt, sampling=1 if avg else 0), 0)


def _to_device(frames):
    import torch
    return torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint32).reshape(-1).view(np.int32)).cuda()


def _split(res):
    """(n, 6168) words -> (sse (n, 3, 8), hist (n, 3, 8, 256)) uint64"""
    r = np.ascontiguousarray(res).view(np.uint64).reshape(-1, WORDS)
    return r[:, :24].reshape(-1, 3, 8), r[:, 24:].reshape(-1, 3, 8, 256)


def _sweep(pl, d_in, n):
    import torch
    out = pl.qsweep_device(d_in, n)
    torch.cuda.synchronize()
    return _split(out.cpu().numpy())


def three_frames(W, H, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, 1 << 32, W * H, dtype=np.uint32), np.zeros(W * H, dtype=np.uint32), np.full(W * H, 0xFFFFFFFF, dtype=np.uint32)])


# ---- the closed form: the oracle's 8/8/8 outputs, cut to every width in numpy ------------------------
def numpy_sweep(orc, frame, W, H, a, b, f, op, rounding, avg):
    frame = np.asarray(frame, dtype=np.uint32).reshape(H, W)
    o_ycc = orc.process(oracle_params(orc, W, H, a, b, (8, 8, 8), f, op, rounding, orc.FMT_YCC), frame.reshape(-1), form="avg" if avg else "stream")
    rows, cols = np.arange(H) // f, np.arange(W) // f
    ocr, ocb, oy = unpack(np.asarray(o_ycc, dtype=np.uint32)[rows[:, None], cols[None, :]])
    planes = oracle_planes(orc, frame, W, H, a, b, (8, 8, 8), f, op, rounding, avg)
    sse, hist = np.zeros((3, 8), dtype=np.uint64), np.zeros((3, 8, 256), dtype=np.uint64)
    for p, (ref, out) in enumerate(zip(forward(frame, rounding), (oy, ocb, ocr))):
        for q in range(1, 9):
            sse[p, q - 1] = int(((ref - (out & (0xFF00 >> q & 0xFF))) ** 2).sum())
            hist[p, q - 1] = plane_hists(np.asarray(planes[p], dtype=np.uint8).reshape(-1) >> (8 - q), q)[1]
    return sse, hist


def check_identities(csic, orc, frames, W, H, a, b, f, op, rounding, avg, d_in=None, numpy_too=True):
    """Sweeps `frames` (n, W * H) in one call and holds it against the two units width by width, and against numpy.  Returns the
    sweep's kernel name."""
    import torch
    n = len(frames)
    d_in = _to_device(frames) if d_in is None else d_in
    with _plan(csic, W, H, a, b, (6, 5, 5), f, op, rounding, avg) as pl:
        name = pl.qsweep_kernel_name
        sse, hist = _sweep(pl, d_in, n)
    where = (name, W, H, a, b, f, op, rounding, avg)
    for q in range(1, 9):
        with _plan(csic, W, H, a, b, (q, q, q), f, op, rounding, avg, PLANAR) as pq:
            dist = pq.distortion_device(d_in, n)
            stats = pq.code_stats_device(pq.process_device(d_in, None, n), PLANAR, n)
            torch.cuda.synchronize()
            assert np.array_equal(sse[:, :, q - 1], dist.cpu().numpy().view(np.uint64)[:, 3:]), ("A", q) + where
            assert np.array_equal(hist[:, :, q - 1], stats.cpu().numpy().view(np.uint64)[:, 1]), ("B", q) + where
    assert not hist[:, :, 0, 2:].any() and not hist[:, :, 4, 32:].any()
    if numpy_too:
        for k in range(n):
            want_sse, want_hist = numpy_sweep(orc, frames[k], W, H, a, b, f, op, rounding, avg)
            assert np.array_equal(sse[k], want_sse) and np.array_equal(hist[k], want_hist), ("numpy", k) + where
    return name


# ---- identities A and B -------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,f", [(64, 8, 1), (1028, 4, 1), (72, 6, 2)])
def test_fast_kernel_shapes(csic, oracle, W, H, f):
    """64 x 8 and 1028 x 4 at factor 1: 4:x:0 odd rows, and 1028 units against the 1024 of a block; 72 x 6 at factor 2: one partial
    block.  A d_in that is only 4-byte aligned takes the 4-byte loads."""
    import torch
    frames = three_frames(W, H, 100 * W + f)
    for (a, b), rounding in itertools.product(CHROMA6, (0, 1)):
        assert check_identities(csic, oracle, frames, W, H, a, b, f, CSQ, rounding, False) == f"k_qsweep_sse_fast<f{f}>"
    shifted = torch.zeros(frames.size + 1, dtype=torch.int32, device="cuda")
    shifted[1:] = _to_device(frames)
    assert shifted[1:].data_ptr() % 16 == 4
    assert check_identities(csic, oracle, frames, W, H, 2, 0, f, CSQ, 0, False, d_in=shifted[1:]) == f"k_qsweep_sse_fast<f{f}>"
    with _plan(csic, W, H, 2, 0, f=f) as pl:                      # the general kernel on a fast plan's shape
        pl.tune(csic._native.TUNE_FORCE_GENERIC, 1)
        assert pl.qsweep_kernel_name == "k_qsweep_sse_gen<hold>"
        got = _sweep(pl, _to_device(frames), 3)
        pl.tune(csic._native.TUNE_FORCE_GENERIC, 0)
        want = _sweep(pl, _to_device(frames), 3)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("a,b", CHROMA4)
@pytest.mark.parametrize("f", [2, 4, 8])
def test_general_kernel_all_orders(csic, oracle, f, a, b):
    """33 x 17: ragged on both edges at every factor; all six orders, both roundings, and AVG."""
    W, H = 33, 17
    frames = three_frames(W, H, 33 * f + a + b)
    for op, rounding in itertools.product(ORDERS, (0, 1)):
        assert check_identities(csic, oracle, frames, W, H, a, b, f, op, rounding, False) == "k_qsweep_sse_gen<hold>"
    for rounding in (0, 1):
        assert check_identities(csic, oracle, frames, W, H, a, b, f, CSQ, rounding, True) == "k_qsweep_sse_gen<avg>"


@pytest.mark.parametrize("f", [1, 2, 4])
def test_built_frames_against_numpy(csic, oracle, f):
    """The palette and gray mosaics of tests/measure_frames.py: near-maximal chroma contrast inside and across the hold groups, and
    a luma that sits on both sides of every mask."""
    W, H = 40, 104
    for lever, names in (("palette", mf.PALETTE_SET), ("gray", mf.RECIPE_SETS[8])):
        frames, _ = mf.build_frames(lever, names, f, W, H)
        frames = frames.reshape(len(frames), -1)[:4]
        for (a, b), op in (((2, 0), CSQ), ((1, 0), SCQ), ((2, 2), CSQ)):
            check_identities(csic, oracle, frames, W, H, a, b, f, op, 0, False)
        check_identities(csic, oracle, frames, W, H, 2, 0, f, CSQ, 1, True)


def test_the_plans_own_widths_and_format_do_not_matter(csic):
    W, H = 64, 24
    frames = three_frames(W, H, 5)
    d_in = _to_device(frames)
    got = []
    for bits, fmt in (((8, 8, 8), 0), ((1, 1, 1), 1), ((3, 7, 2), 2), ((6, 5, 5), 3)):
        with _plan(csic, W, H, 2, 0, bits, 2, fmt=fmt) as pl:
            got.append(_sweep(pl, d_in, 3))
    assert all(np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1]) for g in got[1:])
    assert got[0][0][1, :, 7].tolist() == [0, 0, 0]                  # a black frame is kept exactly at 8 bits


# ---- csic_qsweep_hist_device on planes built to order --------------------------------------------------
def _want_hist(planes):
    out = np.zeros((3, 8, 256), dtype=np.uint64)
    for p, v in enumerate(planes):
        for q in range(1, 9):
            out[p, q - 1] = plane_hists(np.asarray(v, dtype=np.uint8).reshape(-1) >> (8 - q), q)[1]
    return out


def _hist_of(pl, buf, n=1, d_result=None):
    import torch
    out = pl.qsweep_hist_device(torch.from_numpy(np.ascontiguousarray(buf)).cuda(), n, d_result)
    torch.cuda.synchronize()
    return _split(out.cpu().numpy())


@pytest.mark.parametrize("which", ["B-1", "B", "B+1", "2B+17"])
def test_hist_kernel_on_built_planes(csic, which):
    """Planes of B - 1, B, B + 1 and 2 B + 17 samples (B = csic_qsweep_block_samples): a constant, a ramp (every 8-bit residual 1), a
    falling ramp (every 8-bit residual wraps to 255) and random bytes -- junk below every width under 8."""
    with _plan(csic, 16, 16) as probe:
        B = probe.qsweep_block_samples
    assert B == 65536
    W, H = {"B-1": (255, 257), "B": (256, 256), "B+1": (65537, 1), "2B+17": (427, 307)}[which]
    n = {"B-1": B - 1, "B": B, "B+1": B + 1, "2B+17": 2 * B + 17}[which]
    assert W * H == n
    rng = np.random.default_rng(n)
    i = np.arange(n, dtype=np.int64)
    with _plan(csic, W, H, 4, 4, (8, 8, 8)) as pl:
        assert pf.sample_counts(pl) == (n, n, n)
        sets = [(np.full(n, 0xB7), i % 256, (-i) % 256), (rng.integers(0, 256, n), (i * 7) % 256, np.full(n, 0))]
        for planes in sets:
            want = _want_hist(planes)
            for fill in (0x00, 0xFF):
                sse, hist = _hist_of(pl, pf.frame_of(pl, PLANAR, *planes, fill))
                assert np.array_equal(hist[0], want), (which, fill)
                assert not sse.any()                                 # a fresh result is zeroed, and sse is left alone
        ramp = _want_hist(sets[0])
        assert ramp[1, 7, 1] == n - 1 and ramp[1, 7, 0] == 1 and ramp[2, 7, 255] == n - 1 and ramp[0, 7, 0] == n - 1
        assert ramp[1, 0, 0] == n - (n - 1) // 128 and ramp[0, 0, 1] == 1


def test_hist_kernel_does_not_count_the_tail_of_a_partial_chroma_row(csic):
    """30 x 34 at 4:2:0, factor 4, spatial before chroma: the last chroma row holds 21 samples of 30 (tests/test_gpu_code_stats.py);
    what lies behind them is a canary here, 0xFF or random, and must not reach a bin.  sse keeps what it held."""
    import torch
    W, H, f, op = 30, 34, 4, SCQ
    with _plan(csic, W, H, 2, 0, (8, 8, 8), f, op) as pl:
        g = pl.planar_layout
        assert g.chroma_samples < g.chroma_width * g.chroma_height
        planes = pf.random_planes(pl, 11)
        want = _want_hist(planes)
        for fill in (0xFF, 0x00, np.random.default_rng(1)):
            res = torch.full((1, WORDS), CANARY, dtype=torch.int64, device="cuda")
            sse, hist = _hist_of(pl, pf.frame_of(pl, PLANAR, *planes, fill), 1, res)
            assert np.array_equal(hist[0], want)
            assert (sse == np.uint64(CANARY)).all()
        assert int(want[1, 7].sum()) == g.chroma_samples and int(want[0, 0].sum()) == g.y_width * g.y_height


# ---- batches, graph capture, the host paths ------------------------------------------------------
def test_batch_of_three_different_frames(csic, oracle):
    W, H, f = 100, 36, 2
    rng = np.random.default_rng(1003)
    frames = np.stack([rng.integers(0, 1 << 32, W * H, dtype=np.uint32), np.full(W * H, 0xFF336699, dtype=np.uint32),
                       (np.arange(W * H, dtype=np.uint32) * np.uint32(2654435761)) | np.uint32(0xFF000000)])
    want = [numpy_sweep(oracle, fr, W, H, 2, 0, f, CSQ, 0, False) for fr in frames]
    with _plan(csic, W, H, 2, 0, f=f) as pl:
        d_in = _to_device(frames)
        sse, hist = _sweep(pl, d_in, 3)
        for k in range(3):
            assert np.array_equal(sse[k], want[k][0]) and np.array_equal(hist[k], want[k][1])
            one = _sweep(pl, d_in[k * W * H:(k + 1) * W * H], 1)
            assert np.array_equal(one[0][0], sse[k]) and np.array_equal(one[1][0], hist[k])
        assert not np.array_equal(hist[0], hist[1]) and not np.array_equal(hist[0], hist[2])
        # a constant frame: one residual bin per plane and width apart from e_0, and no error at 8 bits
        assert sse[1, :, 7].tolist() == [0, 0, 0] and all(np.count_nonzero(hist[1, p, q]) <= 2 for p in range(3) for q in range(8))


def test_capture_and_replay_in_a_graph(csic, oracle):
    """The kernel that clears hist is part of the capture: a replay over a result filled with a canary gives the counts again, not
    twice the counts and not the canary."""
    import torch
    W, H = 320, 240
    rng = np.random.default_rng(77)
    frames = rng.integers(0, 1 << 32, (2, W * H), dtype=np.uint32)
    want = [numpy_sweep(oracle, fr, W, H, 2, 0, 1, CSQ, 0, False) for fr in frames]
    with _plan(csic, W, H, 2, 0) as pl:
        d_in = _to_device(frames)
        warm = _sweep(pl, d_in, 2)                                   # allocates the plan's workspace
        assert all(np.array_equal(warm[0][k], want[k][0]) and np.array_equal(warm[1][k], want[k][1]) for k in range(2))
        res = torch.full((2, WORDS), CANARY, dtype=torch.int64, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                pl.qsweep_device(d_in, 2, res)
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(2):
            res.fill_(CANARY)
            g.replay()
            torch.cuda.synchronize()
            sse, hist = _split(res.cpu().numpy())
            assert all(np.array_equal(sse[k], want[k][0]) and np.array_equal(hist[k], want[k][1]) for k in range(2))


def test_host_and_python_paths_agree_with_the_device(csic, oracle):
    W, H, f = 100, 60, 2
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 1 << 32, (H, W), dtype=np.uint32)
    want = numpy_sweep(oracle, frame, W, H, 2, 0, f, CSQ, 0, False)
    top = csic.ImageCompressorTop(W, H, 2, 0, 6, 5, 5, f, csic.ProcessingStep.ChromaSubsampling, csic.ProcessingStep.SpatialSampling,
                                  csic.ProcessingStep.ColorQuantization)
    try:
        pl = top.plan()
        dev = _sweep(pl, _to_device(frame), 1)
        assert np.array_equal(dev[0][0], want[0]) and np.array_equal(dev[1][0], want[1])
        host = _split(pl.qsweep_host(frame))
        assert np.array_equal(host[0], dev[0]) and np.array_equal(host[1], dev[1])
        s = top.qsweep(frame)                                          # numpy in: csic_qsweep_host
        t = top.qsweep(_to_device(frame).reshape(H, W))                # a CUDA tensor: csic_qsweep_device
        assert isinstance(s, csic.QSweep) and np.array_equal(s.sse, want[0]) and np.array_equal(s.hist, want[1])
        assert np.array_equal(t.sse, s.sse) and np.array_equal(t.hist, s.hist) and s.nframes == 1 and s.pixels == W * H
        # the table against the units it replaces, through the Python layer
        with _plan(csic, W, H, 2, 0, (3, 4, 2), f) as p342:
            d = p342.distortion(frame)
            assert (int(s.sse[0, 2]), int(s.sse[1, 3]), int(s.sse[2, 1])) == d.sse[3:]
            assert s.psnr("Y", 3) == d.psnr("Y") and s.psnr("Cb", 4) == d.psnr("Cb") and s.psnr(2, 2) == d.psnr("Cr")
        ranked = s.rank("rans")
        assert ranked == rank_numpy(s.sse, s.hist) or all(abs(g[1] - w[1]) <= 1 and (g[0], g[2]) == (w[0], w[2]) for g, w in zip(ranked, rank_numpy(s.sse, s.hist)))
        lay = N_layout(csic, pl, (3, 4, 2))
        assert s.est_bytes((3, 4, 2), "raw") == 80 + lay.payload_bytes
        two = top.qsweep(np.stack([frame, frame]))
        assert two.nframes == 2 and np.array_equal(two.sse[1], s.sse) and two.rank("raw")[0][1] == 80 + 2 * N_layout(csic, pl, two.rank("raw")[0][2]).payload_bytes
    finally:
        top.close()


def N_layout(csic, pl, bits):
    N = csic._native
    p = pl.c_params
    cp = csic.make_c_params(p.width, p.height, p.chroma_a, p.chroma_b, *bits, p.factor, tuple(p.op), rounding=p.rounding, sampling=p.sampling)
    lay = N.CsicPlanarBitsLayout()
    N.check(N.lib().csic_planar_bits_layout_of(C.byref(cp), C.byref(lay)))
    return lay


def test_headline_plan_kernel_names(csic):
    """8192 x 8192 at 4:2:0: names and sizes only, no launch."""
    N = csic._native
    for f in (1, 2):
        with _plan(csic, 8192, 8192, 2, 0, f=f) as pl:
            assert pl.qsweep_kernel_name == f"k_qsweep_sse_fast<f{f}>" == pl.distortion_kernel_name.replace("k_dist", "k_qsweep_sse")
            g = pl.planar_layout
            blocks = pl.distortion_workspace_bytes(1) // 48
            assert pl.qsweep_workspace_bytes(1) == (blocks * 192 + 255) // 256 * 256 + g.frame_bytes
            assert pl.qsweep_workspace_bytes(3) == (3 * blocks * 192 + 255) // 256 * 256 + 3 * g.frame_bytes
            pl.tune(N.TUNE_FORCE_GENERIC, 1)
            assert pl.qsweep_kernel_name == "k_qsweep_sse_gen<hold>"
    with _plan(csic, 8192, 8192, 2, 0, f=2, avg=True) as pl:
        assert pl.qsweep_kernel_name == "k_qsweep_sse_gen<avg>"


# ---- refusals ----------------------------------------------------------------------------------
def test_refusals(csic):
    import torch
    L, N = csic._native.lib(), csic._native
    W, H = 64, 16
    with _plan(csic, W, H, 2, 0) as pl:
        need = pl.qsweep_workspace_bytes(2)
        d_in = torch.zeros(2 * W * H + 4, dtype=torch.int32, device="cuda")
        ws = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
        res = torch.zeros(2 * WORDS + 2, dtype=torch.int64, device="cuda")
        planar = torch.zeros(2 * pl.planar_layout.frame_bytes + 256, dtype=torch.uint8, device="cuda")
        s = pl._stream()
        assert ws.data_ptr() % 256 == 0 and planar.data_ptr() % 256 == 0

        def call(n=2, in_off=0, res_off=0, ws_off=0, ws_bytes=need):
            return L.csic_qsweep_device(pl._h, C.c_void_p(d_in.data_ptr() + in_off), n, C.c_void_p(res.data_ptr() + res_off),
                                        C.c_void_p(ws.data_ptr() + ws_off), ws_bytes, s)

        def hist_call(n=2, src_off=0, res_off=0):
            return L.csic_qsweep_hist_device(pl._h, C.c_void_p(planar.data_ptr() + src_off), n, C.c_void_p(res.data_ptr() + res_off), s)
        assert call(n=0) == N.EINVAL_SIZE and call(n=65536) == N.EINVAL_SIZE
        assert call(ws_bytes=need - 1) == N.EINVAL_SIZE and b"smaller" in L.csic_last_error()
        assert call(in_off=2) == N.EINVAL_SIZE and call(res_off=4) == N.EINVAL_SIZE and call(ws_off=128) == N.EINVAL_SIZE and call(ws_off=8) == N.EINVAL_SIZE
        assert hist_call(n=0) == N.EINVAL_SIZE and hist_call(src_off=128) == N.EINVAL_SIZE and hist_call(res_off=4) == N.EINVAL_SIZE
        assert L.csic_qsweep_device(pl._h, None, 2, C.c_void_p(res.data_ptr()), C.c_void_p(ws.data_ptr()), need, s) == N.EINVAL_NULL
        assert call() == N.OK and call(in_off=4, res_off=8, ws_off=256, ws_bytes=need + 256) == N.OK and hist_call() == N.OK and hist_call(res_off=8) == N.OK
        torch.cuda.synchronize()
        with pytest.raises(csic.IllegalArgumentException):
            pl.qsweep_device(d_in[:W * H + 1])
        with pytest.raises(csic.IllegalArgumentException):
            pl.qsweep_hist_device(planar[:pl.planar_layout.frame_bytes + 1])
        with pytest.raises(csic.IllegalArgumentException) as ei:
            pl.qsweep_host(np.zeros(W * H + 1, dtype=np.uint32))
        assert ei.value.status == N.EINVAL_SIZE
    cp = csic.make_c_params(W, H, 2, 0, 6, 5, 5, 1, CSQ)
    cp.in_format = N.FMT_YCBCR888X
    with csic.Plan(cp, 0) as ycc:
        with pytest.raises(csic.IllegalArgumentException) as ei:
            ycc.qsweep_workspace_bytes(1)
        assert ei.value.status == N.EINVAL_FORMAT
        with pytest.raises(csic.IllegalArgumentException) as ei:
            ycc.qsweep_host(np.zeros(W * H, dtype=np.uint32))
        assert ei.value.status == N.EINVAL_FORMAT


# ---- compress --target-bytes, end to end ---------------------------------------------------------------
OPS = ("chroma", "spatial", "color")


def procedure(ranked, target, size_of, max_tries=4):
    """The procedure of ImageCompressionApp.compressImageToSize on a ranked table and the coder's real sizes -> (bits, est, size, tries);
    bits None: refused (tries 0) or not reachable."""
    r, tries = 1.0, 0
    for _, est, bits in ranked:
        if est * r > target:
            continue
        if tries == max_tries:
            break
        size = size_of(bits)
        tries += 1
        if size <= target:
            return bits, est, size, tries
        r = max(r, size / est)
    return None, None, None, tries


@pytest.fixture(scope="module")
def in512(csic, tmp_path_factory):
    """The sweep of in512.png at 4:2:0, factor 1, and the size of the file `compress` writes for a bit set (each written once)."""
    png = os.path.join(GOLDEN, "inputs", "in512.png")
    PS = csic.ProcessingStep
    argb = csic.ImageProcessorModel.readImage(png).argb
    top = csic.ImageCompressorTop(512, 512, 2, 0, 8, 8, 8, 1, PS.ChromaSubsampling, PS.SpatialSampling, PS.ColorQuantization)
    sweep = top.qsweep(argb)
    top.close()
    d = tmp_path_factory.mktemp("qsweep")
    sizes = {}

    def size_of(bits, coding):
        if (bits, coding) not in sizes:
            sizes[bits, coding] = csic.ImageCompressionApp.compressImage(png, str(d / "probe.csic"), 2, 0, *bits, 1, PS.ChromaSubsampling, PS.SpatialSampling,
                                                                         PS.ColorQuantization, coding=coding)
        return sizes[bits, coding]
    return png, sweep, size_of, d


def _cli(csic, png, out, target, coding=None, extra=()):
    args = ["compress", "--input", png, "--output", out, "--a", "2", "--b", "0", "--sf", "1", "--op1", OPS[0], "--op2", OPS[1], "--op3", OPS[2],
            "--target-bytes", str(target)] + (["--coding", coding] if coding else []) + list(extra)
    return csic.app.main(args)


@pytest.mark.parametrize("target", [100000, 30000])
def test_target_bytes_lands_under_the_target(csic, in512, capsys, target):
    """Measured with the device's exact table and the files `compress` writes: 100 000 -> 4/4/2, estimate 77 349, 82 268 bytes in 2
    tries; 30 000 -> 1/4/1, estimate 24 334, 27 500 bytes in 2 tries (every target from 200 000 down to 20 000 took at most 2)."""
    png, sweep, size_of, d = in512
    ranked = rank_numpy(sweep.sse, sweep.hist)
    bits, est, size, tries = procedure(ranked, target, lambda b: size_of(b, "rans"))
    print(f"target {target}: numpy procedure -> bits {bits}, est {est}, size {size}, tries {tries}")
    assert bits is not None and tries <= 4
    out = str(d / f"t{target}.csic")
    assert _cli(csic, png, out, target) == 0
    text = capsys.readouterr().out
    assert os.path.getsize(out) == size <= target
    info = csic.container_info(out)
    assert (info.params.y_bits, info.params.cb_bits, info.params.cr_bits) == bits and info.version == 7
    assert f"Bits Y/Cb/Cr {bits[0]}/{bits[1]}/{bits[2]}," in text and f"written {size} bytes" in text and f"in {tries} tries" in text
    assert abs(int(text.split("estimated ")[1].split(" ")[0]) - est) <= 1
    back = str(d / f"t{target}.png")
    assert csic.app.main(["decompress", "--input", out, "--output", back]) == 0
    assert csic.ImageProcessorModel.imageSize(back) == (512, 512)


def test_an_unreachable_target_leaves_no_file(csic, in512, capsys):
    """1/1/1 is 15 104 bytes against an estimate of 12 155: two bit sets are estimated to fit 15 000, both are encoded, neither fits."""
    png, sweep, size_of, d = in512
    target = 15000
    bits, _, _, tries = procedure(rank_numpy(sweep.sse, sweep.hist), target, lambda b: size_of(b, "rans"))
    print(f"target {target}: numpy procedure -> bits {bits}, tries {tries}; 1/1/1 is {size_of((1, 1, 1), 'rans')} bytes")
    assert bits is None and size_of((1, 1, 1), "rans") > target
    out = str(d / "t15000.csic")
    assert _cli(csic, png, out, target) != 0
    text = capsys.readouterr().out
    assert not os.path.exists(out)
    assert ("not reachable in 4 tries" in text) if tries else ("no bit set is estimated to fit" in text)


def test_raw_takes_one_try_and_its_size_is_the_estimate(csic, in512, capsys):
    png, sweep, size_of, d = in512
    target = 200000
    ranked = sweep.rank("raw")
    bits, est, size, tries = procedure(ranked, target, lambda b: size_of(b, "raw"))
    assert tries == 1 and size == est <= target
    out = str(d / "raw.csic")
    assert _cli(csic, png, out, target, "raw") == 0
    text = capsys.readouterr().out
    assert os.path.getsize(out) == est and f"estimated {est} bytes, written {est} bytes" in text and "in 1 tries" in text
    info = csic.container_info(out)
    assert (info.params.y_bits, info.params.cb_bits, info.params.cr_bits) == bits and info.version == 1
    # --yq / --cbq / --crq are upper bounds
    assert _cli(csic, png, out, target, "raw", ("--yq", "4", "--cbq", "3", "--crq", "8")) == 0
    capsys.readouterr()
    p = csic.container_info(out).params
    assert p.y_bits <= 4 and p.cb_bits <= 3 and os.path.getsize(out) <= target
    want = procedure(sweep.rank("raw", max_bits=(4, 3, 8)), target, lambda b: size_of(b, "raw"))
    assert (p.y_bits, p.cb_bits, p.cr_bits) == want[0] and os.path.getsize(out) == want[1]
