"""Distortion measurement on the GPU (csic_distortion_*): every sum equal, exactly, to the numpy statement of the definition
(tests/test_distortion_host.py) on the oracle's outputs; the reference's golden images; batches, alignment, the host paths, graph
capture, refusals and a frame whose sums pass 2^32.  Run with `-m gpu` on an MI355X."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_png_rgb
from test_distortion_host import oracle_sse, sse_numpy

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "manifest.json")) as _fh:
    _GOLDENS = json.load(_fh)["goldens"]

ORDERS = list(itertools.permutations((1, 2, 3)))
CSQ = (3, 1, 2)
CHROMA = [(4, 4), (2, 2), (2, 0), (1, 1), (4, 0), (1, 0)]


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    assert csic_amd._native.lib().csic_device_count() >= 1
    return csic_amd


def _plan(csic, W, H, a=4, b=4, bits=(8, 8, 8), f=1, op=CSQ, rounding=0, avg=False, in_format=0, fmt=0):
    cp = csic.make_c_params(W, H, a, b, *bits, f, op, rounding=rounding, out_format=fmt, sampling=1 if avg else 0,
                            in_format=in_format)
    return csic.Plan(cp, 0)


def _device_sse(csic, pl, frames, nframes=1):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint32).reshape(-1).view(np.int32)).cuda()
    out = pl.distortion_device(d, nframes)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.uint64)


# ---- random parameters, both kernels, against numpy-from-oracle --------------------------------
@pytest.mark.parametrize("seed", range(3))
def test_random_shapes_vs_numpy(csic, oracle, seed):
    rng = np.random.default_rng(9100 + seed)
    fixed = [dict(W=1, H=1, f=1), dict(W=1, H=1, f=8), dict(W=7, H=3, f=8), dict(W=13, H=5, f=2), dict(W=64, H=32, f=2),
             dict(W=64, H=31, f=1), dict(W=6, H=4, f=4)]
    names = set()
    for i in range(70):
        W, H = int(rng.integers(1, 90)), int(rng.integers(1, 40))
        if rng.random() < 0.5:
            W = (W + 3) // 4 * 4                                  # the fast kernels' shapes, often
        f = int(rng.choice([1, 2, 4, 8]))
        if i < len(fixed):
            W, H, f = fixed[i]["W"], fixed[i]["H"], fixed[i]["f"]
        a, b = CHROMA[int(rng.integers(0, 6))]
        bits = tuple(int(x) for x in rng.integers(1, 9, 3))
        avg = rng.random() < 0.3
        op = CSQ if avg else ORDERS[int(rng.integers(0, 6))]
        rounding, in_format = int(rng.integers(0, 2)), int(rng.random() < 0.25)
        frame = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        if in_format == 1:
            frame &= np.uint32(0x00FFFFFF)
        want = oracle_sse(oracle, frame, W, H, a, b, bits, f, op, rounding, avg=avg, in_format=in_format)
        with _plan(csic, W, H, a, b, bits, f, op, rounding, avg, in_format) as pl:
            names.add(pl.distortion_kernel_name)
            got = _device_sse(csic, pl, frame)[0].tolist()
            assert got == want, (pl.distortion_kernel_name, W, H, a, b, bits, f, op, rounding, avg, in_format)
            pl.tune(csic._native.TUNE_FORCE_GENERIC, 1)
            assert pl.distortion_kernel_name.startswith("k_dist_gen")
            got = _device_sse(csic, pl, frame)[0].tolist()
            assert got == want, ("generic", W, H, a, b, bits, f, op, rounding, avg, in_format)
    assert {"k_dist_fast<f1>", "k_dist_fast<f2>"} <= names and any(n.startswith("k_dist_gen") for n in names)


@pytest.mark.parametrize("a,b", CHROMA)
@pytest.mark.parametrize("f", [1, 2])
def test_fast_kernel_every_chroma_mode(csic, oracle, a, b, f):
    """Both roundings, every order, the fast kernels' own shapes (rows of whole units, several blocks, a partial last block); then
    the same plan under TUNE_NO_VECTOR: the sums must not move.  (The kernel name is defined for an aligned d_in and the sums are
    equal whichever load width ran, so this does not show that the 4-byte loads were taken -- only that the knob is harmless.)"""
    rng = np.random.default_rng(a * 10 + b + f)
    W, H = 136, 62
    frame = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
    for op in ORDERS:
        rounding = int(rng.integers(0, 2))
        want = oracle_sse(oracle, frame, W, H, a, b, (6, 5, 5), f, op, rounding)
        with _plan(csic, W, H, a, b, (6, 5, 5), f, op, rounding) as pl:
            s_first = op.index(1) < op.index(3)
            assert pl.distortion_kernel_name == ("k_dist_gen<hold>" if f == 2 and s_first else f"k_dist_fast<f{f}>")
            got = _device_sse(csic, pl, frame)[0].tolist()
            assert got == want
            name = pl.distortion_kernel_name
            pl.tune(csic._native.TUNE_NO_VECTOR, 1)
            assert pl.distortion_kernel_name == name
            assert _device_sse(csic, pl, frame)[0].tolist() == got == want


def test_headline_plans_take_the_fast_kernel(csic):
    for f in (1, 2):
        with _plan(csic, 8192, 8192, 2, 0, (8, 8, 8), f) as pl:
            assert pl.distortion_kernel_name == f"k_dist_fast<f{f}>"
            pl.tune(csic._native.TUNE_FORCE_GENERIC, 1)
            assert pl.distortion_kernel_name == "k_dist_gen<hold>"


# ---- the reference's golden images -------------------------------------------------------------
def _argb(rgb):
    r, g, b = (rgb[..., k].astype(np.uint32) for k in range(3))
    return 0xFF000000 | (r << 16) | (g << 8) | b


@pytest.mark.parametrize("e", _GOLDENS, ids=[g["name"] for g in _GOLDENS])
def test_golden_files_rgb_sums(csic, input_images, e):
    """RGB sums between the committed input PNG and the committed golden output PNG, paired by replication, == the GPU's."""
    rgb_in = input_images[e["input"]]
    want_img = load_png_rgb(os.path.join(GOLDEN, e["file"]))
    H, W = rgb_in.shape[:2]
    f = e["factor"]
    src = rgb_in.astype(np.int64)
    up = want_img.astype(np.int64)[(np.arange(H) // f)[:, None], (np.arange(W) // f)[None, :]]
    files = [int(((src[..., k] - up[..., k]) ** 2).sum()) for k in range(3)]
    if e["rounding"] == "IDENTITY":             # readImage -> writeImage round trip: no pipeline, nothing lost
        assert files == [0, 0, 0]
        return
    rounding = 1 if e["rounding"] == "TRUNC_SW" else 0
    with _plan(csic, W, H, e["chroma_a"], e["chroma_b"], tuple(e["bits"]), f, tuple(e["op"]), rounding) as pl:
        got = _device_sse(csic, pl, _argb(rgb_in))[0].tolist()
        assert got[:3] == files
        pl.tune(csic._native.TUNE_FORCE_GENERIC, 1)
        assert _device_sse(csic, pl, _argb(rgb_in))[0].tolist()[:3] == files


# ---- batches, alignment, the host paths ---------------------------------------------------------
@pytest.mark.parametrize("W,H,f", [(33, 7, 2), (64, 32, 2), (128, 20, 1), (30, 9, 1)])
def test_batch_equals_single_calls(csic, W, H, f):
    rng = np.random.default_rng(W + H)
    frames = rng.integers(0, 1 << 32, (5, H, W), dtype=np.uint32)
    with _plan(csic, W, H, 2, 0, (6, 5, 5), f) as pl:
        batch = _device_sse(csic, pl, frames, 5)
        for k in range(5):
            assert batch[k].tolist() == _device_sse(csic, pl, frames[k])[0].tolist()
        assert np.array_equal(pl.distortion_host(frames, 5), batch)
        ds = pl.distortion(frames)
        assert [d.sse for d in ds] == [tuple(int(v) for v in row) for row in batch]


@pytest.mark.parametrize("f", [1, 2])
def test_input_offset_by_four_bytes(csic, f):
    """A d_in that is only 4-byte aligned takes the fast kernel's 4-byte loads: the same sums."""
    import torch
    W, H = 256, 64
    rng = np.random.default_rng(f)
    frames = rng.integers(0, 1 << 32, 2 * W * H, dtype=np.uint32)
    with _plan(csic, W, H, 2, 0, (3, 3, 2), f) as pl:
        want = _device_sse(csic, pl, frames, 2)
        buf = torch.zeros(2 * W * H + 4, dtype=torch.int32, device="cuda")
        buf[1:1 + 2 * W * H] = torch.from_numpy(frames.view(np.int32)).cuda()
        got = pl.distortion_device(buf[1:1 + 2 * W * H], 2)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy().astype(np.uint64), want)


def test_host_and_python_paths_agree_with_the_device(csic, oracle):
    import torch
    W, H = 100, 60
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 1 << 32, (H, W), dtype=np.uint32)
    top = csic.ImageCompressorTop(W, H, 2, 0, 6, 5, 5, 2, csic.ProcessingStep.ChromaSubsampling,
                                  csic.ProcessingStep.SpatialSampling, csic.ProcessingStep.ColorQuantization)
    try:
        pl = top.plan()
        dev = _device_sse(csic, pl, frame)[0].tolist()
        assert pl.distortion_host(frame)[0].tolist() == dev
        d = top.distortion(frame)
        assert isinstance(d, csic.Distortion) and list(d.sse) == dev and d.pixels == W * H
        assert top.distortion(torch.from_numpy(frame.view(np.int32)).cuda()) == d
        assert list(d.sse) == oracle_sse(oracle, frame, W, H, 2, 0, (6, 5, 5), 2)
        assert d.psnr_rgb == pytest.approx(10 * np.log10(65025.0 * 3 * W * H / sum(dev[:3])))
    finally:
        top.close()


def test_capture_and_replay_in_a_graph(csic):
    import torch
    W, H = 512, 256
    rng = np.random.default_rng(11)
    frames = torch.from_numpy(rng.integers(0, 1 << 32, 3 * W * H, dtype=np.uint32).view(np.int32)).cuda()
    with _plan(csic, W, H, 2, 0, (6, 5, 5), 2) as pl:
        want = pl.distortion_device(frames, 3).clone()                  # also allocates the plan's workspace
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                out = pl.distortion_device(frames, 3)
        torch.cuda.current_stream().wait_stream(s)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


def test_refusals(csic):
    import torch
    L, N = csic._native.lib(), csic._native
    W, H = 64, 16
    with _plan(csic, W, H, 2, 0, (8, 8, 8), 2) as pl:
        b = C.c_size_t()
        assert L.csic_distortion_workspace_bytes(pl._h, 0, C.byref(b)) == N.EINVAL_SIZE
        assert L.csic_distortion_workspace_bytes(pl._h, 65536, C.byref(b)) == N.EINVAL_SIZE
        assert L.csic_distortion_workspace_bytes(pl._h, 65535, C.byref(b)) == N.OK and b.value > 0
        need = pl.distortion_workspace_bytes(2)
        d_in = torch.zeros(2 * W * H, dtype=torch.int32, device="cuda")
        ws = torch.zeros(need // 8 + 2, dtype=torch.int64, device="cuda")
        sse = torch.zeros(2 * 6 + 2, dtype=torch.int64, device="cuda")
        s = pl._stream()
        call = lambda n, sse_ptr, ws_bytes: L.csic_distortion_device(pl._h, C.c_void_p(d_in.data_ptr()), n, C.c_void_p(sse_ptr),
                                                                       C.c_void_p(ws.data_ptr()), ws_bytes, s)
        assert call(0, sse.data_ptr(), need) == N.EINVAL_SIZE
        assert call(65536, sse.data_ptr(), need) == N.EINVAL_SIZE
        assert call(2, sse.data_ptr(), need - 1) == N.EINVAL_SIZE
        assert call(2, sse.data_ptr() + 4, need) == N.EINVAL_SIZE
        assert L.csic_distortion_device(pl._h, None, 2, C.c_void_p(sse.data_ptr()), C.c_void_p(ws.data_ptr()), need, s) == N.EINVAL_NULL
        assert L.csic_distortion_device(pl._h, C.c_void_p(d_in.data_ptr()), 2, None, C.c_void_p(ws.data_ptr()), need, s) == N.EINVAL_NULL
        assert L.csic_distortion_device(pl._h, C.c_void_p(d_in.data_ptr()), 2, C.c_void_p(sse.data_ptr()), None, need, s) == N.EINVAL_NULL
        assert call(2, sse.data_ptr(), need) == N.OK
        torch.cuda.synchronize()
        with pytest.raises(csic.IllegalArgumentException):
            pl.distortion_host(np.zeros(W * H + 1, dtype=np.uint32))


# ---- sums past 2^32 ----------------------------------------------------------------------------
def test_overflow_8k_checkerboard(csic, oracle):
    """8192 x 8192, 4:2:0, factor 2, black / white checkerboard: every output pixel is white, half the input pixels black, so
    R, G, B and Y each sum 2^25 * 255^2 (> 2^32).  numpy on a 512 x 512 crop of the same period-2 pattern, times 256."""
    import torch
    W = H = 8192
    r = torch.arange(H, device="cuda", dtype=torch.int32)[:, None]
    c = torch.arange(W, device="cuda", dtype=torch.int32)[None, :]
    white = ((r + c) & 1) == 0
    frame = torch.where(white, torch.tensor(-1, dtype=torch.int32, device="cuda"),      # 0xFFFFFFFF
                        torch.tensor(-16777216, dtype=torch.int32, device="cuda")).contiguous()  # 0xFF000000
    crop = frame[:512, :512].cpu().numpy().view(np.uint32)
    want = [256 * v for v in oracle_sse(oracle, crop, 512, 512, 2, 0, (8, 8, 8), 2)]
    assert want == [(W * H // 2) * 65025] * 4 + [0, 0] and want[0] > 2 ** 32
    with _plan(csic, W, H, 2, 0, (8, 8, 8), 2) as pl:
        assert pl.distortion_kernel_name == "k_dist_fast<f2>"
        got = pl.distortion_device(frame)
        torch.cuda.synchronize()
        assert got.cpu().numpy()[0].tolist() == want
        pl.tune(csic._native.TUNE_FORCE_GENERIC, 1)
        got = pl.distortion_device(frame)
        torch.cuda.synchronize()
        assert got.cpu().numpy()[0].tolist() == want
    del frame
    torch.cuda.empty_cache()
