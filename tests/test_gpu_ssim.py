"""Structural similarity on the GPU (csic_ssim_*): every sum, and the map where asked for, equal, exactly, to the numpy statement of
the definition (tests/test_ssim_host.py) on the oracle's outputs; the decode path, the reference's golden images, batches, alignment,
the host paths, graph capture, refusals and a frame whose sums pass 2^32.  Run with `-m gpu` on an MI355X."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_png_rgb
from test_ssim_host import ONE, oracle_ssim, ssim_numpy

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "manifest.json")) as _fh:
    _MANIFEST = json.load(_fh)
_GOLDENS = [g for g in _MANIFEST["goldens"]
            if min(_MANIFEST["inputs"][g["input"]]["width"], _MANIFEST["inputs"][g["input"]]["height"]) >= 8]

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


def _to_device(frames):
    import torch
    return torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint32).reshape(-1).view(np.int32)).cuda()


def _device_ssim(pl, frames, nframes=1, want_map=False):
    import torch
    out = pl.ssim_device(_to_device(frames), nframes, want_map=want_map)
    torch.cuda.synchronize()
    if want_map:
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy()


# ---- random parameters, both kernels, against numpy-from-oracle --------------------------------
@pytest.mark.parametrize("seed", range(3))
def test_random_shapes_vs_numpy(csic, oracle, seed):
    rng = np.random.default_rng(9300 + seed)
    shapes = [(8, 8), (16, 8), (13, 9), (24, 17), (64, 31), (72, 40)]
    fixed = [dict(W=W, H=H, f=8) for W, H in shapes] + [dict(W=W, H=H, f=f) for (W, H), f in zip(shapes, (1, 2, 4, 2, 1, 4))]
    names = set()
    for i in range(50):
        W, H = int(rng.integers(8, 91)), int(rng.integers(8, 41))
        if rng.random() < 0.5:
            W, H = (W + 7) // 8 * 8, (H + 7) // 8 * 8              # the fast kernels' shapes, often
        f = int(rng.choice([1, 2, 4, 8]))
        if i < len(fixed):
            W, H, f = fixed[i]["W"], fixed[i]["H"], fixed[i]["f"]
        a, b = CHROMA[int(rng.integers(0, 6))]
        bits = tuple(int(x) for x in rng.integers(1, 9, 3))
        avg = rng.random() < 0.3
        op = CSQ if avg else ORDERS[int(rng.integers(0, 6))]
        rounding, in_format = int(rng.integers(0, 2)), int(rng.random() < 0.25)
        if len(fixed) <= i < len(fixed) + 2:                        # every seed meets both fast kernels, whatever it draws
            W, H, f = (W + 7) // 8 * 8, (H + 7) // 8 * 8, 1 + i - len(fixed)
            avg, op, in_format = False, CSQ, 0
        frame = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        if in_format == 1:
            frame &= np.uint32(0x00FFFFFF)
        want, want_map = oracle_ssim(oracle, frame, W, H, a, b, bits, f, op, rounding, avg=avg, in_format=in_format)
        with _plan(csic, W, H, a, b, bits, f, op, rounding, avg, in_format) as pl:
            names.add(pl.ssim_kernel_name)
            what = (pl.ssim_kernel_name, W, H, a, b, bits, f, op, rounding, avg, in_format)
            got, got_map = _device_ssim(pl, frame, want_map=True)
            assert got[0].tolist() == want, what
            assert np.array_equal(got_map[0], want_map), what
            pl.tune(csic._native.TUNE_FORCE_GENERIC, 1)
            assert pl.ssim_kernel_name.startswith("k_ssim_gen")
            got, got_map = _device_ssim(pl, frame, want_map=True)
            assert got[0].tolist() == want, ("generic",) + what
            assert np.array_equal(got_map[0], want_map), ("generic",) + what
    assert {"k_ssim_fast<f1>", "k_ssim_fast<f2>"} <= names and any(n.startswith("k_ssim_gen") for n in names)


@pytest.mark.parametrize("a,b", CHROMA)
@pytest.mark.parametrize("f", [1, 2])
def test_fast_kernel_every_chroma_mode(csic, oracle, a, b, f):
    """Both roundings, every order, the fast kernels' own shapes: 33 x 9 windows, 10 blocks of 32 with a partial last one."""
    rng = np.random.default_rng(a * 10 + b + f)
    W, H = 264, 72
    frame = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
    for op in ORDERS:
        rounding = int(rng.integers(0, 2))
        want, want_map = oracle_ssim(oracle, frame, W, H, a, b, (6, 5, 5), f, op, rounding)
        with _plan(csic, W, H, a, b, (6, 5, 5), f, op, rounding) as pl:
            s_first = op.index(1) < op.index(3)
            assert pl.ssim_kernel_name == ("k_ssim_gen<hold>" if f == 2 and s_first else f"k_ssim_fast<f{f}>")
            got, got_map = _device_ssim(pl, frame, want_map=True)
            assert got[0].tolist() == want and np.array_equal(got_map[0], want_map), (op, rounding)
            pl.tune(csic._native.TUNE_NO_VECTOR, 1)                 # the 4-byte loads
            assert _device_ssim(pl, frame)[0].tolist() == want, (op, rounding, "no-vector")


def test_headline_plans_take_the_fast_kernel(csic):
    for f in (1, 2):
        with _plan(csic, 8192, 8192, 2, 0, (8, 8, 8), f) as pl:
            assert pl.ssim_kernel_name == f"k_ssim_fast<f{f}>"
            pl.tune(csic._native.TUNE_FORCE_GENERIC, 1)
            assert pl.ssim_kernel_name == "k_ssim_gen<hold>"
        with _plan(csic, 8192, 8190, 2, 0, (8, 8, 8), f) as pl:      # a cut last window row: the general kernel
            assert pl.ssim_kernel_name == "k_ssim_gen<hold>"
    with _plan(csic, 64, 64, 2, 0, (8, 8, 8), 2, avg=True, in_format=1) as pl:
        assert pl.ssim_kernel_name == "k_ssim_gen<avg,ycc-in>"


# ---- independence from the fused path: the decoded frame, measured by numpy -------------------------
def test_equals_numpy_on_the_decoded_frames(csic):
    import torch
    W, H, f = 64, 48, 2
    N = csic._native
    rng = np.random.default_rng(31)
    frame = rng.integers(0, 1 << 32, (H, W), dtype=np.uint32)
    d_in = _to_device(frame)
    dec = []
    for fmt in (N.FMT_ARGB8888, N.FMT_YCBCR888X):
        with _plan(csic, W, H, 2, 0, (6, 5, 5), f, fmt=fmt) as pl:
            d = pl.decode_device(pl.process_device(d_in), src_format=fmt, out_format=fmt)
            torch.cuda.synchronize()
            dec.append(d.cpu().numpy().view(np.uint32).reshape(H, W))
    want, want_map = ssim_numpy(frame, dec[0], dec[1], 1)               # decoded frames are full size: paired one to one
    with _plan(csic, W, H, 2, 0, (6, 5, 5), f) as pl:
        got, got_map = _device_ssim(pl, frame, want_map=True)
        assert got[0].tolist() == want and np.array_equal(got_map[0], want_map)
    assert want != [ONE * 48] * 6 and max(want) <= ONE * 48


# ---- the reference's golden images -------------------------------------------------------------
def _argb(rgb):
    r, g, b = (rgb[..., k].astype(np.uint32) for k in range(3))
    return 0xFF000000 | (r << 16) | (g << 8) | b


@pytest.mark.parametrize("e", _GOLDENS, ids=[g["name"] for g in _GOLDENS])
def test_golden_files_rgb_sums(csic, input_images, e):
    """R, G, B SSIM sums between the committed input PNG and the committed golden output PNG, paired by replication, == the GPU's."""
    rgb_in = input_images[e["input"]]
    want_img = load_png_rgb(os.path.join(GOLDEN, e["file"]))
    H, W = rgb_in.shape[:2]
    f = e["factor"]
    files = ssim_numpy(_argb(rgb_in), _argb(want_img), np.zeros(want_img.shape[:2], dtype=np.uint32), f)[0][:3]
    if e["rounding"] == "IDENTITY":             # readImage -> writeImage round trip: no pipeline, nothing lost
        assert files == [ONE * (W // 8) * (H // 8)] * 3
        return
    rounding = 1 if e["rounding"] == "TRUNC_SW" else 0
    with _plan(csic, W, H, e["chroma_a"], e["chroma_b"], tuple(e["bits"]), f, tuple(e["op"]), rounding) as pl:
        assert _device_ssim(pl, _argb(rgb_in))[0].tolist()[:3] == files
        pl.tune(csic._native.TUNE_FORCE_GENERIC, 1)
        assert _device_ssim(pl, _argb(rgb_in))[0].tolist()[:3] == files


# ---- sums past 2^32 ----------------------------------------------------------------------------
def test_accumulation_past_2_32(csic):
    """4:4:4, 8 / 8 / 8, factor 1 loses nothing in Y, Cb, Cr: every window's q is 65536, and 2048 x 2056 has 65 792 windows."""
    import torch
    W, H = 2048, 2056
    r = torch.arange(H, device="cuda", dtype=torch.int64)[:, None]
    c = torch.arange(W, device="cuda", dtype=torch.int64)[None, :]
    frame = (((r * 40503 + c * 1048573) ^ (r * c * 7 + 12345)) & 0x7FFFFFFF).to(torch.int32).contiguous()      # any bits will do
    want = ONE * 65792
    assert want > 2 ** 32
    with _plan(csic, W, H) as pl:
        assert pl.ssim_kernel_name == "k_ssim_fast<f1>"
        got = pl.ssim_device(frame)
        torch.cuda.synchronize()
        assert got.cpu().numpy()[0].tolist()[3:] == [want] * 3
        fast_rgb = got.cpu().numpy()[0].tolist()[:3]
        pl.tune(csic._native.TUNE_FORCE_GENERIC, 1)
        got = pl.ssim_device(frame)
        torch.cuda.synchronize()
        assert got.cpu().numpy()[0].tolist() == fast_rgb + [want] * 3
    del frame
    torch.cuda.empty_cache()


# ---- batches, alignment, the host paths, the map ---------------------------------------------------
def test_batch_equals_single_calls(csic, oracle):
    W, H, f = 40, 24, 2
    rng = np.random.default_rng(W + H)
    frames = rng.integers(0, 1 << 32, (3, H, W), dtype=np.uint32)
    with _plan(csic, W, H, 2, 0, (6, 5, 5), f) as pl:
        batch, batch_map = _device_ssim(pl, frames, 3, want_map=True)
        for k in range(3):
            want, want_map = oracle_ssim(oracle, frames[k].reshape(-1), W, H, 2, 0, (6, 5, 5), f)
            assert batch[k].tolist() == want and np.array_equal(batch_map[k], want_map)
            assert _device_ssim(pl, frames[k])[0].tolist() == want
        host, host_map = pl.ssim_host(frames, 3, want_map=True)
        assert np.array_equal(host, batch) and np.array_equal(host_map, batch_map)
        assert np.array_equal(pl.ssim_host(frames, 3), batch)
        ss = pl.ssim(frames)
        assert [s.sums for s in ss] == [tuple(int(v) for v in row) for row in batch] and ss[0].windows == 15


@pytest.mark.parametrize("f", [1, 2])
def test_input_offset_by_four_bytes(csic, f):
    """A d_in that is only 4-byte aligned takes the fast kernel's 4-byte loads: the same sums."""
    import torch
    W, H = 256, 64
    rng = np.random.default_rng(f)
    frames = rng.integers(0, 1 << 32, 2 * W * H, dtype=np.uint32)
    with _plan(csic, W, H, 2, 0, (3, 3, 2), f) as pl:
        assert pl.ssim_kernel_name == f"k_ssim_fast<f{f}>"
        want = _device_ssim(pl, frames, 2)
        buf = torch.zeros(2 * W * H + 4, dtype=torch.int32, device="cuda")
        buf[1:1 + 2 * W * H] = torch.from_numpy(frames.view(np.int32)).cuda()
        got = pl.ssim_device(buf[1:1 + 2 * W * H], 2)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want)


def test_host_and_python_paths_agree_with_the_device(csic, oracle):
    W, H = 100, 60
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 1 << 32, (H, W), dtype=np.uint32)
    top = csic.ImageCompressorTop(W, H, 2, 0, 6, 5, 5, 2, csic.ProcessingStep.ChromaSubsampling,
                                  csic.ProcessingStep.SpatialSampling, csic.ProcessingStep.ColorQuantization)
    try:
        pl = top.plan()
        dev = _device_ssim(pl, frame)[0].tolist()
        assert pl.ssim_host(frame)[0].tolist() == dev
        s = top.ssim(frame)
        assert isinstance(s, csic.Ssim) and list(s.sums) == dev and s.windows == 12 * 7
        assert top.ssim(_to_device(frame).reshape(H, W)) == s
        assert dev == oracle_ssim(oracle, frame.reshape(-1), W, H, 2, 0, (6, 5, 5), 2)[0]
        assert s.mean_rgb == pytest.approx(sum(dev[:3]) / (3 * ONE * 84))
    finally:
        top.close()


def test_map_on_request_and_sums_without_it(csic, oracle):
    W, H = 88, 40
    rng = np.random.default_rng(12)
    frame = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
    for f, avg in ((1, False), (4, False), (2, True)):
        want, want_map = oracle_ssim(oracle, frame, W, H, 2, 0, (5, 4, 4), f, avg=avg)
        with _plan(csic, W, H, 2, 0, (5, 4, 4), f, avg=avg) as pl:
            got, got_map = _device_ssim(pl, frame, want_map=True)
            assert got_map.shape == (1, 6, 5, 11) and got_map.dtype == np.int32 and np.array_equal(got_map[0], want_map)
            assert got[0].tolist() == want
            assert _device_ssim(pl, frame)[0].tolist() == want            # d_map = NULL
            assert got_map[0].reshape(6, -1).sum(axis=1).tolist() == want


def test_capture_and_replay_in_a_graph(csic):
    import torch
    W, H = 512, 256
    rng = np.random.default_rng(11)
    frames = torch.from_numpy(rng.integers(0, 1 << 32, 3 * W * H, dtype=np.uint32).view(np.int32)).cuda()
    with _plan(csic, W, H, 2, 0, (6, 5, 5), 2) as pl:
        want = pl.ssim_device(frames, 3).clone()                  # the warm-up: also allocates the plan's workspace
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                out = pl.ssim_device(frames, 3)
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(2):
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want)


def test_refusals(csic):
    import torch
    L, N = csic._native.lib(), csic._native
    for W, H in ((7, 20), (20, 7)):
        with _plan(csic, W, H) as pl:
            b = C.c_size_t()
            assert L.csic_ssim_workspace_bytes(pl._h, 1, C.byref(b)) == N.EINVAL_DIMS
            buf = torch.zeros(256, dtype=torch.int64, device="cuda")
            p = C.c_void_p(buf.data_ptr())
            assert L.csic_ssim_device(pl._h, p, 1, p, None, p, 2048, pl._stream()) == N.EINVAL_DIMS
            with pytest.raises(csic.IllegalArgumentException):
                pl.ssim_host(np.zeros(W * H, dtype=np.uint32))
    W, H = 64, 16
    with _plan(csic, W, H, 2, 0, (8, 8, 8), 2) as pl:
        b = C.c_size_t()
        assert L.csic_ssim_workspace_bytes(pl._h, 0, C.byref(b)) == N.EINVAL_SIZE
        assert L.csic_ssim_workspace_bytes(pl._h, 65536, C.byref(b)) == N.EINVAL_SIZE
        assert L.csic_ssim_workspace_bytes(pl._h, 65535, C.byref(b)) == N.OK and b.value > 0
        need = pl.ssim_workspace_bytes(2)
        d_in = torch.zeros(2 * W * H + 4, dtype=torch.int32, device="cuda")
        ws = torch.zeros(need // 8 + 2, dtype=torch.int64, device="cuda")
        sums = torch.zeros(2 * 6 + 2, dtype=torch.int64, device="cuda")
        dmap = torch.zeros(2 * 6 * 16 + 2, dtype=torch.int32, device="cuda")
        s = pl._stream()

        def call(n=2, in_off=0, sums_off=0, map_off=None, ws_off=0, ws_bytes=need):
            return L.csic_ssim_device(pl._h, C.c_void_p(d_in.data_ptr() + in_off), n, C.c_void_p(sums.data_ptr() + sums_off),
                                      None if map_off is None else C.c_void_p(dmap.data_ptr() + map_off),
                                      C.c_void_p(ws.data_ptr() + ws_off), ws_bytes, s)
        assert call(n=0) == N.EINVAL_SIZE
        assert call(n=65536) == N.EINVAL_SIZE
        assert call(ws_bytes=need - 1) == N.EINVAL_SIZE
        assert call(sums_off=4) == N.EINVAL_SIZE
        assert call(ws_off=4) == N.EINVAL_SIZE
        assert call(map_off=2) == N.EINVAL_SIZE
        assert call(in_off=2) == N.EINVAL_SIZE
        pi, ps, pw = C.c_void_p(d_in.data_ptr()), C.c_void_p(sums.data_ptr()), C.c_void_p(ws.data_ptr())
        assert L.csic_ssim_device(pl._h, None, 2, ps, None, pw, need, s) == N.EINVAL_NULL
        assert L.csic_ssim_device(pl._h, pi, 2, None, None, pw, need, s) == N.EINVAL_NULL
        assert L.csic_ssim_device(pl._h, pi, 2, ps, None, None, need, s) == N.EINVAL_NULL
        assert call() == N.OK and call(map_off=0) == N.OK
        torch.cuda.synchronize()
        with pytest.raises(csic.IllegalArgumentException):
            pl.ssim_host(np.zeros(W * H + 1, dtype=np.uint32))
