"""The device codec of the row-prediction layer (csic_rows.hip: k_rows, k_unrows) against the host codec (csic_rows_host, which
tests/test_rows_host.py pins to the numpy statement of tests/rows_ref.py), on code planes built on the host and uploaded.  The shapes
are the smallest that reach each path of the kernels:

    32 x 34                 delta = 0, three bands (16 + 16 + 2 rows): the register walk of k_unrows
    33 x 40, 63 x 35        delta = 1 and delta = 31: two reference groups, the steps behind barriers
    40 x 36 at 4:2:0        chroma rows of 20 samples: K = 0 beside a live Y (at 8/8/8 in one launch with it)
    95 x 33                 n = 3135 = 97 groups and 31 samples: a ragged last group, delta = 31
    8256 x 34 at 4:4:4      K = 258 > 256: lanes loop over the groups of a step (delta = 0); 8257 x 18 the same with delta = 1
    3 frames of 64 x 40     frames on grid z

with q over 1 .. 8 across the cases and CSIC_TUNE_NONTEMPORAL 1 and 0.  Per case: the difference frames inside the payload ranges and
the maps inside map_bytes byte for byte, 0xEE everywhere else, the source only read; unrows restores the source apart and in place.
Then one capture into a graph with one replay, the refusals, and the CLI.  The content here is loosely random; planes built to order
-- every delta at every q, ties and choices decided by one, the group, block and lane-loop edges, maps no encoder wrote -- live in
tests/rows_planes.py and run in tests/test_gpu_rows_planes.py against the numpy statement.  Run with `-m gpu` on an MI355X."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from delta_ref import frame_buffers
from test_gpu_pack import EE, _filled, _plan

pytestmark = pytest.mark.gpu

CASES = [(32, 34, 4, 4, (1, 2, 3), 1), (32, 34, 4, 4, (8, 8, 8), 1),
         (33, 40, 4, 4, (4, 5, 6), 1), (33, 40, 4, 4, (2, 2, 2), 1), (63, 35, 4, 4, (7, 8, 1), 1), (63, 35, 4, 4, (3, 6, 5), 1),
         (40, 36, 2, 0, (6, 5, 5), 1), (40, 36, 2, 0, (8, 8, 8), 1),
         (95, 33, 4, 4, (5, 3, 7), 1), (95, 33, 4, 4, (2, 4, 8), 1),
         (8256, 34, 4, 4, (8, 8, 8), 1), (8257, 18, 4, 4, (3, 3, 3), 1),
         (64, 40, 4, 4, (6, 5, 5), 3), (64, 40, 2, 0, (1, 8, 4), 3)]


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    assert csic_amd._native.lib().csic_device_count() >= 1
    return csic_amd


def _plane(w, h, q, rng):
    """w x h codes: rows in runs that repeat the row above with a little noise, between rows that are new -- both choices occur."""
    rows = [rng.integers(0, 1 << q, w)]
    for r in range(1, h):
        fresh = r % 5 == 0
        noise = (rng.integers(0, 12, w) == 0).astype(np.int64)
        rows.append(rng.integers(0, 1 << q, w) if fresh else (rows[-1] + noise) % (1 << q))
    return np.concatenate(rows)


def _frames(pl, bits, nframes, rng):
    g = pl.planar_bits_layout.geometry
    dims = [(g.y_width, g.y_height), (g.chroma_width, g.chroma_height), (g.chroma_width, g.chroma_height)]
    return [[_plane(w, h, q, rng) for (w, h), q in zip(dims, bits)] for _ in range(nframes)]


def _host(csic, pl, src):
    """The host codec on the same buffers, destinations pre-filled with 0xEE."""
    N = csic._native
    ml = pl.rows_layout
    diff, maps = np.full_like(src, EE), np.full((src.shape[0], ml.map_stride), EE, dtype=np.uint8)
    N.check(N.lib().csic_rows_host(C.byref(pl.c_params), src.ctypes.data_as(C.c_void_p), src.shape[0], diff.ctypes.data_as(C.c_void_p),
                                   maps.ctypes.data_as(C.c_void_p)))
    return diff, maps


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("W,H,a,b,bits,nframes", CASES)
def test_device_equals_host_and_inverts(csic, W, H, a, b, bits, nframes, nt):
    import torch
    N = csic._native
    rng = np.random.default_rng(23700 + W + 3 * H + bits[0])
    with _plan(csic, W, H, a, b, bits) as pl:
        if not nt:
            pl.tune(N.TUNE_NONTEMPORAL, 0)
        assert pl.rows_kernel_name == "k_rows<q%d,%d,%d,%s>" % (*bits, "nt" if nt else "cached")
        ml, fb = pl.rows_layout, pl.frame_bytes
        src = frame_buffers(pl.planar_bits_layout, _frames(pl, bits, nframes, rng), bits, EE)
        want_d, want_m = _host(csic, pl, src)
        live = [p for p in range(3) if ml.k[p]]
        assert want_m[:, :ml.map_bytes].any() and not want_m[:, :ml.map_bytes].all() and live     # both choices occur
        d_src = torch.from_numpy(src).cuda()
        diff, maps = pl.rows_device(d_src, nframes, _filled((nframes, fb)), _filled((nframes, ml.map_stride)))
        assert np.array_equal(diff.cpu().numpy(), want_d)                      # the payload ranges, and 0xEE outside them
        assert np.array_equal(maps.cpu().numpy(), want_m)                      # map_bytes, and 0xEE behind them
        assert np.array_equal(d_src.cpu().numpy(), src)                        # the source is only read
        back = pl.unrows_device(diff, maps, nframes, _filled((nframes, fb)))
        assert torch.equal(back, d_src)                                        # apart: the payload restored, 0xEE kept
        work = diff.clone()
        assert pl.unrows_device(work, maps, nframes, work) is work and torch.equal(work, d_src)     # in place
        # a map of ones in every live section decodes on the device to what the host decodes it to (the device does not validate)
        ones = np.zeros_like(want_m)
        for p in live:
            sec = np.zeros(4 * ((ml.groups[p] + 31) // 32) * 8, dtype=np.uint8)
            sec[:ml.groups[p]] = 1
            ones[:, ml.map_offset[p]:ml.map_offset[p] + sec.size // 8] = np.packbits(sec, bitorder="little")
        host = csic.unrows_host(pl.c_params, want_d, ones, out=want_d.copy())
        dev = pl.unrows_device(diff, torch.from_numpy(ones).cuda(), nframes, _filled((nframes, fb)))
        assert np.array_equal(dev.cpu().numpy(), host)


def test_capture_and_replay_in_a_graph(csic):
    """One linear capture of rows -> rans pack -> rans unpack -> unrows, replayed once on new contents."""
    import torch
    W, H, bits, nframes = 95, 33, (6, 5, 5), 2
    rng = np.random.default_rng(23800)
    with _plan(csic, W, H, 4, 4, bits) as pl:
        ml, fb, bound = pl.rows_layout, pl.frame_bytes, pl.rans_layout.bound_bytes
        first, second = (frame_buffers(pl.planar_bits_layout, _frames(pl, bits, nframes, rng), bits, EE) for _ in range(2))
        src = torch.from_numpy(first).cuda()
        diff, maps, coded, undone, back = (_filled((nframes, fb)), _filled((nframes, ml.map_stride)), _filled((nframes, bound)), _filled((nframes, fb)),
                                           _filled((nframes, fb)))

        def chain():
            pl.rows_device(src, nframes, diff, maps)
            pl.rans_pack_device(diff, nframes, coded)
            pl.rans_unpack_device(coded, nframes, undone)
            pl.unrows_device(undone, maps, nframes, back)
        chain()                                             # the warm-up
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                chain()
        torch.cuda.current_stream().wait_stream(s)
        src.copy_(torch.from_numpy(second).cuda())
        g.replay()
        torch.cuda.synchronize()
        want_d, want_m = _host(csic, pl, second)
        assert np.array_equal(diff.cpu().numpy(), want_d) and np.array_equal(maps.cpu().numpy(), want_m)
        assert torch.equal(undone, diff) and torch.equal(back, src)


def test_refusals(csic):
    """All before any device is touched."""
    import torch
    L, N = csic._native.lib(), csic._native
    with _plan(csic, 64, 16, 2, 0, (6, 5, 5)) as pl:
        fb, ms = pl.frame_bytes, pl.rows_layout.map_stride
        frames = torch.zeros(4 * fb + 256, dtype=torch.uint8, device="cuda")
        diff = torch.zeros(3 * fb + 256, dtype=torch.uint8, device="cuda")
        maps = torch.zeros(3 * ms + 256, dtype=torch.uint8, device="cuda")
        s = pl._stream()
        ptr = lambda t, o=0: C.c_void_p(t.data_ptr() + o)

        def rows(n=3, f=ptr(frames), d=ptr(diff), m=ptr(maps), plan=pl._h):
            return L.csic_rows_device(plan, f, n, d, m, s)

        def unrows(n=3, f=ptr(frames), d=ptr(diff), m=ptr(maps), plan=pl._h):
            return L.csic_unrows_device(plan, d, m, n, f, s)
        nul = C.c_void_p(None)
        for call in (rows, unrows):
            assert call(plan=None) == N.EINVAL_NULL and call(f=nul) == N.EINVAL_NULL and call(d=nul) == N.EINVAL_NULL and call(m=nul) == N.EINVAL_NULL
            assert call(n=0) == N.EINVAL_SIZE and call(n=65536) == N.EINVAL_SIZE
            assert call(f=ptr(frames, 64)) == N.EINVAL_SIZE and call(d=ptr(diff, 128)) == N.EINVAL_SIZE and call(m=ptr(maps, 4)) == N.EINVAL_SIZE
            assert call(d=ptr(frames, fb)) == N.EINVAL_SIZE                    # a partial overlap (frame_bytes is a multiple of 256)
            assert call(m=ptr(frames, 256)) == N.EINVAL_SIZE                   # the maps inside the frames
            assert L.csic_last_error().decode() != ""
            assert call() == N.OK
        assert rows(d=ptr(frames)) == N.EINVAL_SIZE                            # forward: not even in place
        assert unrows(d=ptr(frames)) == N.OK                                   # inverse: exactly in place
        torch.cuda.synchronize()
        assert not frames.any() and not diff.any() and not maps.any()           # zeros: a constant frame, every group a tie
        assert L.csic_rows_kernel_name(None) == b""
        with pytest.raises(csic.IllegalArgumentException):
            pl.rows_device(frames[:fb + 1])
        with pytest.raises(csic.IllegalArgumentException):
            pl.unrows_device(diff[:2 * fb].reshape(2, fb), None, 2)


def test_cli_writes_the_host_writers_file(csic, tmp_path, capsys):
    """compress --rows --coding rans on in512.png: the device pipeline's file is the host writer's, byte for byte; decompress gives the
    PNG of the file written without --rows; inspect names the layer."""
    png = os.path.join(GOLDEN, "inputs", "in512.png")
    common = ["--a", "2", "--b", "0", "--yq", "6", "--cbq", "5", "--crq", "5", "--sf", "1", "--op1", "chroma", "--op2", "spatial", "--op3", "color"]
    with_rows, plain, host = str(tmp_path / "rows.csic"), str(tmp_path / "plain.csic"), str(tmp_path / "host.csic")
    assert csic.app.main(["compress", "--input", png, "--output", with_rows, "--coding", "rans", "--rows"] + common) == 0
    assert csic.app.main(["compress", "--input", png, "--output", plain, "--coding", "rans"] + common) == 0
    info = csic.container_info(with_rows)
    assert (info.version, info.nframes, info.rows, info.coding) == (8, 1, True, csic._native.CODING_RANS)
    assert os.path.getsize(with_rows) < os.path.getsize(plain)
    cp, _, frames = csic.read_container(with_rows)
    assert np.array_equal(frames, csic.read_container(plain)[2])
    csic.write_container(host, cp, frames, coding="rans", rows=True)
    assert open(host, "rb").read() == open(with_rows, "rb").read()
    a, b = str(tmp_path / "a.png"), str(tmp_path / "b.png")
    assert csic.app.main(["decompress", "--input", with_rows, "--output", a]) == 0
    assert csic.app.main(["decompress", "--input", plain, "--output", b]) == 0
    assert open(a, "rb").read() == open(b, "rb").read()
    capsys.readouterr()
    assert csic.app.main(["inspect", "--input", with_rows]) == 0
    text = capsys.readouterr().out
    assert "version 8" in text and "coding: rans, row prediction" in text and "groups (" in text and "predicted from the row above" in text
    # out of scope: refused, not half-built
    for extra in (["--gop", "2"], ["--motion", "1"], ["--target-bytes", "100000"]):
        assert csic.app.main(["compress", "--input", png, "--output", host, "--coding", "rans", "--rows"] + extra + common) == 2
    assert csic.app.main(["compress", "--input", png, "--output", host, "--coding", "raw", "--rows"] + common) == 2
    assert csic.app.main(["compress", "--inputs", png, "--output", host, "--coding", "rans", "--rows"] + common) == 2
