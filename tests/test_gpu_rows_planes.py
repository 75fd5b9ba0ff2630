"""The device codec of the row-prediction layer (csic_rows.hip: k_rows, k_unrows) on the planes built to order of
tests/rows_planes.py, whose conditions tests/test_rows_planes_host.py proves without a GPU, against the numpy statement of
tests/rows_ref.py -- the host codec is a second witness.  Every comparison is byte for byte:

    every q = 1 .. 8 with every delta = 0 .. 31     all 44 <Q, WS> paths of rw_shift, bits = 0 included, on contest planes (every group
                                                    a tie or decided by one, a ragged tail, the band-second groups) and the extremes
    G = 32, 33, 64, 65, 256, 257                    a full map dword and one bit more, both halves of a ballot, one block of k_rows and
                                                    one lane into a second; with delta = 0 and with delta = 1
    K = 256, 257 with delta = 0 and 1               the lane loop of k_unrows: one pass, and one lane in a second pass
    planes of one frame on different paths          register walk beside barrier walk, and a K = 0 plane of two workgroups of the copy
                                                    path beside a live Y of 65 bands; in one launch (8/8/8) and in two (6/5/5)
    k_unrows on D and maps that no encoder wrote    random codes, random bits, set padding bits and set bits of K = 0 sections
    the bytes between the planes                    0x00, 0xEE, 0xFF in the source: the same payload and maps

Per case: difference frames and maps equal ref_rows with 0xEE outside the payload ranges and behind map_bytes, the source only read,
unrows restores it apart and in place, the host codec writes the same bytes.  Run with `-m gpu` on an MI355X."""
import functools

import numpy as np
import pytest

from delta_ref import frame_buffers, map_buffers
from rows_planes import band_second_plane, built_frames, contest_plane, plan_bits
from rows_ref import ref_rows, ref_unrows
from test_gpu_pack import EE, _filled, _plan
from test_gpu_rows import _host, _plane

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    assert csic_amd._native.lib().csic_device_count() >= 1
    return csic_amd


def _dims(pl):
    g = pl.planar_bits_layout.geometry
    return [(g.y_width, g.y_height), (g.chroma_width, g.chroma_height), (g.chroma_width, g.chroma_height)]


def _check(csic, W, H, a, b, bits, content, nt=1, fill=EE, facts=None):
    """The frames content(dims) -- or the list `content` -- through k_rows and k_unrows against ref_rows.  -> (diff, maps) as numpy."""
    import torch
    tag = (W, H, a, b, bits, nt, fill)
    with _plan(csic, W, H, a, b, bits) as pl:
        if not nt:
            pl.tune(csic._native.TUNE_NONTEMPORAL, 0)
        assert pl.rows_kernel_name == "k_rows<q%d,%d,%d,%s>" % (*bits, "nt" if nt else "cached")
        lay, ml, fb = pl.planar_bits_layout, pl.rows_layout, pl.frame_bytes
        widths = [int(w) for w in ml.width]
        assert widths == [w for w, _ in _dims(pl)] and [int(k) for k in ml.k] == [w // 32 for w in widths], tag
        if facts is not None:
            facts(ml)
        frames = content(_dims(pl)) if callable(content) else content
        nframes = len(frames)
        ref = [ref_rows(f, widths, bits) for f in frames]
        src, plain = frame_buffers(lay, frames, bits, fill), frame_buffers(lay, frames, bits, EE)
        want_d, want_m = frame_buffers(lay, [r[0] for r in ref], bits, EE), map_buffers([r[1] for r in ref], ml.map_stride, EE)
        d_src = torch.from_numpy(src).cuda()
        diff, maps = pl.rows_device(d_src, nframes, _filled((nframes, fb)), _filled((nframes, ml.map_stride)))
        got_d, got_m = diff.cpu().numpy(), maps.cpu().numpy()
        assert np.array_equal(got_m, want_m), tag                              # map_bytes, and 0xEE behind them
        assert np.array_equal(got_d, want_d), tag                              # the payload ranges, and 0xEE outside them
        assert np.array_equal(d_src.cpu().numpy(), src), tag                   # the source is only read
        back = pl.unrows_device(diff, maps, nframes, _filled((nframes, fb)))
        assert np.array_equal(back.cpu().numpy(), plain), tag                  # apart: the payload restored, 0xEE kept
        work = diff.clone()
        assert pl.unrows_device(work, maps, nframes, work) is work and np.array_equal(work.cpu().numpy(), plain), tag     # in place
        host_d, host_m = _host(csic, pl, src)
        assert np.array_equal(host_d, want_d) and np.array_equal(host_m, want_m), tag
    return got_d, got_m


# ---- every path of the shift ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", range(1, 9))
def test_every_width_and_delta(csic, q):
    """The 32 plans of built_frames(q, .), (32 + delta) x 19: q in the Y plane, delta q bits of shift."""
    for delta in range(32):
        bits, frames = built_frames(q, delta)
        _check(csic, 32 + delta, 19, 4, 4, bits, frames)


@pytest.mark.parametrize("q", range(1, 9))
def test_cached_variants(csic, q):
    for delta in (0, 1, 17, 31):
        bits, frames = built_frames(q, delta)
        _check(csic, 32 + delta, 19, 4, 4, bits, frames, nt=0)


# ---- group, wave and block edges --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _contest(w, H, q):
    return contest_plane(w, H, q, np.random.default_rng(24000 + 1000 * q + 7 * w + H))


def _contest_frame(w, H, bits):
    """Three different planes of contest content: one built plane per bit width, a plane that shares its width with an earlier one is
    that plane plus a constant -- u stays what it is wherever there is a reference, so do the relations."""
    planes = []
    for p, q in enumerate(bits):
        planes.append((_contest(w, H, q) + 37 * bits[:p].count(q)) % (1 << q))
    return planes


@pytest.mark.parametrize("w,H,G", [(32, 32, 32), (32, 33, 33), (32, 64, 64), (32, 65, 65), (32, 256, 256), (32, 257, 257),
                                   (33, 31, 32), (33, 32, 33), (33, 62, 64), (33, 63, 65), (33, 248, 256), (33, 249, 257)])
def test_group_wave_and_block_edges(csic, w, H, G):
    def facts(ml):
        assert list(ml.groups) == [G] * 3 and list(ml.k) == [1] * 3
    for bits in ((8, 8, 8), (6, 5, 5)):
        _check(csic, w, H, 4, 4, bits, [_contest_frame(w, H, bits)], facts=facts)


# ---- the lane loop ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,bits", [(8192, (8, 8, 8)), (8224, (6, 5, 5)), (8193, (3, 7, 2)), (8225, (1, 8, 4))])
def test_lane_loop_edges(csic, w, bits):
    """K = 256: one pass of `for (k = t; k < K; k += 256)`; K = 257: lane 0 takes a second one.  18 rows: a band of 16 steps and one of
    2 (and a group, where delta = 1).  Sparse-noise rows with the band-second groups set."""
    rng = np.random.default_rng(24100 + w)

    def facts(ml):
        assert list(ml.k) == [w // 32] * 3 and [-(-g // (16 * k)) for g, k in zip(ml.groups, ml.k)] == [2] * 3
    _check(csic, w, 18, 4, 4, bits, [[band_second_plane(w, 18, q, rng) for q in bits]], facts=facts)


# ---- planes of one frame on different paths ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [(8, 8, 8), (6, 5, 5)])
@pytest.mark.parametrize("W,H,a,b,widths,ks,bands", [
    (160, 40, 1, 1, [160, 40, 40], [5, 1, 1], [3, 4, 4]),                      # the register walk beside the barrier walk (delta = 8)
    (66, 36, 2, 2, [66, 33, 33], [2, 1, 1], [3, 3, 3]),                        # delta = 2 beside delta = 1
    (62, 532, 2, 0, [62, 31, 31], [1, 0, 0], [65, 2, 2])])                     # 65 bands beside two workgroups of the copy path
def test_planes_on_different_paths(csic, W, H, a, b, widths, ks, bands, bits):
    """At 8/8/8 the three planes are one launch whose grid x is the largest workgroup count of the three; at 6/5/5 they are two."""
    rng = np.random.default_rng(24200 + W + bits[0])

    def facts(ml):
        assert list(ml.width) == widths and list(ml.k) == ks
        assert [-(-g // (16 * k if k else 256)) for g, k in zip(ml.groups, ml.k)] == bands
    _check(csic, W, H, a, b, bits, lambda dims: [[_plane(w, h, q, rng) for (w, h), q in zip(dims, bits)] for _ in range(3)], facts=facts)


# ---- k_unrows on what no encoder wrote --------------------------------------------------------------------------------------------
def _unrows_case(csic, W, H, a, b, bits, nframes, rng):
    """D is random codes.  First maps of random bits -- padding bits and the sections of planes with K = 0 included, which the device
    ignores and the host refuses: numpy alone is the reference --, then the same maps with those bits cleared: numpy and the host."""
    import torch
    tag = (W, H, a, b, bits)
    with _plan(csic, W, H, a, b, bits) as pl:
        lay, ml, fb = pl.planar_bits_layout, pl.rows_layout, pl.frame_bytes
        widths = [int(w) for w in ml.width]
        D = [[rng.integers(0, 1 << q, w * h).astype(np.int64) for (w, h), q in zip(_dims(pl), bits)] for _ in range(nframes)]
        d_buf = frame_buffers(lay, D, bits, EE)
        wild = [rng.integers(0, 256, ml.map_bytes, dtype=np.uint8) for _ in range(nframes)]
        ignored = np.zeros(8 * ml.map_bytes, dtype=bool)                       # the bits that the device does not look at
        for p in range(3):
            first = 8 * ml.map_offset[p] + (ml.groups[p] if ml.k[p] else 0)
            ignored[first:8 * ml.map_offset[p] + 32 * ((ml.groups[p] + 31) // 32)] = True
        keep = np.packbits(~ignored, bitorder="little")
        assert ignored.any() == any(g % 32 != 0 or k == 0 for g, k in zip(ml.groups, ml.k)), tag
        wild[0] |= ~keep                                                       # every one of them set in frame 0, random ones behind it
        for maps, valid in (([m.tobytes() for m in wild], False), ([(m & keep).tobytes() for m in wild], True)):
            want = frame_buffers(lay, [ref_unrows(d, m, widths, bits) for d, m in zip(D, maps)], bits, EE)
            m_buf = map_buffers(maps, ml.map_stride, EE)
            d_diff, d_maps = torch.from_numpy(d_buf).cuda(), torch.from_numpy(m_buf).cuda()
            back = pl.unrows_device(d_diff, d_maps, nframes, _filled((nframes, fb)))
            assert np.array_equal(back.cpu().numpy(), want), (tag, valid)     # apart
            assert np.array_equal(d_diff.cpu().numpy(), d_buf) and np.array_equal(d_maps.cpu().numpy(), m_buf), (tag, valid)
            work = d_diff.clone()
            assert pl.unrows_device(work, d_maps, nframes, work) is work and np.array_equal(work.cpu().numpy(), want), (tag, valid)
            if valid:
                assert np.array_equal(csic.unrows_host(pl.c_params, d_buf, m_buf, out=np.full_like(d_buf, EE)), want), tag
        assert not np.array_equal(want, d_buf), tag


@pytest.mark.parametrize("shapes", ["every_delta", "copy_path", "lane_loop"])
def test_unrows_on_maps_built_to_order(csic, shapes):
    rng = np.random.default_rng(24300 + len(shapes))
    if shapes == "every_delta":                                                # one q per delta, two others beside it; 3 bands
        for delta in range(32):
            _unrows_case(csic, 32 + delta, 35, 4, 4, plan_bits(delta % 8 + 1), 2, rng)
    elif shapes == "copy_path":                                                # chroma: K = 0, 258 groups -- every bit of it ignored
        _unrows_case(csic, 62, 532, 2, 0, (8, 8, 8), 2, rng)
        _unrows_case(csic, 62, 532, 2, 0, (6, 5, 5), 2, rng)
    else:                                                                      # K = 257, delta = 1
        _unrows_case(csic, 8225, 18, 4, 4, (7, 4, 2), 1, rng)


# ---- the bytes between the planes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", range(1, 9))
def test_fill_independence(csic, q):
    delta = 4 * q - 3
    bits, frames = built_frames(q, delta)
    got = [_check(csic, 32 + delta, 19, 4, 4, bits, frames[:1], fill=fill) for fill in (0x00, EE, 0xFF)]
    assert all(np.array_equal(d, got[0][0]) and np.array_equal(m, got[0][1]) for d, m in got[1:])
