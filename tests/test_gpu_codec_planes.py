"""Both device codecs -- the group coding (csic_pack.hip) and the Rice coding (csic_rice.hip) -- on code planes built to order
(tests/codec_planes.py; their conditions are proved on the CPU in tests/test_codec_planes_host.py).  The PLANAR_BITS frame is built on
the host and uploaded, so what the kernels see does not depend on the colour transform or the quantiser.  The comparison is the one of
tests/test_gpu_pack.py and tests/test_gpu_rice.py (_compare): coded bytes and sizes equal to the numpy statement of the formats, 0xEE
behind coded_bytes, unpack into a 0xEE-filled buffer restores the source byte for byte.  Where to find the case for each edge:

  test_runs_and_shuffled_frames   every mode (15, k = 0 .. q but q - 1) and every width w = 0 .. q of every q, as the Y plane and as a
                                  chroma plane, three per-width launches (plane0 = 0, 1, 2) and the shared launches of (8, 8, 8) and
                                  (5, 5, 3); blocks of 256 groups of one mode: lane t's run starts at bit 31 k t, every residue mod 32,
                                  and at k = 1 a run that never fills a dword (RcWriter::finish alone writes it, the shared-dword
                                  atomicOr on both sides); a batch of two frames; pk_store_sections and k_pack_emit / k_unpack_emit on
                                  every width.
  test_long_unary_runs            runs of 62 zeros at q = 6, 7, 8 (k = 0, 1, 2): the second turn of the loop in RcWriter::unary, a
                                  dword of U without a terminator, the plateau of s_cum that rice_after_terminator steps over.
  test_full_and_empty_chunks      chunks of exactly 248 q + 1 dwords -- the last element of s_chunk and s_cum, the edge of
                                  CSIC_CHECK(ndw <= RcCap<Q>::DW) -- around an empty chunk (dir[b] == dir[b + 1]).
  test_foreign_streams_unpack     valid streams that the encoders here never write: every group at k = 0 .. q, k = q - 1 among them, a
                                  run of 2^q - 1 zeros (255 at q = 8, the clamp of rice_next_u); groups stored wider than necessary.
                                  Only streams that the host decoders accepted are shown to the device; damaged ones are not (the
                                  clamps: tests/test_cpp_rice.py, tests/test_cpp_pack.py).
  test_cached_variants            the TUNE_NONTEMPORAL = 0 instantiations (k_pack<.., cached>, k_rice<.., cached>) on a ragged frame and
                                  on full and empty chunks: the same bytes as the non-temporal run and as the reference.
Random parameter sets (AVG, rounding, f = 8, the stage orders) are test_random_sets_vs_numpy of the two codecs' own modules.
Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

from codec_planes import (BLOCK, SHUFFLED_N, TRIPLES, foreign_frames, full_chunk_dwords, full_chunk_frame, long_run_groups, modes_of, planes_for,
                          reachable_modes, runs_frame, shuffled_frame, widths_of)
from test_container import _frame_buffer
from test_gpu_pack import EE, _compare, _filled, _plan
from test_pack_host import plane_bytes, ref_encode
from test_rice_host import ref_encode_rice

pytestmark = pytest.mark.gpu

QS = range(1, 9)


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    assert csic_amd._native.lib().csic_device_count() >= 1
    return csic_amd


class Groups:
    name = "groups"
    encode = staticmethod(ref_encode)
    layout = staticmethod(lambda pl: pl.pack_layout)
    pack = staticmethod(lambda pl, *a: pl.pack_device(*a))
    unpack = staticmethod(lambda pl, *a: pl.unpack_device(*a))
    kernel = staticmethod(lambda pl: pl.pack_kernel_name)


class Rice:
    name = "rice"
    encode = staticmethod(ref_encode_rice)
    layout = staticmethod(lambda pl: pl.rice_layout)
    pack = staticmethod(lambda pl, *a: pl.rice_pack_device(*a))
    unpack = staticmethod(lambda pl, *a: pl.rice_unpack_device(*a))
    kernel = staticmethod(lambda pl: pl.rice_kernel_name)


CODECS = (Groups, Rice)


def _host_frames(pl, frames, bits):
    """The PLANAR_BITS frame buffers of `frames` (three planes of codes each), built on the host: 0xEE between the planes, zero in
    the unused high bits of a plane's last byte.  uint8 (nframes, frame_bytes)."""
    lay = pl.planar_bits_layout
    return np.stack([_frame_buffer(lay, [plane_bytes(c, q) for c, q in zip(planes, bits)], EE) for planes in frames])


def _unpack(pl, codec, coded, nframes):
    import torch
    back = codec.unpack(pl, coded, nframes, _filled((nframes, pl.frame_bytes)))
    torch.cuda.synchronize()
    return back.cpu().numpy().reshape(nframes, -1)


def _roundtrip(pl, codec, buf, nframes):
    import torch
    coded, sizes = codec.pack(pl, buf, nframes, _filled((nframes, codec.layout(pl).bound_bytes)))
    torch.cuda.synchronize()
    return coded.cpu().numpy(), sizes.cpu().numpy(), _unpack(pl, codec, coded, nframes)


def _check(pl, frames, bits, wants=None):
    """`frames` through both device codecs of plan `pl` against numpy.  -> {codec name: (the reference's coded frames, the device's)};
    `wants` takes the first from an earlier call."""
    import torch
    host = _host_frames(pl, frames, bits)
    buf = torch.from_numpy(host).cuda()
    out = {}
    for codec in CODECS:
        tag = (codec.kernel(pl), frames[0][0].size, bits)
        want = wants[codec.name][0] if wants else [codec.encode(planes, bits) for planes in frames]
        coded, sizes, back = _roundtrip(pl, codec, buf, len(frames))
        assert np.array_equal(buf.cpu().numpy(), host), tag                  # the source is only read
        _compare(tag, pl.planar_bits_layout, bits, frames, host, coded, sizes, back, codec.layout(pl).bound_bytes, want)
        out[codec.name] = (want, coded)
    return out


def _planes_plan(csic, frames, bits):
    n = frames[0][0].size
    assert all(c.size == n and c.max() < (1 << q) for planes in frames for c, q in zip(planes, bits))
    pl = _plan(csic, n, 1, 4, 4, bits)
    g = (n + 31) // 32
    assert list(pl.rice_layout.groups) == [g] * 3 == list(pl.pack_layout.groups) and list(pl.rice_layout.blocks) == [(g + BLOCK - 1) // BLOCK] * 3
    return pl


def _directory(pl, coded_row):
    rl = pl.rice_layout
    return np.frombuffer(coded_row[rl.directory_offset:rl.directory_offset + 4 * (sum(rl.blocks) + 1)].tobytes(), dtype="<u4").astype(np.int64)


# ---- 1. every mode and every width, in runs and shuffled ----------------------------------------------------
@pytest.mark.parametrize("bits", TRIPLES)
def test_runs_and_shuffled_frames(csic, bits):
    runs = planes_for(runs_frame, bits)
    frames = [runs, planes_for(shuffled_frame, bits, runs[0].size)]
    for p, q in enumerate(bits):
        assert modes_of(frames[0][p], q) | modes_of(frames[1][p], q) == set(reachable_modes(q))
        assert widths_of(frames[0][p], q) | widths_of(frames[1][p], q) == set(range(q + 1))
    with _planes_plan(csic, frames, bits) as pl:
        assert pl.rice_kernel_name == "k_rice<q%d,%d,%d,nt>" % bits and pl.pack_kernel_name == "k_pack<q%d,%d,%d,nt>" % bits
        _check(pl, frames, bits)


# ---- 2. long unary runs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", QS)
def test_long_unary_runs(csic, q):
    bits = TRIPLES[q - 1]
    frames = [planes_for(long_run_groups, bits)]
    with _planes_plan(csic, frames, bits) as pl:
        _check(pl, frames, bits)


# ---- 3. the longest chunk and an empty one ----------------------------------------------------------------------
@pytest.mark.parametrize("q", QS)
def test_full_and_empty_chunks(csic, q):
    bits = TRIPLES[q - 1]
    frames = [planes_for(full_chunk_frame, bits)]
    with _planes_plan(csic, frames, bits) as pl:
        assert list(pl.rice_layout.blocks) == [3] * 3
        out = _check(pl, frames, bits)
        d = _directory(pl, out["rice"][1][0])
        for p, qp in enumerate(bits):                          # every plane: full, empty, full
            assert d[3 * p + 1] - d[3 * p] == full_chunk_dwords(qp) == d[3 * p + 3] - d[3 * p + 2], (bits, p, d.tolist())
            assert d[3 * p + 2] == d[3 * p + 1]
        assert bits[0] == q and full_chunk_dwords(q) == (248 * q + 1 if q > 1 else 248) and d[0] == 0


# ---- 4. valid streams of another encoder, unpack only -------------------------------------------------------------
@pytest.mark.parametrize("q", QS)
def test_foreign_streams_unpack(csic, q):
    import torch
    planes, rice_streams, grp_streams = foreign_frames(q)
    bits = (q, q, q)
    with _planes_plan(csic, [planes], bits) as pl:
        src = _host_frames(pl, [planes], bits)[0]
        for codec, streams in ((Rice, rice_streams), (Groups, grp_streams)):
            bound = codec.layout(pl).bound_bytes
            rows = np.full((q + 1, bound), EE, dtype=np.uint8)     # one batch: frame k is the stream of mode / width k
            for k, coded in streams:
                assert len(coded) <= bound
                rows[k, :len(coded)] = np.frombuffer(coded, dtype=np.uint8)
            back = _unpack(pl, codec, torch.from_numpy(rows).cuda(), q + 1)
            for k, _ in streams:
                assert np.array_equal(back[k], src), (codec.name, q, k)


# ---- 5. the cached instantiations -------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", TRIPLES)
def test_cached_variants(csic, bits):
    N = csic._native
    for builder in (shuffled_frame, full_chunk_frame):
        frames = [planes_for(builder, bits)]
        assert builder is not shuffled_frame or frames[0][0].size == SHUFFLED_N
        with _planes_plan(csic, frames, bits) as pl:
            nt = _check(pl, frames, bits)
            pl.tune(N.TUNE_NONTEMPORAL, 0)
            try:
                assert pl.rice_kernel_name == "k_rice<q%d,%d,%d,cached>" % bits and pl.pack_kernel_name == "k_pack<q%d,%d,%d,cached>" % bits
                cached = _check(pl, frames, bits, wants=nt)
                for codec in CODECS:                           # (each run also equals the reference: _check)
                    assert np.array_equal(cached[codec.name][1], nt[codec.name][1]), (codec.name, bits)
            finally:
                pl.tune(N.TUNE_NONTEMPORAL, 1)
            assert pl.rice_kernel_name.endswith(",nt>") and pl.pack_kernel_name.endswith(",nt>")
