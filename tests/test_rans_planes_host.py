"""The planes of tests/rans_planes.py meet their conditions: proved here with the numpy statement of the rANS coding alone
(tests/test_rans_host.py), then each plane goes through the host codec as the Y plane of a frame (check_frame: byte for byte, both
directions).  No GPU."""
import numpy as np
import pytest

from rans_planes import built_planes
from test_container import CSQ, _c_params
from test_pack_host import ref_groups
from test_rans_host import BLOCK, LANES, M, STEPS, check_frame, raw_dwords, ref_rans_plane, ref_scale


@pytest.fixture(scope="module")
def planes():
    return built_planes()


def _coded(plane):
    q, codes = plane
    u = ref_groups(codes, q)[2]
    trace = []
    f, blocks = ref_rans_plane(u, q, trace)
    return q, u, f, blocks, trace


def test_constant_plane_has_one_frequency_and_empty_word_strings(planes):
    q, u, f, blocks, _ = _coded(planes["constant"])
    assert f.tolist() == [M] + [0] * ((1 << q) - 1) and (planes["constant"][1].size % 32) != 0
    assert [(raw, len(chunk), words) for raw, chunk, words in blocks] == [(False, 4 * LANES, 0)]


def test_two_symbol_planes(planes):
    q, u, f, blocks, _ = _coded(planes["two_symbols"])
    assert np.flatnonzero(f).tolist() == [0, 2] and len(blocks) == 2 and not any(raw for raw, _, _ in blocks)
    q, u, f, blocks, _ = _coded(planes["one_bit"])
    assert q == 1 and np.all(f > 0) and len(blocks) == 1


def test_skewed_plane_takes_the_negative_remainder_path(planes):
    q, u, f, blocks, _ = _coded(planes["skewed"])
    c = np.bincount(u[:, 1:].reshape(-1), minlength=256)
    assert c[0] == 31 * BLOCK - 250 and np.all(c[1:251] == 1) and np.all(c[251:] == 0)
    floors = np.where(c > 0, np.maximum(1, c * M // c.sum()), 0)
    assert floors.sum() - M > 100                              # the sum overshoots: the excess comes off the largest f, one at a time
    assert f[0] == floors[0] - (floors.sum() - M) and np.all(f[1:251] == 1) and np.array_equal(f, ref_scale(c))
    assert not blocks[0][0]


def test_noise_block_plane_has_one_raw_block_among_rans_blocks(planes):
    q, u, f, blocks, _ = _coded(planes["noise_block"])
    assert [raw for raw, _, _ in blocks] == [False, True, False]
    assert len(blocks[1][1]) == 4 * raw_dwords(BLOCK, q) and all(len(chunk) < 4 * raw_dwords(BLOCK, q) for raw, chunk, _ in blocks if not raw)


def test_noise_plane_is_raw_throughout(planes):
    q, u, f, blocks, _ = _coded(planes["noise"])
    assert len(blocks) == 2 and all(raw for raw, _, _ in blocks)


def test_words_at_the_first_and_at_the_latest_step(planes):
    """A stream's last decode step is the encoder's first, from x = L < f << 20: no stream takes a word there, so 494 is the latest
    step with a word; step 0 takes one when the encoder emits before its last symbol."""
    for name in planes:
        for words in _coded(planes[name])[4]:
            assert all(t < STEPS - 1 for t, _ in words)
    late = _coded(planes["late_word"])[4][0]
    assert (STEPS - 2, 5) in late
    early = _coded(planes["early_word"])[4][0]
    assert (0, 7) in early and early[0] == (0, 7)


@pytest.mark.parametrize("name", sorted(built_planes()))
def test_host_codec_on_every_plane(planes, name):
    q, codes = planes[name]
    bits = (q, 3, 2)
    rng = np.random.default_rng(len(name))
    cp = _c_params(codes.size, 1, 4, 4, bits, 1, CSQ)
    check_frame(cp, [codes] + [rng.integers(0, 1 << b, codes.size).astype(np.int64) for b in bits[1:]], bits)
