"""tests/plane_frames.py before it is trusted, without a GPU: ref_pixels against the oracle's sample-by-sample replay of the chroma latch
(oracle.planar_reconstruct) through frame_of and the library's own unpackers, the whole 8 / 8 / 8 cube against the pinned digest of the
inverse transform, the conditions the plane builders and the case list of tests/test_gpu_plane_frames.py promise, and the fills."""
import hashlib
import itertools

import numpy as np
import pytest

from plane_frames import (ARGB, AVG_SHAPES, BITS, INVERSE_CUBE_DIGEST, CHROMA, CSQ, PLANAR, SHAPES, TRIPLES, YCC, bits_of, chroma_sample_index, clamps_fired,
                          combos, cube_planes, cube_shape, extreme_planes, frame_of, host_plan, index_planes, pack_codes, random_planes, ref_decode,
                          ref_pixels, regions, sample_counts, slice_layout, unowned, values_of)

ORDERS = list(itertools.permutations((1, 2, 3)))
MODES = [(4, 4), (2, 2), (2, 0), (1, 1), (4, 0), (1, 0)]


def _oracle_layout(oracle, W, H, a, b, bits, f, op, avg):
    return oracle.planar_layout(oracle.OracleParams(width=W, height=H, chroma_a=a, chroma_b=b, y_bits=bits[0], cb_bits=bits[1], cr_bits=bits[2],
                                                    factor=f, op=op), avg)


def _unpacked(plan, fmt, frame):
    return plan.unpack_planar_bits(frame) if fmt == BITS else plan.split_planar(frame)


@pytest.mark.parametrize("W,H", [(64, 40), (37, 21), (30, 34), (5, 3), (1, 1)])
def test_ref_pixels_equals_the_oracles_replay(oracle, W, H):
    """All 6 orders x 6 chroma modes x 4 factors under HOLD, 6 modes x 4 factors under AVG, random planes: frame_of -> the library's
    unpacker -> ref_pixels equals oracle.planar_reconstruct of the same values, in both output formats; a PLANAR frame with random
    low bits gives its raw bytes to both."""
    rng = np.random.default_rng(4100 + W)
    sets = [(a, b, f, op, False) for (a, b), f, op in itertools.product(MODES, (1, 2, 4, 8), ORDERS)]
    sets += [(a, b, f, CSQ, True) for (a, b), f in itertools.product(MODES, (1, 2, 4, 8))]
    replayed = 0
    for i, (a, b, f, op, avg) in enumerate(sets):
        bits = TRIPLES[i % len(TRIPLES)]
        plan = host_plan(W, H, a, b, bits, f, op, avg)
        olay = _oracle_layout(oracle, W, H, a, b, bits, f, op, avg)
        lay = plan.planar_layout
        for name in ("y_width", "y_height", "chroma_width", "chroma_height", "module_width", "hold_h", "hold_v", "replay_last", "chroma_samples"):
            assert getattr(lay, name) == getattr(olay, name), (name, W, H, a, b, f, op, avg)
        replayed += bool(lay.replay_last and lay.hold_v > 1 and lay.y_width * lay.y_height > lay.module_width)
        planes = random_planes(plan, int(rng.integers(1 << 30)))
        for fmt, low in ((BITS, None), (PLANAR, None), (PLANAR, rng)):
            frame = frame_of(plan, fmt, *planes, fill=rng, low_bits=low)
            y8, cb8, cr8 = _unpacked(plan, fmt, frame)
            if low is None:
                assert all(np.array_equal(np.asarray(g).reshape(-1), v) for g, v in zip((y8, cb8, cr8), values_of(planes, bits)))
            for o in (ARGB, YCC):
                want = oracle.planar_reconstruct(olay, y8, cb8, cr8, o)
                assert np.array_equal(ref_pixels(lay, y8, cb8, cr8, o), want), (W, H, a, b, bits, f, op, avg, fmt, o)
    assert replayed or H == 1


def test_the_whole_cube_reproduces_the_pinned_digest():
    W, H = cube_shape((8, 8, 8))
    assert (W, H) == (256, 65536)
    px = ref_pixels(slice_layout(1 << 24), *cube_planes((8, 8, 8)), ARGB).reshape(-1)
    assert (px >> 24 == 0xFF).all()
    rgb = np.stack([(px >> 16) & 255, (px >> 8) & 255, px & 255], -1).astype(np.uint8)
    assert hashlib.sha256(rgb.tobytes()).hexdigest() == INVERSE_CUBE_DIGEST
    y, cb, cr = (c[-65536:] for c in cube_planes((8, 8, 8)))
    assert np.array_equal(ref_pixels(slice_layout(65536), y, cb, cr, YCC).reshape(-1), (y | cb << 8 | cr << 16).astype(np.uint32))


@pytest.mark.parametrize("bits", [(6, 5, 5), (3, 3, 2), (5, 6, 5), (8, 4, 4), (8, 8, 8)])
def test_a_cube_holds_every_triple_once(bits):
    y, cb, cr = cube_planes(bits)
    W, H = cube_shape(bits)
    assert y.size == cb.size == cr.size == W * H == 1 << sum(bits)
    assert y.max() == (1 << bits[0]) - 1 and cb.max() == (1 << bits[1]) - 1 and cr.max() == (1 << bits[2]) - 1
    key = (y << (bits[1] + bits[2])) | (cb << bits[2]) | cr
    assert np.array_equal(np.sort(key), np.arange(1 << sum(bits)))
    plan = host_plan(W, H, 4, 4, bits)                                  # 4:4:4 at factor 1: one chroma sample per position
    assert sample_counts(plan) == (W * H,) * 3
    assert np.array_equal(chroma_sample_index(plan.planar_layout, np.arange(W * H)), np.arange(W * H))
    for f in (2, 4, 8):                                                 # the same planes under a plan whose OUTPUT is the cube's
        big = host_plan(W * f, H * f, 4, 4, bits, f)
        assert sample_counts(big) == (W * H,) * 3 and (big.planar_layout.y_width, big.planar_layout.y_height) == (W, H)
        assert regions(big, BITS) == regions(plan, BITS) and regions(big, PLANAR) == regions(plan, PLANAR)


def test_every_clamp_fires_on_the_655_cube():
    bits = (6, 5, 5)
    assert clamps_fired(*values_of(cube_planes(bits), bits)) == {"r_lo", "r_hi", "g_lo", "g_hi", "b_lo", "b_hi"}
    assert clamps_fired([128], [128], [128]) == set() and clamps_fired([200], [128], [255]) == {"r_hi"}


def test_index_and_extreme_planes():
    plan = host_plan(64, 40, 2, 0, (3, 8, 2))
    y, cb, cr = index_planes(plan)
    n, cs, _ = sample_counts(plan)
    assert (n, cs) == (2560, 640)
    assert (np.diff(y) % 8 == 1).all() and (np.diff(cb) % 256 == 1).all() and cr.tolist() == [k >> 8 for k in range(cs)]
    # no two samples of the frame carry the same (cb, cr): a wrong chroma index is a wrong pixel
    assert np.unique(cb * 4 + cr).size == cs
    zero, ones, alt = extreme_planes(plan)
    assert not any(c.any() for c in zero) and [int(c.min()) for c in ones] == [7, 255, 3]
    assert [c[:4].tolist() for c in alt] == [[0, 7, 0, 7], [0, 255, 0, 255], [0, 3, 0, 3]]
    assert all(not c.flags.writeable for c in (y, cb, cr) + zero + ones + alt)
    assert all(np.array_equal(p, q) for p, q in zip(random_planes(plan, 5), random_planes(plan, 5)))
    assert not np.array_equal(random_planes(plan, 5)[0], random_planes(plan, 6)[0])


def _plans():
    for W, H, f in SHAPES:
        for a, b, op in combos(W, H, f):
            for bits in TRIPLES:
                yield (W, H, f, a, b, op, bits), host_plan(W, H, a, b, bits, f, op)
    for W, H, f in AVG_SHAPES:
        for a, b in CHROMA:
            for bits in TRIPLES:
                yield (W, H, f, a, b, CSQ, bits, "avg"), host_plan(W, H, a, b, bits, f, CSQ, True)


def test_the_case_list_holds_what_it_promises():
    seen = set()
    mid_byte, on_dword = set(), set()
    for key, plan in _plans():
        g = plan.planar_layout
        n, cs, _ = sample_counts(plan)
        rows = -(-n // g.module_width)
        if g.replay_last and g.hold_v > 1 and rows > 1:
            seen |= {"sample row", "replayed row"}
        if not g.replay_last and g.hold_v == 2:
            seen.add("box rows")
        if cs < g.chroma_width * g.chroma_height:
            seen.add("partial last chroma row")
        if g.module_width % 4:
            seen.add("module width % 4 != 0")
        seen.add(f"tail {n % 4}")
        lay = plan.planar_bits_layout
        for s, q in zip((n, cs, cs), bits_of(plan)):
            if (s * q) % 8:
                mid_byte.add(q)
            if (s * q) % 32 == 0:
                on_dword.add(q)
        if lay.cr_bytes % 256 == 0:
            seen.add("the last sample dword is the frame's last")
            assert lay.cr_offset + lay.cr_bytes == lay.frame_bytes
    assert seen >= {"sample row", "replayed row", "box rows", "partial last chroma row", "module width % 4 != 0", "tail 1", "tail 2", "tail 3",
                    "the last sample dword is the frame's last"}, seen
    # a plane of 8-bit codes cannot end inside a byte; every other width does somewhere, and every width ends on a dword somewhere
    assert mid_byte == set(range(1, 8)) and on_dword == set(range(1, 9))
    assert {q for bits in TRIPLES for q in bits} == set(range(1, 9))


def test_the_three_fills_differ_in_every_unowned_region():
    checked = set()
    for key, plan in _plans():
        planes = random_planes(plan, 77)
        for fmt in (PLANAR, BITS):
            frames = [frame_of(plan, fmt, *planes, fill=fill) for fill in (0x00, 0xFF, np.random.default_rng(4300))]
            own = np.ones(frames[0].size, dtype=np.uint8) * 0xFF
            for name, (idx, mask) in unowned(plan, fmt).items():
                parts = [f[idx] & mask for f in frames]
                assert not parts[0].any() and (parts[1] == mask).all(), (key, fmt, name)
                if idx.size >= 8:                                       # (a random byte equals 0x00 or 0xFF once in 128)
                    assert not np.array_equal(parts[2], parts[0]) and not np.array_equal(parts[2], parts[1]), (key, fmt, name)
                own[idx] &= ~np.uint8(mask)
                checked.add((fmt, name.split(".")[1]))
            # and nowhere else: what the format owns is the same in all three
            assert np.array_equal(frames[0] & own, frames[1] & own) and np.array_equal(frames[0] & own, frames[2] & own), (key, fmt)
            back = [np.asarray(v).reshape(-1) for v in _unpacked(plan, fmt, frames[2])]
            assert all(np.array_equal(g, v) for g, v in zip(back, values_of(planes, bits_of(plan)))), (key, fmt)
    assert checked == {(PLANAR, "padding"), (PLANAR, "row_tail"), (BITS, "padding"), (BITS, "row_tail"), (BITS, "high_bits")}


def test_low_bits_and_the_packer():
    plan = host_plan(5, 3, 4, 4, (3, 8, 2))
    planes = random_planes(plan, 9)
    zeros, ones, rnd = (frame_of(plan, PLANAR, *planes, fill=0, low_bits=lb) for lb in ("zeros", "ones", np.random.default_rng(1)))
    assert np.array_equal(frame_of(plan, PLANAR, *planes, fill=0), zeros)
    y0, y1, y2 = (plan.split_planar(f)[0].reshape(-1) for f in (zeros, ones, rnd))
    assert np.array_equal(y0, planes[0] << 5) and np.array_equal(y1, (planes[0] << 5) | 31) and np.array_equal(y2 >> 5, planes[0])
    assert (y2 & 31).any() and np.array_equal(plan.split_planar(ones)[1], plan.split_planar(zeros)[1])          # 8 bits: nothing below
    assert pack_codes(np.array([1, 2, 3, 4, 5, 6, 7, 0]) << 5, 3).tobytes().hex() == "d1581f"
    small = np.arange(6, dtype=np.uint32).reshape(2, 3)
    assert ref_decode(small, 5, 3, 2).tolist() == [[0, 0, 1, 1, 2], [0, 0, 1, 1, 2], [3, 3, 4, 4, 5]]
