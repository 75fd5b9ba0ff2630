"""The Rice coding on the host (csic_rice_layout_of, csic_rice_pack_host, csic_rice_unpack_host; include/csic.h) without a GPU, against a
numpy encoder and decoder written here from the format's text: they share nothing with the library but the groups, anchors and folded
residuals of tests/test_pack_host.py (ref_groups), which the format carries over from the group coding.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_png_rgb
from test_container import CANARY, CSQ, _c_params, _frame_buffer, _layout, _random_sets, pack_codes
from test_pack_host import codes_of, lib_layout, lib_pack, plane_bytes, ref_groups

import csic_amd as csic

N = csic._native
BLOCK = 256


# ---- the definition, in numpy ---------------------------------------------------------------------
def ref_modes(u, q):
    """(G, 32) folded residuals -> the mode nibble of every group: 15, or the cheapest k = 0 .. q, the smallest on a tie."""
    cost = np.stack([31 * k + ((u[:, 1:] >> k) + 1).sum(axis=1) for k in range(q)] + [np.full(u.shape[0], 31 * q)], axis=1)
    m = np.argmin(cost, axis=1)                                # the first minimum: the smallest k
    assert np.all(cost[np.arange(u.shape[0]), m] <= 31 * q)
    return np.where(u[:, 1:].max(axis=1) == 0, 15, m).astype(np.int64)


def _pack_bits(bits):
    """A bit string -> its dwords as bytes, LSB first, zero-padded to a dword."""
    bits = np.concatenate([bits, np.zeros(-bits.size % 32, dtype=np.uint8)])
    return np.packbits(bits, bitorder="little").tobytes()


def ref_chunk(u, m, q):
    """The groups of one block -> (R bits, U bits, number of unary groups)."""
    live = m != 15
    k = np.where(live, m, 0)
    # R: group after group, slot j's k low bits at [(j - 1) k, j k) of the group's run; zero and k = 0 groups contribute nothing
    slot_bits = ((u[:, 1:, None] >> np.arange(8)) & 1).astype(np.uint8)                    # (groups, 31 slots, bit)
    R = slot_bits[np.broadcast_to(np.arange(8)[None, None, :] < k[:, None, None], slot_bits.shape)]
    # U: for each unary group (k < q) in order and j = 1 .. 31, (u_j >> k) zero bits and then the terminator
    unary = live & (m < q)
    v = (u[unary, 1:] >> k[unary, None]).reshape(-1)
    U = np.zeros(int(v.sum()) + v.size, dtype=np.uint8)
    U[np.cumsum(v + 1) - 1] = 1
    return R, U, int(unary.sum())


def ref_rice_layout(ns, bits):
    G = [(n + 31) // 32 for n in ns]
    B = [(g + BLOCK - 1) // BLOCK for g in G]
    msz = [4 * ((g + 7) // 8) for g in G]
    asz = [4 * ((g * q + 31) // 32) for g, q in zip(G, bits)]
    moff = [0, msz[0], msz[0] + msz[1]]
    aoff = [sum(msz), sum(msz) + asz[0], sum(msz) + asz[0] + asz[1]]
    doff = sum(msz) + sum(asz)
    fixed = doff + 4 * (sum(B) + 1)
    top = fixed + 4 * sum(b * (248 * q + 1) for b, q in zip(B, bits))
    return dict(G=G, B=B, moff=moff, aoff=aoff, doff=doff, fixed=fixed, top=top, bound=(top + 255) // 256 * 256)


def ref_encode_rice(planes, bits, info=None, force=None):
    """Three planes of codes -> the coded frame's bytes.  `info` (a list) receives per block (plane, dir, R bits, U bits, unary groups).
    force = k: every group that is not zero takes mode k instead of the cheapest (what another encoder may write)."""
    parts = [ref_groups(c, q) for c, q in zip(planes, bits)]
    modes = [ref_modes(u, q) for (_, _, u), q in zip(parts, bits)]
    if force is not None:
        modes = [np.where(m == 15, 15, force) for m in modes]
    out = b""
    for m in modes:                                            # 1. modes: nibble g at bits [4 g, 4 g + 4)
        nib = np.zeros((m.size + 7) // 8 * 8, dtype=np.uint8)
        nib[:m.size] = m
        out += (nib[0::2] | (nib[1::2] << 4)).astype(np.uint8).tobytes()
    for (_, anchors, _), q in zip(parts, bits):                # 2. anchors, as in the group coding
        a = pack_codes(anchors.astype(np.uint8) << (8 - q), q).tobytes()
        out += a + bytes(-len(a) % 4)
    directory, payload = [], b""
    for p, ((_, _, u), m, q) in enumerate(zip(parts, modes, bits)):
        for g0 in range(0, m.size, BLOCK):                     # 4. one chunk per block: R then U, each padded to a dword
            R, U, z = ref_chunk(u[g0:g0 + BLOCK], m[g0:g0 + BLOCK], q)
            assert R.size + U.size <= 256 * 31 * q or force is not None
            directory.append(len(payload) // 4)
            if info is not None:
                info.append((p, len(payload) // 4, R.size, U.size, z))
            payload += _pack_bits(R) + _pack_bits(U)
    directory.append(len(payload) // 4)                        # 3. directory: NB + 1 uint32
    return out + np.array(directory, dtype="<u4").tobytes() + payload


def ref_decode_rice(coded, ns, bits):
    """Coded bytes -> three planes of codes, by the decode rule: nothing but the modes, the directory and counted terminators."""
    lay = ref_rice_layout(ns, bits)
    raw = np.frombuffer(coded, dtype=np.uint8)
    allbits = np.unpackbits(raw, bitorder="little")
    nb = sum(lay["B"])
    directory = np.frombuffer(coded[lay["doff"]:lay["doff"] + 4 * (nb + 1)], dtype="<u4").astype(np.int64)
    assert directory[0] == 0 and lay["fixed"] + 4 * directory[nb] == len(coded)
    planes, blk = [], 0
    for p, (n, q) in enumerate(zip(ns, bits)):
        G = lay["G"][p]
        out = np.zeros(32 * G, dtype=np.int64)
        mode = lambda g: (int(raw[lay["moff"][p] + g // 2]) >> (4 * (g % 2))) & 15
        for g0 in range(0, G, BLOCK):
            groups = range(g0, min(g0 + BLOCK, G))
            rstart = 8 * (lay["fixed"] + 4 * int(directory[blk]))
            rbits = sum(31 * mode(g) for g in groups if mode(g) != 15)
            ustart = rstart + 32 * ((rbits + 31) // 32)
            ones = np.flatnonzero(allbits[ustart:8 * (lay["fixed"] + 4 * int(directory[blk + 1]))])     # the terminators of U
            rpos, z = rstart, 0
            for g in groups:
                k = mode(g)
                ab = allbits[lay["aoff"][p] * 8 + g * q: lay["aoff"][p] * 8 + g * q + q]
                c = int((ab.astype(np.int64) << np.arange(q)).sum())
                out[32 * g] = c
                at = 0 if z == 0 else int(ones[31 * z - 1]) + 1          # right after terminator number 31 z
                for j in range(1, 32):
                    u = 0
                    if k != 15:
                        rb = allbits[rpos:rpos + k]
                        u = int((rb.astype(np.int64) << np.arange(k)).sum()) if k else 0
                        rpos += k
                        if k < q:
                            t = int(ones[31 * z + j - 1])
                            u |= (t - at) << k
                            at = t + 1
                    assert u < (1 << q)
                    s = u // 2 if u % 2 == 0 else -(u + 1) // 2
                    c = (c + s) % (1 << q)
                    out[32 * g + j] = c
                z += k < q
            assert ones.size == 31 * z
            blk += 1
        planes.append(out[:n])
    return planes


# ---- calling the library ----------------------------------------------------------------------------
def rice_layout(cp):
    lay = N.CsicRiceLayout()
    N.check(N.lib().csic_rice_layout_of(C.byref(cp), C.byref(lay)))
    return lay


def rice_pack(cp, frame, capacity=None, fill=CANARY):
    """-> (status, the whole destination buffer, coded_bytes)"""
    cap = rice_layout(cp).bound_bytes if capacity is None else capacity
    dst = np.full(max(cap, 1), fill, dtype=np.uint8)
    n = C.c_uint64(0)
    st = N.lib().csic_rice_pack_host(C.byref(cp), frame.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    return st, dst, n.value


def rice_unpack(cp, coded, fill=CANARY):
    """-> (status, the whole frame buffer, pre-filled with `fill`)"""
    coded = np.frombuffer(bytes(coded), dtype=np.uint8) if not isinstance(coded, np.ndarray) else coded
    src = np.ascontiguousarray(coded) if coded.size else np.zeros(1, dtype=np.uint8)
    out = np.full(_layout(cp).frame_bytes, fill, dtype=np.uint8)
    st = N.lib().csic_rice_unpack_host(C.byref(cp), src.ctypes.data_as(C.c_void_p), coded.size, out.ctypes.data_as(C.c_void_p))
    return st, out


def check_frame(cp, planes, bits, decode=True):
    """One frame through csic_rice_pack_host and csic_rice_unpack_host against the numpy reference, canaries included."""
    lay, rl = _layout(cp), rice_layout(cp)
    ref = ref_rice_layout([c.size for c in planes], bits)
    assert list(rl.groups) == ref["G"] and list(rl.blocks) == ref["B"] and list(rl.modes_offset) == ref["moff"]
    assert list(rl.anchors_offset) == ref["aoff"] and rl.directory_offset == ref["doff"]
    assert rl.payload_offset == rl.fixed_bytes == ref["fixed"] and rl.bound_bytes == ref["bound"] and rl.bound_bytes % 256 == 0
    assert bytes(csic.rice_layout(cp)) == bytes(rl)
    pbytes = [plane_bytes(c, q) for c, q in zip(planes, bits)]
    want = ref_encode_rice(planes, bits)
    frame = _frame_buffer(lay, pbytes, CANARY)
    st, dst, size = rice_pack(cp, frame)
    assert st == N.OK and size == len(want) and dst[:size].tobytes() == want
    assert rl.fixed_bytes <= size <= ref["top"] <= rl.bound_bytes and np.all(dst[size:] == CANARY)
    assert csic.rice_pack_host(cp, frame).tobytes() == want
    # neither the padding of the source nor the unused high bits of a plane's last byte are read into a value
    other = _frame_buffer(lay, pbytes, 0x11)
    for off, nb, c, q in zip((lay.y_offset, lay.cb_offset, lay.cr_offset), (lay.y_bytes, lay.cb_bytes, lay.cr_bytes), planes, bits):
        if (c.size * q) % 8:
            other[off + nb - 1] |= (0xFF << ((c.size * q) % 8)) & 0xFF
    st, dst2, size2 = rice_pack(cp, other)
    assert st == N.OK and size2 == size and dst2[:size].tobytes() == want
    # the capacity rule: exactly the size suffices, less fails with the size that was needed and writes nothing behind the capacity
    st, dst3, size3 = rice_pack(cp, frame, capacity=size)
    assert st == N.OK and size3 == size and dst3[:size].tobytes() == want
    for cap in {rl.fixed_bytes, size - 4}:
        if rl.fixed_bytes <= cap < size:
            st, dst4, need = rice_pack(cp, frame, capacity=cap)
            assert st == N.EINVAL_SIZE and need == size and np.all(dst4[cap:] == CANARY)
    assert rice_pack(cp, frame, capacity=rl.fixed_bytes - 1)[0] == N.EINVAL_SIZE
    # decode: the payload ranges come back, the canary around them stays
    st, back = rice_unpack(cp, dst[:size])
    assert st == N.OK and np.array_equal(back, frame)
    if decode:
        assert [c.tolist() for c in ref_decode_rice(want, [c.size for c in planes], bits)] == [c.tolist() for c in planes]
    return size


# ---- what the two codings share --------------------------------------------------------------------------
def _nibbles(coded, offset, groups):
    b = coded[offset:offset + (groups + 1) // 2]
    return np.stack([b & 15, b >> 4], axis=1).reshape(-1)[:groups]


@pytest.mark.parametrize("bits", [(8, 8, 8), (6, 5, 5), (1, 7, 4)])
@pytest.mark.parametrize("W,H,a,b", [(1, 1, 4, 4), (33, 1, 4, 4), (8224, 1, 4, 4), (13, 9, 2, 0), (30, 34, 2, 0)])
def test_the_two_codings_share_groups_sections_and_anchors(W, H, a, b, bits):
    """The Rice coding takes its groups, nibble and anchors sections and blocks from the group coding's geometry: the two layouts agree
    on them, the anchors sections of the two coded frames of one frame are the same bytes, and a group has width 0 exactly when it
    has mode 15."""
    cp = _c_params(W, H, a, b, bits, 1, CSQ)
    pk, rl = lib_layout(cp), rice_layout(cp)
    assert list(rl.groups) == list(pk.groups) and list(rl.modes_offset) == list(pk.widths_offset)
    assert list(rl.anchors_offset) == list(pk.anchors_offset) and rl.directory_offset == pk.fixed_bytes
    assert rl.fixed_bytes == pk.fixed_bytes + 4 * (sum(rl.blocks) + 1)
    frame = np.random.default_rng(W * 1000 + H * 10 + bits[0]).integers(0, 256, _layout(cp).frame_bytes, dtype=np.uint8)
    st, g, gsize = lib_pack(cp, frame)
    st2, r, rsize = rice_pack(cp, frame)
    assert st == N.OK and st2 == N.OK
    a0 = pk.anchors_offset[0]
    assert g[a0:pk.fixed_bytes].tobytes() == r[a0:rl.directory_offset].tobytes()
    for p in range(3):
        w, m = _nibbles(g, pk.widths_offset[p], pk.groups[p]), _nibbles(r, rl.modes_offset[p], rl.groups[p])
        assert np.array_equal(w == 0, m == 15), (p, w.tolist(), m.tolist())


def test_both_codings_refuse_empty_input():
    cp = _c_params(33, 1, 4, 4, (6, 5, 5), 1, CSQ)
    for unpack in (csic.unpack_frame_host, csic.rice_unpack_host):
        with pytest.raises(csic.CsicIOError):
            unpack(cp, b"")
        with pytest.raises(csic.CsicIOError):
            unpack(cp, np.zeros(0, dtype=np.uint8))


# ---- the worked vector ---------------------------------------------------------------------------------
def test_worked_vector():
    codes = np.array([1, 2, 3, 4, 5, 6, 7, 0], dtype=np.int64)
    _, a, u = ref_groups(codes, 3)
    assert u[0].tolist() == [0] + [2] * 7 + [0] * 24 and ref_modes(u, 3).tolist() == [0]
    assert 31 * 0 + int(((u[0, 1:] >> 0) + 1).sum()) == 45
    # one plane alone: the Y plane's sections of an 8 x 1 frame at 3/3/3 (all planes alike at 4:4:4)
    cp = _c_params(8, 1, 4, 4, (3, 3, 3), 1, CSQ)
    planes = [codes] * 3
    frame = _frame_buffer(_layout(cp), [plane_bytes(c, 3) for c in planes], CANARY)
    st, dst, size = rice_pack(cp, frame)
    assert st == N.OK and size == 12 + 12 + 16 + 24
    got = dst[:size].tobytes().hex()
    assert got == "00000000" * 3 + "01000000" * 3 + "00000000" + "02000000" + "04000000" + "06000000" + "2449f2ffff1f0000" * 3
    assert dst[:size].tobytes() == ref_encode_rice(planes, (3, 3, 3))
    check_frame(cp, planes, (3, 3, 3))


# ---- random parameters ---------------------------------------------------------------------------------
def test_random_sets_match_the_reference_byte_for_byte(oracle):
    seen_bits, seen_modes = set(), set()
    for i, (W, H, a, b, bits, f, op, rounding, avg, _, rng) in enumerate(_random_sets(60, 11100)):
        cp = _c_params(W, H, a, b, bits, f, op, rounding, avg)
        argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        if i % 3 == 1:                                        # smooth content: zero groups and small k
            argb = (np.arange(W * H, dtype=np.uint32) // 3 * np.uint32(0x010101)) | np.uint32(0xFF000000)
        elif i % 3 == 2:                                      # a ramp with a few outliers: every k in between
            argb = (np.arange(W * H, dtype=np.uint32) // 2 * np.uint32(0x010101)) | np.uint32(0xFF000000)
            hit = rng.random(W * H) < 0.08
            argb[hit] = rng.integers(0, 1 << 32, int(hit.sum()), dtype=np.uint32)
        planes = codes_of(oracle, W, H, a, b, bits, f, op, rounding, avg, argb)
        lay = _layout(cp)
        assert [c.size for c in planes] == [lay.geometry.y_width * lay.geometry.y_height] + [lay.geometry.chroma_samples] * 2
        check_frame(cp, planes, bits)
        seen_bits |= set(bits)
        for c, q in zip(planes, bits):
            seen_modes |= {(q, int(m)) for m in ref_modes(ref_groups(c, q)[2], q)}
    assert seen_bits == set(range(1, 9))
    assert {m for _, m in seen_modes} == set(range(0, 9)) | {15}


def test_every_mode_of_every_width():
    """Groups built to order: for each q, a frame whose Y groups take mode 15 and then every k that can be the cheapest, in turn: every
    k = 0 .. q but q - 1.  (k = q - 1 costs 31 q + sum (u >> (q - 1)) bits, never less than raw; on a tie every u is below 2^(q - 1), and
    then k = q - 2 costs no more and is the smaller one.  A decoder still has to take it: test_unpack_takes_every_mode_the_format_allows.)"""
    from codec_planes import groups_of_mode                    # (imported here: codec_planes takes its reference from this module)
    for q in range(1, 9):
        rng = np.random.default_rng(11200 + q)
        groups, want = [np.full(32, 1, dtype=np.int64)], [15]
        for k in range(q + 1):
            for c in groups_of_mode(q, k, rng, 1):             # steps of about k bits, until k is the cheapest parameter: 200 draws
                groups.append(c)
                want.append(k)
        assert want == [15] + [k for k in range(q + 1) if k != q - 1], (q, want)
        codes = np.concatenate(groups).astype(np.int64)
        assert ref_modes(ref_groups(codes, q)[2], q).tolist() == want
        cp = _c_params(codes.size, 1, 4, 4, (q, q, q), 1, CSQ)
        check_frame(cp, [codes] * 3, (q, q, q))


def test_constant_and_noise_frames():
    rng = np.random.default_rng(11300)
    W, H = 70, 33
    for bits in ((8, 8, 8), (6, 5, 5), (1, 1, 1)):
        cp = _c_params(W, H, 2, 0, bits, 1, CSQ)
        lay, rl = _layout(cp), rice_layout(cp)
        ns = [lay.geometry.y_width * lay.geometry.y_height] + [lay.geometry.chroma_samples] * 2
        const = [np.full(n, (1 << q) - 1, dtype=np.int64) for n, q in zip(ns, bits)]
        assert check_frame(cp, const, bits) == rl.fixed_bytes          # every group in zero mode: no payload at all
    for bits in ((8, 8, 8), (3, 3, 2)):
        cp = _c_params(W, H, 4, 4, bits, 1, CSQ)
        rl = rice_layout(cp)
        noise = [rng.integers(0, 1 << q, W * H).astype(np.int64) for q in bits]
        size = check_frame(cp, noise, bits)
        assert rl.fixed_bytes < size <= rl.fixed_bytes + 4 * sum(b * (248 * q + 1) for b, q in zip(rl.blocks, bits))
    # more than one block per plane, the last one ragged: 300 groups
    cp = _c_params(32 * 300 - 5, 1, 4, 4, (5, 4, 3), 1, CSQ)
    steps = [np.cumsum(rng.integers(-2, 3, 32 * 300 - 5)) % (1 << q) for q in (5, 4, 3)]
    assert list(rice_layout(cp).blocks) == [2, 2, 2]
    check_frame(cp, steps, (5, 4, 3))


@pytest.mark.parametrize("n", [1, 31, 32, 33])
def test_planes_of_a_group_and_its_neighbours(n):
    rng = np.random.default_rng(11400 + n)
    for bits in ((8, 8, 8), (6, 5, 5), (3, 3, 2), (1, 7, 4)):
        cp = _c_params(n, 1, 4, 4, bits, 1, CSQ)
        check_frame(cp, [rng.integers(0, 1 << q, n).astype(np.int64) for q in bits], bits)
        check_frame(cp, [np.arange(n, dtype=np.int64) // 3 % (1 << q) for q in bits], bits)


def test_unpack_takes_every_mode_the_format_allows():
    """Whether the encoder's k was the cheapest is not checked: frames in which every group takes k = 0, 1, ..., q in turn, from the
    numpy encoder, decode to the same planes (few groups, so that no chunk outgrows 248 q + 1 dwords)."""
    rng = np.random.default_rng(11350)
    for q in (1, 2, 5, 8):
        n = 32 * 9 + 7
        codes = (np.cumsum(rng.integers(-1, 2, n)) % (1 << q)).astype(np.int64)
        codes[64:96] = codes[64]                               # a zero group in between
        cp = _c_params(n, 1, 4, 4, (q, q, q), 1, CSQ)
        frame = _frame_buffer(_layout(cp), [plane_bytes(codes, q)] * 3, CANARY)
        for k in range(q + 1):
            coded = ref_encode_rice([codes] * 3, (q, q, q), force=k)
            assert [c.tolist() for c in ref_decode_rice(coded, [n] * 3, (q, q, q))] == [codes.tolist()] * 3
            st, back = rice_unpack(cp, coded)
            assert st == N.OK and np.array_equal(back, frame), (q, k)


# ---- the reference's image ---------------------------------------------------------------------------------
README_SETS = [(4, 4, (8, 8, 8)), (2, 0, (6, 5, 5)), (2, 0, (4, 4, 4)), (2, 0, (3, 3, 2))]      # factor 1, HOLD


def test_in512_rice_is_smaller_than_groups(oracle, capsys):
    """in512.png at the README's four parameter sets: the library's size equals the numpy reference's and is strictly below the group
    coding's size of the same planes.  The printed sizes are the ones the README and DESIGN.md 4.8 quote."""
    rgb = load_png_rgb(os.path.join(GOLDEN, "inputs", "in512.png"))
    argb = oracle.rgb_to_argb(rgb).reshape(-1)
    lines = []
    for a, b, bits in README_SETS:
        cp = _c_params(512, 512, a, b, bits, 1, CSQ)
        lay = _layout(cp)
        planes = codes_of(oracle, 512, 512, a, b, bits, 1, CSQ, 0, False, argb)
        frame = _frame_buffer(lay, [plane_bytes(c, q) for c, q in zip(planes, bits)], CANARY)
        want = ref_encode_rice(planes, bits)
        st, dst, size = rice_pack(cp, frame)
        assert st == N.OK and size == len(want) and dst[:size].tobytes() == want
        st, _, groups_size = lib_pack(cp, frame)
        assert st == N.OK
        lines.append(f"4:{a}:{b} {bits[0]}/{bits[1]}/{bits[2]}: raw {lay.payload_bytes} groups {groups_size} rice {size} "
                     f"({groups_size / lay.payload_bytes:.3f} / {size / lay.payload_bytes:.3f} of raw)")
        assert size < groups_size < lay.payload_bytes, lines[-1]
        st, back = rice_unpack(cp, dst[:size])
        assert st == N.OK and np.array_equal(back, frame)
    with capsys.disabled():
        print("\n" + "\n".join(lines))


# ---- refusals ------------------------------------------------------------------------------------------------
BITS = (5, 4, 3)


@pytest.fixture(scope="module")
def coded_frame():
    """A valid coded frame with zero, Rice and raw groups in every plane, 10 groups each (the nibbles and the anchors both end in
    padding): (c_params, frame buffer, coded bytes, rice layout, per-block info of the numpy encoder)."""
    rng = np.random.default_rng(11500)
    n = 315
    cp = _c_params(n, 1, 4, 4, BITS, 1, CSQ)
    planes = []
    for q in BITS:
        c = np.cumsum(rng.integers(-1, 2, n)) % (1 << q)
        c[:32] = 3                                             # group 0: zero mode
        c[32:64] = rng.integers(0, 1 << q, 32)                 # group 1: noise
        planes.append(c.astype(np.int64))
    frame = _frame_buffer(_layout(cp), [plane_bytes(c, q) for c, q in zip(planes, BITS)], CANARY)
    info = []
    want = ref_encode_rice(planes, BITS, info)
    st, dst, size = rice_pack(cp, frame)
    assert st == N.OK and dst[:size].tobytes() == want
    return cp, frame, dst[:size].copy(), rice_layout(cp), info


def _refused(cp, coded):
    st, out = rice_unpack(cp, coded)
    assert st == N.EFORMAT, st
    assert N.lib().csic_last_error().decode() != ""
    assert np.all(out == CANARY)                               # a refused frame writes nothing
    with pytest.raises(csic.CsicIOError):
        csic.rice_unpack_host(cp, coded)


def _dir(coded, rl, i, value=None):
    at = rl.directory_offset + 4 * i
    if value is not None:
        coded[at:at + 4] = np.frombuffer(np.uint32(value).tobytes(), dtype=np.uint8)
    return int(np.frombuffer(coded[at:at + 4].tobytes(), dtype="<u4")[0])


def _flip(coded, rl, dword, bit):
    """Flips bit `bit` of the payload, counted from payload dword `dword`."""
    coded[rl.payload_offset + 4 * dword + bit // 8] ^= 1 << (bit % 8)


def test_unpack_refuses_damaged_input(coded_frame):
    cp, frame, coded, rl, info = coded_frame
    assert rice_unpack(cp, coded)[0] == N.OK
    for p, q in enumerate(BITS):
        bad = coded.copy()                                     # a nibble outside {0 .. q, 15}
        bad[rl.modes_offset[p]] = (bad[rl.modes_offset[p]] & 0xF0) | (q + 1)
        _refused(cp, bad)
        bad = coded.copy()
        bad[rl.modes_offset[p]] = (bad[rl.modes_offset[p]] & 0xF0) | 14
        _refused(cp, bad)
        bad = coded.copy()                                     # a padding nibble (10 groups: nibbles 10 .. 15 are padding)
        bad[rl.modes_offset[p] + 7] |= 0x10
        _refused(cp, bad)
        bad = coded.copy()                                     # the last bit of the anchors section (10 q bits: 50 / 64, 40 / 64, 30 / 32)
        bad[rl.anchors_offset[p] + 4 * ((10 * q + 31) // 32) - 1] |= 0x80
        _refused(cp, bad)
        _, d0, rbits, ubits, z = info[p]
        assert rbits % 32 and ubits % 32 and z > 0
        bad = coded.copy()                                     # the first padding bit of R
        _flip(bad, rl, d0, rbits)
        _refused(cp, bad)
        bad = coded.copy()                                     # the first padding bit of U: one terminator too many
        _flip(bad, rl, d0 + (rbits + 31) // 32, ubits)
        _refused(cp, bad)
        bad = coded.copy()                                     # the last terminator of U gone: one too few
        _flip(bad, rl, d0 + (rbits + 31) // 32, ubits - 1)
        _refused(cp, bad)
    nb = 3
    assert [_dir(coded, rl, i) for i in range(nb + 1)] == [i[1] for i in info] + [(coded.size - rl.fixed_bytes) // 4]
    bad = coded.copy()                                         # dir[0] != 0
    _dir(bad, rl, 0, 1)
    _refused(cp, bad)
    for delta in (+1, -1):                                     # a chunk that is one dword longer / shorter than its modes and U imply
        bad = coded.copy()
        _dir(bad, rl, 1, _dir(coded, rl, 1) + delta)
        _refused(cp, bad)
    bad = coded.copy()                                         # not monotonic
    _dir(bad, rl, 1, _dir(coded, rl, 2) + 1)
    _refused(cp, bad)
    # a zero dword slipped in behind the first chunk, every later entry and the size adjusted: U is not ceil(U bits / 32) dwords
    at = rl.payload_offset + 4 * info[1][1]
    bad = np.concatenate([coded[:at], np.zeros(4, dtype=np.uint8), coded[at:]])
    for i in (1, 2, 3):
        _dir(bad, rl, i, _dir(coded, rl, i) + 1)
    _refused(cp, bad)
    # coded_bytes != fixed_bytes + 4 dir[NB]
    _refused(cp, np.concatenate([coded, np.zeros(4, dtype=np.uint8)]))
    _refused(cp, coded[:-4])
    _refused(cp, coded[:-1])
    _refused(cp, coded[:rl.fixed_bytes - 4])
    _refused(cp, coded[:0])
    bad = coded.copy()
    _dir(bad, rl, nb, _dir(coded, rl, nb) + 1)
    _refused(cp, bad)
    # a terminator moved inside U: the count stays right, a later group starts elsewhere -- refused or decoded to SOME valid frame
    bad = coded.copy()
    _, d0, rbits, ubits, z = info[0]
    ub = np.unpackbits(coded[rl.payload_offset + 4 * (d0 + (rbits + 31) // 32):], bitorder="little")[:ubits]
    one = int(np.flatnonzero(ub)[5])
    zero = int(np.flatnonzero(ub == 0)[-1])
    _flip(bad, rl, d0 + (rbits + 31) // 32, one)
    _flip(bad, rl, d0 + (rbits + 31) // 32, zero)
    st, out = rice_unpack(cp, bad)
    assert st in (N.OK, N.EFORMAT)
    if st == N.OK:
        assert rice_pack(cp, out)[0] == N.OK
    else:
        assert np.all(out == CANARY)


def test_unpack_refuses_a_residual_of_more_than_q_bits():
    """q = 2, u_1 = u_2 = 2 and the rest 0: k = 0, U = 001 001 1...; with the first terminator moved to the front U still holds 31,
    and slot 2 reads four zero bits: u_2 = 4 >= 2^q."""
    codes = np.array([0, 1] + [2] * 30, dtype=np.int64)
    cp = _c_params(32, 1, 4, 4, (2, 2, 2), 1, CSQ)
    frame = _frame_buffer(_layout(cp), [plane_bytes(codes, 2)] * 3, CANARY)
    st, dst, size = rice_pack(cp, frame)
    rl = rice_layout(cp)
    assert st == N.OK and dst[:size].tobytes() == ref_encode_rice([codes] * 3, (2, 2, 2))
    assert dst[rl.modes_offset[0]] == 0 and dst[rl.payload_offset] == 0b11100100
    coded = dst[:size].copy()
    assert rice_unpack(cp, coded)[0] == N.OK
    coded[rl.payload_offset] = 0b11100001
    _refused(cp, coded)


def test_argument_refusals(coded_frame):
    cp, frame, coded, rl, _ = coded_frame
    L = N.lib()
    size = coded.size
    n = C.c_uint64()
    pf, pc = frame.ctypes.data_as(C.c_void_p), coded.ctypes.data_as(C.c_void_p)
    assert L.csic_rice_pack_host(None, pf, pc, size, C.byref(n)) == N.EINVAL_NULL
    assert L.csic_rice_pack_host(C.byref(cp), None, pc, size, C.byref(n)) == N.EINVAL_NULL
    assert L.csic_rice_pack_host(C.byref(cp), pf, None, size, C.byref(n)) == N.EINVAL_NULL
    assert L.csic_rice_pack_host(C.byref(cp), pf, pc, size, None) == N.EINVAL_NULL
    assert L.csic_rice_unpack_host(None, pc, size, pf) == N.EINVAL_NULL
    assert L.csic_rice_unpack_host(C.byref(cp), None, size, pf) == N.EINVAL_NULL
    assert L.csic_rice_unpack_host(C.byref(cp), pc, size, None) == N.EINVAL_NULL
    assert L.csic_rice_layout_of(None, C.byref(N.CsicRiceLayout())) == N.EINVAL_NULL
    assert L.csic_rice_layout_of(C.byref(cp), None) == N.EINVAL_NULL
    bad = _c_params(45, 7, 3, 3, BITS, 1, CSQ)
    assert L.csic_rice_layout_of(C.byref(bad), C.byref(N.CsicRiceLayout())) == N.EINVAL_CHROMA_A
    assert L.csic_rice_pack_host(C.byref(bad), pf, pc, size, C.byref(n)) == N.EINVAL_CHROMA_A
    assert L.csic_rice_unpack_host(C.byref(bad), pc, size, pf) == N.EINVAL_CHROMA_A
    bad = _c_params(45, 7, 4, 4, (5, 9, 3), 1, CSQ)
    assert L.csic_rice_pack_host(C.byref(bad), pf, pc, size, C.byref(n)) == N.EINVAL_BITS
    ycc = csic.make_c_params(45, 7, 4, 4, 5, 4, 3, 1, CSQ, in_format=N.FMT_YCBCR888X, out_format=N.FMT_ARGB8888)
    assert L.csic_rice_pack_host(C.byref(ycc), pf, pc, size, C.byref(n)) == N.EINVAL_FORMAT
