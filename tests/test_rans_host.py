"""The rANS coding on the host (csic_rans_layout_of, csic_rans_pack_host, csic_rans_unpack_host; include/csic.h) without a GPU, against a
numpy encoder and decoder written here from the format's text alone -- its own scaling rule, interleave and raw decision.  They share
nothing with the library but the groups, anchors and folded residuals of tests/test_pack_host.py (ref_groups), which the format
carries over from the group coding.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_png_rgb
from test_container import CANARY, CSQ, _c_params, _frame_buffer, _layout, _random_sets, pack_codes
from test_pack_host import codes_of, lib_pack, plane_bytes, ref_groups
from test_rice_host import README_SETS, rice_pack

import csic_amd as csic

N = csic._native
M, L, BLOCK, LANES, STEPS = 4096, 1 << 16, 1024, 64, 496
RAW_FLAG = 1 << 31


# ---- the definition, in numpy ---------------------------------------------------------------------
def ref_scale(counts):
    """The scaling rule: counts c_s (their sum N > 0) -> frequencies f_s with sum M."""
    c = np.asarray(counts, dtype=np.int64)
    f = np.where(c > 0, np.maximum(1, c * M // c.sum()), 0)
    d = M - int(f.sum())
    if d > 0:
        f[np.argmax(c)] += d                                   # the largest count, the smallest s on a tie (argmax: the first)
    for _ in range(-d):
        f[np.argmax(f)] -= 1                                   # the currently largest f, the smallest s on a tie
    assert f.sum() == M and np.all((f >= 1) == (c > 0))
    return f


def _pack_bits(bits):
    """A bit string -> its dwords as bytes, LSB first, zero-padded to a dword."""
    bits = np.concatenate([bits, np.zeros(-bits.size % 32, dtype=np.uint8)])
    return np.packbits(bits, bitorder="little").tobytes()


def raw_dwords(ng, q):
    return (ng * 31 * q + 31) // 32


def ref_raw_chunk(u, q):
    """The groups of one block -> the raw chunk: 31 q bits per group, u_j at bits [(j - 1) q, j q) of the group's run."""
    return _pack_bits(((u[:, 1:, None] >> np.arange(q)) & 1).astype(np.uint8).reshape(-1))


def ref_rans_plane(u, q, trace=None):
    """(G, 32) folded residuals of a plane -> (f, [(raw, chunk bytes, words)] per block).  The encoder runs the decode order backwards,
    every block's 64 streams side by side; rec[b, t, l] keeps the word stream l of block b emits at step t, so that reading rec in
    (t, l) order gives the word string in decode order.  `trace` (a list) receives, per block, the (t, l) of every word."""
    G = u.shape[0]
    f = ref_scale(np.bincount(u[:, 1:].reshape(-1), minlength=1 << q))
    cum = np.cumsum(f) - f
    B = (G + BLOCK - 1) // BLOCK
    sym = np.zeros((B * BLOCK, 32), dtype=np.int64)
    sym[:G] = u
    sym = sym.reshape(B, 16, LANES, 32)                        # group 1024 b + 64 i + l
    exists = (np.arange(B * BLOCK) < G).reshape(B, 16, LANES)
    x = np.full((B, LANES), L, dtype=np.int64)
    rec = np.full((B, STEPS, LANES), -1, dtype=np.int64)
    for t in range(STEPS - 1, -1, -1):
        i, j = t // 31, 1 + t % 31
        s, act = sym[:, i, :, j], exists[:, i]
        fs = np.where(act, f[s], 1)
        emit = act & (x >= (fs << 20))
        rec[:, t][emit] = x[emit] & 0xFFFF
        x = np.where(emit, x >> 16, x)
        x = np.where(act, ((x // fs) << 12) + x % fs + cum[s], x)
        assert np.all((x >= L) & (x < (1 << 32)))
    blocks = []
    for b in range(B):
        ub = u[BLOCK * b:BLOCK * (b + 1)]
        ng = ub.shape[0]
        flat = rec[b].reshape(-1)
        words = flat[flat >= 0]
        if trace is not None:
            trace.append([(int(k) // LANES, int(k) % LANES) for k in np.flatnonzero(flat >= 0)])
        rans = x[b, :min(ng, LANES)].astype("<u4").tobytes() + words.astype("<u2").tobytes()
        rans += bytes(-len(rans) % 4)
        raw = raw_dwords(ng, q) < len(rans) // 4                # raw iff strictly smaller
        blocks.append((raw, ref_raw_chunk(ub, q) if raw else rans, int(words.size)))
    return f, blocks


def ref_rans_layout(ns, bits):
    G = [(n + 31) // 32 for n in ns]
    B = [(g + BLOCK - 1) // BLOCK for g in G]
    tsz = [2 << q for q in bits]
    asz = [4 * ((g * q + 31) // 32) for g, q in zip(G, bits)]
    toff = [0, tsz[0], tsz[0] + tsz[1]]
    aoff = [sum(tsz), sum(tsz) + asz[0], sum(tsz) + asz[0] + asz[1]]
    doff = sum(tsz) + sum(asz)
    fixed = doff + 4 * (sum(B) + 1)
    top = fixed + 4 * sum(raw_dwords(min(BLOCK, g - BLOCK * b), q) for g, nb, q in zip(G, B, bits) for b in range(nb))
    return dict(G=G, B=B, toff=toff, aoff=aoff, doff=doff, fixed=fixed, top=top, bound=(top + 255) // 256 * 256)


def ref_encode_rans(planes, bits, info=None):
    """Three planes of codes -> the coded frame's bytes.  `info` (a list) receives per block (plane, dir offset, raw, dwords, words)."""
    parts = [ref_groups(c, q) for c, q in zip(planes, bits)]
    coded = [ref_rans_plane(u, q) for (_, _, u), q in zip(parts, bits)]
    out = b"".join(f.astype("<u2").tobytes() for f, _ in coded)                # 1. tables
    for (_, anchors, _), q in zip(parts, bits):                # 2. anchors, as in the group coding
        a = pack_codes(anchors.astype(np.uint8) << (8 - q), q).tobytes()
        out += a + bytes(-len(a) % 4)
    directory, payload = [], b""
    for p, (_, blocks) in enumerate(coded):
        for raw, chunk, words in blocks:                       # 4. one chunk per block
            directory.append(len(payload) // 4 | (RAW_FLAG if raw else 0))
            if info is not None:
                info.append((p, len(payload) // 4, raw, len(chunk) // 4, words))
            payload += chunk
    directory.append(len(payload) // 4)                        # 3. directory: NB + 1 uint32
    return out + np.array(directory, dtype="<u4").tobytes() + payload


def ref_decode_rans(coded, ns, bits):
    """Coded bytes -> three planes of codes, by the decode rule: nothing but the tables, the anchors, the directory and the chunks."""
    lay = ref_rans_layout(ns, bits)
    rawb = np.frombuffer(coded, dtype=np.uint8)
    allbits = np.unpackbits(rawb, bitorder="little")
    nb = sum(lay["B"])
    directory = np.frombuffer(coded[lay["doff"]:lay["doff"] + 4 * (nb + 1)], dtype="<u4").astype(np.int64)
    assert directory[0] & ~RAW_FLAG == 0 and directory[nb] & RAW_FLAG == 0 and lay["fixed"] + 4 * directory[nb] == len(coded)
    planes, blk = [], 0
    for p, (n, q) in enumerate(zip(ns, bits)):
        G = lay["G"][p]
        f = np.frombuffer(coded[lay["toff"][p]:lay["toff"][p] + (2 << q)], dtype="<u2").astype(np.int64)
        assert f.sum() == M
        cum = np.cumsum(f) - f
        slot2sym = np.repeat(np.arange(1 << q), f)
        ab = allbits[8 * lay["aoff"][p]:8 * lay["aoff"][p] + G * q].reshape(G, q).astype(np.int64)
        u = np.zeros((G, 32), dtype=np.int64)
        for b in range(lay["B"][p]):
            d0, d1 = int(directory[blk] & ~RAW_FLAG), int(directory[blk + 1] & ~RAW_FLAG)
            ng = min(BLOCK, G - BLOCK * b)
            ns_ = min(ng, LANES)
            at = lay["fixed"] + 4 * d0
            if directory[blk] & RAW_FLAG:
                assert d1 - d0 == raw_dwords(ng, q)
                cb = allbits[8 * at:8 * at + ng * 31 * q].reshape(ng, 31, q).astype(np.int64)
                u[BLOCK * b:BLOCK * b + ng, 1:] = (cb << np.arange(q)).sum(axis=2)
            else:
                assert ns_ <= d1 - d0 <= raw_dwords(ng, q)
                x = np.frombuffer(coded[at:at + 4 * ns_], dtype="<u4").astype(np.int64)
                words = np.frombuffer(coded[at + 4 * ns_:lay["fixed"] + 4 * d1], dtype="<u2").astype(np.int64)
                assert np.all(x >= L)
                nxt = 0
                for t in range(STEPS):
                    i, j = t // 31, 1 + t % 31
                    k = min(ns_, ng - LANES * i)               # the streams whose group i exists: 0 .. k - 1
                    if k <= 0:
                        break
                    slot = x[:k] & (M - 1)
                    s = slot2sym[slot]
                    u[BLOCK * b + LANES * i:BLOCK * b + LANES * i + k, j] = s
                    x[:k] = f[s] * (x[:k] >> 12) + slot - cum[s]
                    need = np.flatnonzero(x[:k] < L)           # ascending stream order
                    x[need] = (x[need] << 16) | words[nxt:nxt + need.size]
                    nxt += need.size
                assert np.all(x == L)
                assert nxt == words.size or (nxt + 1 == words.size and words[-1] == 0)
            blk += 1
        e = np.where(u % 2 == 0, u // 2, -(u + 1) // 2)
        e[:, 0] = (ab << np.arange(q)).sum(axis=1)
        planes.append((np.cumsum(e, axis=1) % (1 << q)).reshape(-1)[:n])
    return planes


# ---- calling the library ----------------------------------------------------------------------------
def rans_layout(cp):
    lay = N.CsicRansLayout()
    N.check(N.lib().csic_rans_layout_of(C.byref(cp), C.byref(lay)))
    return lay


def rans_pack(cp, frame, capacity=None, fill=CANARY):
    """-> (status, the whole destination buffer, coded_bytes)"""
    cap = rans_layout(cp).bound_bytes if capacity is None else capacity
    dst = np.full(max(cap, 1), fill, dtype=np.uint8)
    n = C.c_uint64(0)
    st = N.lib().csic_rans_pack_host(C.byref(cp), frame.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    return st, dst, n.value


def rans_unpack(cp, coded, fill=CANARY):
    """-> (status, the whole frame buffer, pre-filled with `fill`)"""
    coded = np.frombuffer(bytes(coded), dtype=np.uint8) if not isinstance(coded, np.ndarray) else coded
    src = np.ascontiguousarray(coded) if coded.size else np.zeros(1, dtype=np.uint8)
    out = np.full(_layout(cp).frame_bytes, fill, dtype=np.uint8)
    st = N.lib().csic_rans_unpack_host(C.byref(cp), src.ctypes.data_as(C.c_void_p), coded.size, out.ctypes.data_as(C.c_void_p))
    return st, out


def check_frame(cp, planes, bits, info=None):
    """One frame through csic_rans_pack_host and csic_rans_unpack_host against the numpy statement, canaries included."""
    lay, rl = _layout(cp), rans_layout(cp)
    ref = ref_rans_layout([c.size for c in planes], bits)
    assert list(rl.groups) == ref["G"] and list(rl.blocks) == ref["B"] and list(rl.tables_offset) == ref["toff"]
    assert list(rl.anchors_offset) == ref["aoff"] and rl.directory_offset == ref["doff"]
    assert rl.payload_offset == rl.fixed_bytes == ref["fixed"] and rl.bound_bytes == ref["bound"] and rl.bound_bytes % 256 == 0
    assert bytes(csic.rans_layout(cp)) == bytes(rl)
    pbytes = [plane_bytes(c, q) for c, q in zip(planes, bits)]
    want = ref_encode_rans(planes, bits, info)
    frame = _frame_buffer(lay, pbytes, CANARY)
    st, dst, size = rans_pack(cp, frame)
    assert st == N.OK and size == len(want) and dst[:size].tobytes() == want
    assert rl.fixed_bytes <= size <= ref["top"] <= rl.bound_bytes and np.all(dst[size:] == CANARY)
    assert csic.rans_pack_host(cp, frame).tobytes() == want
    # neither the padding of the source nor the unused high bits of a plane's last byte are read into a value
    other = _frame_buffer(lay, pbytes, 0x11)
    for off, nb, c, q in zip((lay.y_offset, lay.cb_offset, lay.cr_offset), (lay.y_bytes, lay.cb_bytes, lay.cr_bytes), planes, bits):
        if (c.size * q) % 8:
            other[off + nb - 1] |= (0xFF << ((c.size * q) % 8)) & 0xFF
    st, dst2, size2 = rans_pack(cp, other)
    assert st == N.OK and size2 == size and dst2[:size].tobytes() == want
    # the capacity rule: exactly the size suffices, less fails with the size that was needed and writes nothing behind the capacity
    st, dst3, size3 = rans_pack(cp, frame, capacity=size)
    assert st == N.OK and size3 == size and dst3[:size].tobytes() == want
    for cap in {rl.fixed_bytes, size - 4}:
        if rl.fixed_bytes <= cap < size:
            st, dst4, need = rans_pack(cp, frame, capacity=cap)
            assert st == N.EINVAL_SIZE and need == size and np.all(dst4[cap:] == CANARY)
    assert rans_pack(cp, frame, capacity=rl.fixed_bytes - 1)[0] == N.EINVAL_SIZE
    # decode: the payload ranges come back, the canary around them stays; the numpy decoder reads the same bytes
    st, back = rans_unpack(cp, dst[:size])
    assert st == N.OK and np.array_equal(back, frame)
    assert np.array_equal(csic.rans_unpack_host(cp, want), _frame_buffer(lay, pbytes, 0))
    assert [c.tolist() for c in ref_decode_rans(want, [c.size for c in planes], bits)] == [np.asarray(c).tolist() for c in planes]
    return size


# ---- the scaling rule ------------------------------------------------------------------------------------
def test_scaling_rule_paths():
    assert ref_scale([24, 0, 7, 0, 0, 0, 0, 0]).tolist() == [3172, 0, 924, 0, 0, 0, 0, 0]       # the worked vector: + 1 to the largest count
    assert ref_scale([5, 0]).tolist() == [M, 0]
    assert ref_scale([3, 3]).tolist() == [2048, 2048]
    assert ref_scale([1, 1, 1, 0]).tolist() == [1366, 1365, 1365, 0]                             # a tie: the smallest s takes the remainder
    f = ref_scale([100000] + [1] * 255)                        # 255 floors of 0 are lifted to 1: the excess comes off the largest f
    assert f[1:].tolist() == [1] * 255 and f[0] == M - 255


# ---- the worked vector ---------------------------------------------------------------------------------
def test_worked_vector():
    codes = np.array([1, 2, 3, 4, 5, 6, 7, 0], dtype=np.int64)
    _, a, u = ref_groups(codes, 3)
    assert u[0].tolist() == [0] + [2] * 7 + [0] * 24
    trace = []
    f, blocks = ref_rans_plane(u, 3, trace)
    assert f.tolist() == [3172, 0, 924, 0, 0, 0, 0, 0] and raw_dwords(1, 3) == 3
    assert [(raw, chunk.hex(), words) for raw, chunk, words in blocks] == [(False, WORKED_CHUNK, 1)] and len(trace[0]) == 1
    # one plane alone: the Y plane's sections of an 8 x 1 frame at 3/3/3 (all planes alike at 4:4:4)
    cp = _c_params(8, 1, 4, 4, (3, 3, 3), 1, CSQ)
    planes = [codes] * 3
    frame = _frame_buffer(_layout(cp), [plane_bytes(c, 3) for c in planes], CANARY)
    st, dst, size = rans_pack(cp, frame)
    assert st == N.OK and size == 48 + 12 + 16 + 24
    got = dst[:size].tobytes().hex()
    assert got == "640c00009c030000" "0000000000000000" * 3 + "01000000" * 3 + "00000000" + "02000000" + "04000000" + "06000000" + WORKED_CHUNK * 3
    assert dst[:size].tobytes() == ref_encode_rans(planes, (3, 3, 3))
    check_frame(cp, planes, (3, 3, 3))


WORKED_CHUNK = "c88ce900d49d0000"


# ---- random parameters ---------------------------------------------------------------------------------
def test_random_sets_match_the_reference_byte_for_byte(oracle):
    seen_bits, kinds = set(), set()
    for i, (W, H, a, b, bits, f, op, rounding, avg, _, rng) in enumerate(_random_sets(40, 21100)):
        cp = _c_params(W, H, a, b, bits, f, op, rounding, avg)
        argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        if i % 3 == 1:                                        # smooth content: skewed tables
            argb = (np.arange(W * H, dtype=np.uint32) // 3 * np.uint32(0x010101)) | np.uint32(0xFF000000)
        elif i % 3 == 2:                                      # a ramp with a few outliers
            argb = (np.arange(W * H, dtype=np.uint32) // 2 * np.uint32(0x010101)) | np.uint32(0xFF000000)
            hit = rng.random(W * H) < 0.08
            argb[hit] = rng.integers(0, 1 << 32, int(hit.sum()), dtype=np.uint32)
        planes = codes_of(oracle, W, H, a, b, bits, f, op, rounding, avg, argb)
        info = []
        check_frame(cp, planes, bits, info)
        seen_bits |= set(bits)
        kinds |= {raw for _, _, raw, _, _ in info}
    assert seen_bits == set(range(1, 9)) and kinds == {False, True}


def test_constant_noise_and_several_blocks():
    rng = np.random.default_rng(21300)
    W, H = 70, 33
    for bits in ((8, 8, 8), (6, 5, 5), (1, 1, 1)):
        cp = _c_params(W, H, 2, 0, bits, 1, CSQ)
        lay, rl = _layout(cp), rans_layout(cp)
        ns = [lay.geometry.y_width * lay.geometry.y_height] + [lay.geometry.chroma_samples] * 2
        const = [np.full(n, (1 << q) - 1, dtype=np.int64) for n, q in zip(ns, bits)]
        info = []
        size = check_frame(cp, const, bits, info)             # f_0 = M codes in zero bits: a chunk is its states
        assert all(not raw and words == 0 for _, _, raw, _, words in info)
        assert size == rl.fixed_bytes + 4 * sum(min(g, LANES) for g in rl.groups)
    for bits in ((8, 8, 8), (3, 3, 2)):                        # noise: every block is capped by its raw chunk
        cp = _c_params(W, H, 4, 4, bits, 1, CSQ)
        noise = [rng.integers(0, 1 << q, W * H).astype(np.int64) for q in bits]
        info = []
        size = check_frame(cp, noise, bits, info)
        assert all(raw for _, _, raw, _, _ in info) and size == ref_rans_layout([W * H] * 3, bits)["top"]
    # more than one block per plane, the last one ragged: 1030 groups
    n = 32 * 1030 - 5
    cp = _c_params(n, 1, 4, 4, (5, 4, 3), 1, CSQ)
    steps = [np.cumsum(rng.integers(-2, 3, n)) % (1 << q) for q in (5, 4, 3)]
    assert list(rans_layout(cp).blocks) == [2, 2, 2]
    check_frame(cp, steps, (5, 4, 3))


@pytest.mark.parametrize("n", [1, 31, 32, 33, 32 * 63 + 1, 32 * 64, 32 * 65 - 3])
def test_planes_of_a_group_and_its_neighbours(n):
    rng = np.random.default_rng(21400 + n)
    for bits in ((8, 8, 8), (6, 5, 5), (3, 3, 2), (1, 7, 4)):
        cp = _c_params(n, 1, 4, 4, bits, 1, CSQ)
        check_frame(cp, [rng.integers(0, 1 << q, n).astype(np.int64) for q in bits], bits)
        check_frame(cp, [np.arange(n, dtype=np.int64) // 3 % (1 << q) for q in bits], bits)


# ---- the reference's image ---------------------------------------------------------------------------------
def test_in512_rans_is_smaller_than_rice(oracle, capsys):
    """in512.png at the README's four parameter sets: the library's size equals the numpy statement's, lies below the Rice coding's
    stored bytes for all four and below 0.93 of them at 8/8/8 and 3/3/2.  The printed sizes are the ones the README and DESIGN.md 4.13
    quote."""
    rgb = load_png_rgb(os.path.join(GOLDEN, "inputs", "in512.png"))
    argb = oracle.rgb_to_argb(rgb).reshape(-1)
    lines = []
    for a, b, bits in README_SETS:
        cp = _c_params(512, 512, a, b, bits, 1, CSQ)
        lay = _layout(cp)
        planes = codes_of(oracle, 512, 512, a, b, bits, 1, CSQ, 0, False, argb)
        frame = _frame_buffer(lay, [plane_bytes(c, q) for c, q in zip(planes, bits)], CANARY)
        info = []
        want = ref_encode_rans(planes, bits, info)
        st, dst, size = rans_pack(cp, frame)
        assert st == N.OK and size == len(want) and dst[:size].tobytes() == want
        st, _, rice_size = rice_pack(cp, frame)
        assert st == N.OK
        lines.append(f"4:{a}:{b} {bits[0]}/{bits[1]}/{bits[2]}: raw {lay.payload_bytes} rice {rice_size} rans {size} "
                     f"({size / rice_size:.3f} of rice, {sum(raw for _, _, raw, _, _ in info)} of {len(info)} blocks raw)")
        with capsys.disabled():
            print("\n" + lines[-1], end="")
        assert size < rice_size, lines[-1]
        if bits in ((8, 8, 8), (3, 3, 2)):
            assert size < 0.93 * rice_size, lines[-1]
        st, back = rans_unpack(cp, dst[:size])
        assert st == N.OK and np.array_equal(back, frame)
    with capsys.disabled():
        print()


# ---- refusals ------------------------------------------------------------------------------------------------
BITS = (5, 4, 3)


@pytest.fixture(scope="module")
def coded_frame():
    """A valid coded frame of two blocks per plane (1024 and 6 groups; the anchors end in padding): Y and Cr smooth -- rANS chunks --, Cb
    smooth with noise in its second block, which is raw.  -> (c_params, frame buffer, coded bytes, rans layout, the numpy encoder's
    per-block info)."""
    rng = np.random.default_rng(21500)
    n = 32 * 1030 - 5
    cp = _c_params(n, 1, 4, 4, BITS, 1, CSQ)
    planes = [(np.cumsum(rng.integers(-1, 2, n)) % (1 << q)).astype(np.int64) for q in BITS]
    planes[1][32 * 1024:] = rng.integers(0, 1 << BITS[1], n - 32 * 1024)
    frame = _frame_buffer(_layout(cp), [plane_bytes(c, q) for c, q in zip(planes, BITS)], CANARY)
    info = []
    want = ref_encode_rans(planes, BITS, info)
    assert [raw for _, _, raw, _, _ in info] == [False, False, False, True, False, False]
    st, dst, size = rans_pack(cp, frame)
    assert st == N.OK and dst[:size].tobytes() == want
    return cp, frame, dst[:size].copy(), rans_layout(cp), info


def _refused(cp, coded):
    st, out = rans_unpack(cp, coded)
    assert st == N.EFORMAT and np.all(out == CANARY), N.lib().csic_last_error()
    with pytest.raises(csic.CsicIOError):
        csic.rans_unpack_host(cp, coded)


def _dir(coded, rl, i, value=None):
    at = rl.directory_offset + 4 * i
    if value is None:
        return int.from_bytes(coded[at:at + 4].tobytes(), "little")
    coded[at:at + 4] = np.frombuffer(int(value).to_bytes(4, "little"), dtype=np.uint8)


def _dword(coded, at, value=None):
    if value is None:
        return int.from_bytes(coded[at:at + 4].tobytes(), "little")
    coded[at:at + 4] = np.frombuffer(int(value).to_bytes(4, "little"), dtype=np.uint8)


def test_unpack_refuses_damaged_input(coded_frame):
    cp, frame, good, rl, info = coded_frame
    st, back = rans_unpack(cp, good)
    assert st == N.OK and np.array_equal(back, frame)
    nb = len(info)
    pay = rl.payload_offset
    groups = [1024, 6] * 3

    def damaged(change):
        c = good.copy()
        c = change(c)
        _refused(cp, good if c is None else c)

    def edit(fn):                                              # a change in place
        def change(c):
            fn(c)
            return c
        return change

    # a table that does not sum to M: one frequency more, then one moved to a symbol that never occurs (the sum stays: decodes wrongly)
    for p in range(3):
        t = rl.tables_offset[p]
        c = good.copy()
        c[t:t + 2] = np.frombuffer(int(int.from_bytes(c[t:t + 2].tobytes(), "little") + 1).to_bytes(2, "little"), dtype=np.uint8)
        _refused(cp, c)
    # a set padding bit: behind the last anchor, behind a raw chunk's last bit, in the padding word of a word string
    for p, q in enumerate(BITS):
        assert (1030 * q) % 32
        c = good.copy()
        c[rl.anchors_offset[p] + 4 * ((1030 * q + 31) // 32) - 1] |= 0x80
        _refused(cp, c)
    (p, off, raw, dwords, words), = [b for b in info if b[2]]
    assert (6 * 31 * BITS[p]) % 32
    c = good.copy()
    c[pay + 4 * (off + dwords) - 1] |= 0x80
    _refused(cp, c)
    wcp = _c_params(8, 1, 4, 4, (3, 3, 3), 1, CSQ)             # the worked vector: one word per chunk, so each ends in a padding word
    wcodes = np.array([1, 2, 3, 4, 5, 6, 7, 0], dtype=np.int64)
    wgood = np.frombuffer(ref_encode_rans([wcodes] * 3, (3, 3, 3)), dtype=np.uint8)
    assert rans_unpack(wcp, wgood)[0] == N.OK
    for k in range(3):
        c = wgood.copy()
        c[rans_layout(wcp).payload_offset + 8 * k + 6] |= 0x01
        _refused(wcp, c)
    # the directory: dir[0] with an offset, offsets that decrease, a flag on dir[NB], a coded_bytes that is not the directory's
    damaged(edit(lambda c: _dir(c, rl, 0, 1)))
    damaged(edit(lambda c: (_dir(c, rl, 1, _dir(good, rl, 2)), _dir(c, rl, 2, _dir(good, rl, 1)))))
    damaged(edit(lambda c: _dir(c, rl, nb, _dir(good, rl, nb) | RAW_FLAG)))
    damaged(lambda c: c[:-4])
    damaged(lambda c: np.concatenate([c, np.zeros(4, dtype=np.uint8)]))
    damaged(edit(lambda c: _dir(c, rl, nb, _dir(good, rl, nb) + 1)))
    damaged(lambda c: c[:rl.fixed_bytes - 4])
    damaged(lambda c: c[:-1])
    # a raw chunk that is not exactly its size: the flag on a rANS chunk; the raw chunk read as a rANS chunk
    for i, (p, off, raw, dwords, words) in enumerate(info):
        assert raw or dwords != raw_dwords(groups[i], BITS[p])
        damaged(edit(lambda c: _dir(c, rl, i, _dir(good, rl, i) ^ RAW_FLAG)))
    # a rANS chunk shorter than its states: block 0 ends one dword early
    damaged(edit(lambda c: _dir(c, rl, 1, LANES - 1)))
    # a rANS chunk longer than its block's raw chunk, and one with words nobody takes: zero dwords behind the last block
    p, off, raw, dwords, words = info[-1]
    room = raw_dwords(6, BITS[2]) - dwords
    assert room >= 1
    for extra in (1, room, room + 1):
        c = np.concatenate([good, np.zeros(4 * extra, dtype=np.uint8)])
        _dir(c, rl, nb, _dir(good, rl, nb) + extra)
        _refused(cp, c)
    # a stored state below L; a state or a word changed: a stream ends elsewhere or the words do not come out even
    for p, off, raw, dwords, words in info:
        if raw:
            continue
        damaged(edit(lambda c: _dword(c, pay + 4 * off, 0xFFFF)))
        damaged(edit(lambda c: _dword(c, pay + 4 * off, _dword(good, pay + 4 * off) ^ 0x10000)))
        damaged(edit(lambda c: _dword(c, pay + 4 * off + 4, _dword(good, pay + 4 * off + 4) + 1)))
        if words:
            ns = min(groups[info.index((p, off, raw, dwords, words))], LANES)
            damaged(edit(lambda c: _dword(c, pay + 4 * (off + ns), _dword(good, pay + 4 * (off + ns)) ^ 0x4)))


def test_both_directions_refuse_their_arguments(coded_frame):
    cp, frame, good, rl, _ = coded_frame
    lib = N.lib()
    n = C.c_uint64()
    dst = np.zeros(rl.bound_bytes, dtype=np.uint8)
    out = np.zeros(_layout(cp).frame_bytes, dtype=np.uint8)
    fp, dp, gp, op = (a.ctypes.data_as(C.c_void_p) for a in (frame, dst, good, out))
    assert lib.csic_rans_layout_of(None, C.byref(N.CsicRansLayout())) == N.EINVAL_NULL
    assert lib.csic_rans_layout_of(C.byref(cp), None) == N.EINVAL_NULL
    assert lib.csic_rans_pack_host(None, fp, dp, dst.size, C.byref(n)) == N.EINVAL_NULL
    assert lib.csic_rans_pack_host(C.byref(cp), None, dp, dst.size, C.byref(n)) == N.EINVAL_NULL
    assert lib.csic_rans_pack_host(C.byref(cp), fp, None, dst.size, C.byref(n)) == N.EINVAL_NULL
    assert lib.csic_rans_pack_host(C.byref(cp), fp, dp, dst.size, None) == N.EINVAL_NULL
    assert lib.csic_rans_unpack_host(None, gp, good.size, op) == N.EINVAL_NULL
    assert lib.csic_rans_unpack_host(C.byref(cp), None, good.size, op) == N.EINVAL_NULL
    assert lib.csic_rans_unpack_host(C.byref(cp), gp, good.size, None) == N.EINVAL_NULL
    for unpack in (csic.rans_unpack_host,):
        with pytest.raises(csic.CsicIOError):
            unpack(cp, b"")
    # parameters the container refuses are refused here, with its statuses
    ycc = csic.make_c_params(45, 7, 4, 4, 5, 4, 3, 1, CSQ, in_format=N.FMT_YCBCR888X, out_format=N.FMT_ARGB8888)
    assert lib.csic_rans_layout_of(C.byref(ycc), C.byref(N.CsicRansLayout())) == lib.csic_rice_layout_of(C.byref(ycc), C.byref(N.CsicRiceLayout())) != N.OK
    assert N.CODING_RANS == 5
