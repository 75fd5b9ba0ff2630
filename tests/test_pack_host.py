"""The group coding on the host (csic_pack_layout_of, csic_pack_host, csic_unpack_host; include/csic.h) without a GPU, against a numpy
encoder and decoder written here straight from the definition: they share nothing with the library (the anchors go through the bit
packer of test_container.py).  Planes come from the oracle's planar form.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_png_rgb
from test_container import CANARY, CSQ, _c_params, _frame_buffer, _layout, _random_sets, pack_codes

import csic_amd as csic

N = csic._native


# ---- the definition, in numpy ---------------------------------------------------------------------
def codes_of(oracle, W, H, a, b, bits, f, op, rounding, avg, argb):
    """The three planes' codes (v >> (8 - q)) of one frame, from the oracle's planar form."""
    p = oracle.OracleParams(width=W, height=H, chroma_a=a, chroma_b=b, y_bits=bits[0], cb_bits=bits[1], cr_bits=bits[2], factor=f,
                            op=op, rounding=rounding)
    _, y, cb, cr = oracle.planar(p, argb, avg=avg)
    return [np.asarray(v, dtype=np.uint8).reshape(-1).astype(np.int64) >> (8 - q) for v, q in zip((y, cb, cr), bits)]


def _pad4(b):
    return b + bytes(-len(b) % 4)


def ref_groups(codes, q):
    """One plane -> (w, anchors, u): per group its width, its anchor and its 32 folded residuals."""
    n = codes.size
    G = (n + 31) // 32
    c = np.concatenate([codes, np.full(32 * G - n, codes[-1], dtype=np.int64)]).reshape(G, 32)
    e = np.zeros_like(c)
    e[:, 1:] = (c[:, 1:] - c[:, :-1]) % (1 << q)
    s = np.where(e < (1 << (q - 1)), e, e - (1 << q))
    u = np.where(s >= 0, 2 * s, -2 * s - 1)
    assert u.min() >= 0 and u.max() < (1 << q)
    w = np.array([int(m).bit_length() for m in u.max(axis=1)], dtype=np.int64)
    return w, c[:, 0], u


def ref_encode(planes, bits, force=None):
    """Three planes of codes -> the coded frame's bytes.  force = w: every group is stored at max(w_g, w) bits per slot, wider than
    necessary (what another encoder may write)."""
    parts = [ref_groups(c, q) for c, q in zip(planes, bits)]
    if force is not None:
        parts = [(np.maximum(w, force), a, u) for w, a, u in parts]
    out = b""
    for w, _, _ in parts:                                  # 1. widths: nibble g at bits [4 g, 4 g + 4)
        nib = np.zeros((w.size + 7) // 8 * 8, dtype=np.uint8)
        nib[:w.size] = w
        out += (nib[0::2] | (nib[1::2] << 4)).astype(np.uint8).tobytes()
    for (w, anchors, _), q in zip(parts, bits):            # 2. anchors: a PLANAR_BITS-style plane of G codes
        out += _pad4(pack_codes(anchors.astype(np.uint8) << (8 - q), q).tobytes())
    for w, _, u in parts:                                  # 3. payload: slot j at bits [j w, j w + w) of the group's w dwords
        offs = np.concatenate([[0], np.cumsum(4 * w)])
        pay = np.zeros(offs[-1], dtype=np.uint8)
        for wv in range(1, 9):                             # (group by group in effect: all groups of one width at a time)
            sel = np.flatnonzero(w == wv)
            if sel.size:
                slot_bits = ((u[sel][:, :, None] >> np.arange(wv)) & 1).astype(np.uint8).reshape(sel.size, 32 * wv)
                pay[offs[sel][:, None] + np.arange(4 * wv)] = np.packbits(slot_bits, axis=1, bitorder="little")
        out += pay.tobytes()
    return out


def ref_layout(ns, bits):
    G = [(n + 31) // 32 for n in ns]
    wsz = [4 * ((g + 7) // 8) for g in G]
    asz = [4 * ((g * q + 31) // 32) for g, q in zip(G, bits)]
    woff = [0, wsz[0], wsz[0] + wsz[1]]
    fixed_w = sum(wsz)
    aoff = [fixed_w, fixed_w + asz[0], fixed_w + asz[0] + asz[1]]
    fixed = fixed_w + sum(asz)
    bound = (fixed + 4 * sum(g * q for g, q in zip(G, bits)) + 255) // 256 * 256
    return G, woff, aoff, fixed, bound


def ref_decode(coded, ns, bits):
    """Coded bytes -> three planes of codes, by the decode rule."""
    G, woff, aoff, fixed, _ = ref_layout(ns, bits)
    raw = np.frombuffer(coded, dtype=np.uint8)
    allbits = np.unpackbits(raw, bitorder="little")
    pos = fixed * 8
    planes = []
    for p, (n, q) in enumerate(zip(ns, bits)):
        out = np.zeros(32 * G[p], dtype=np.int64)
        for g in range(G[p]):
            w = (int(raw[woff[p] + g // 2]) >> (4 * (g % 2))) & 15
            ab = allbits[aoff[p] * 8 + g * q: aoff[p] * 8 + g * q + q]
            c = int((ab.astype(np.int64) << np.arange(q)).sum())
            out[32 * g] = c
            for j in range(1, 32):
                ub = allbits[pos + j * w: pos + j * w + w]
                u = int((ub.astype(np.int64) << np.arange(w)).sum()) if w else 0
                s = u // 2 if u % 2 == 0 else -(u + 1) // 2
                c = (c + s) % (1 << q)
                out[32 * g + j] = c
            pos += 32 * w
        planes.append(out[:n])
    assert pos == 8 * len(coded)
    return planes


def plane_bytes(codes, q):
    return pack_codes(codes.astype(np.uint8) << (8 - q), q)


# ---- calling the library ----------------------------------------------------------------------------
def lib_layout(cp):
    lay = N.CsicPackLayout()
    N.check(N.lib().csic_pack_layout_of(C.byref(cp), C.byref(lay)))
    return lay


def lib_pack(cp, frame, capacity=None, fill=CANARY):
    """-> (status, the whole destination buffer, coded_bytes)"""
    cap = lib_layout(cp).bound_bytes if capacity is None else capacity
    dst = np.full(max(cap, 1), fill, dtype=np.uint8)
    n = C.c_uint64(0)
    st = N.lib().csic_pack_host(C.byref(cp), frame.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    return st, dst, n.value


def lib_unpack(cp, coded, fill=CANARY):
    """-> (status, the whole frame buffer, pre-filled with `fill`)"""
    coded = np.frombuffer(bytes(coded), dtype=np.uint8) if not isinstance(coded, np.ndarray) else coded
    src = np.ascontiguousarray(coded) if coded.size else np.zeros(1, dtype=np.uint8)
    out = np.full(_layout(cp).frame_bytes, fill, dtype=np.uint8)
    st = N.lib().csic_unpack_host(C.byref(cp), src.ctypes.data_as(C.c_void_p), coded.size, out.ctypes.data_as(C.c_void_p))
    return st, out


def check_frame(cp, planes, bits, decode=True):
    """One frame through csic_pack_host and csic_unpack_host against the numpy reference, canaries included.  decode = False leaves
    out the numpy decoder, a loop per sample, for a large frame."""
    lay, pl = _layout(cp), lib_layout(cp)
    pbytes = [plane_bytes(c, q) for c, q in zip(planes, bits)]
    want = ref_encode(planes, bits)
    frame = _frame_buffer(lay, pbytes, CANARY)
    st, dst, size = lib_pack(cp, frame)
    assert st == N.OK and size == len(want) and dst[:size].tobytes() == want
    assert pl.fixed_bytes <= size <= pl.bound_bytes and np.all(dst[size:] == CANARY)
    # neither the padding of the source nor the unused high bits of a plane's last byte are read into a value
    other = _frame_buffer(lay, pbytes, 0x11)
    for off, nb, c, q in zip((lay.y_offset, lay.cb_offset, lay.cr_offset), (lay.y_bytes, lay.cb_bytes, lay.cr_bytes), planes, bits):
        if (c.size * q) % 8:
            other[off + nb - 1] |= (0xFF << ((c.size * q) % 8)) & 0xFF
    st, dst2, size2 = lib_pack(cp, other)
    assert st == N.OK and size2 == size and dst2[:size].tobytes() == want
    # decode: the payload ranges come back, the canary around them stays
    st, back = lib_unpack(cp, dst[:size])
    assert st == N.OK and np.array_equal(back, frame)
    if decode:
        assert [c.tolist() for c in ref_decode(want, [c.size for c in planes], bits)] == [c.tolist() for c in planes]
    return size


# ---- the worked vectors --------------------------------------------------------------------------------
def test_worked_vectors():
    w, a, u = ref_groups(np.array([1, 2, 3, 4, 5, 6, 7, 0], dtype=np.int64), 3)
    assert w.tolist() == [2] and a.tolist() == [1] and u[0].tolist() == [0] + [2] * 7 + [0] * 24
    w, a, u = ref_groups(np.array([0x1F, 0, 0x15], dtype=np.int64), 5)
    assert w.tolist() == [5] and a.tolist() == [0x1F] and u[0].tolist() == [0, 2, 21] + [0] * 29
    # the first one through the library, as the Y plane of an 8 x 1 frame at 3/3/3 (all planes alike at 4:4:4)
    cp = _c_params(8, 1, 4, 4, (3, 3, 3), 1, CSQ)
    planes = [np.array([1, 2, 3, 4, 5, 6, 7, 0], dtype=np.int64)] * 3
    frame = _frame_buffer(_layout(cp), [plane_bytes(c, 3) for c in planes], CANARY)
    assert frame[:3].tobytes().hex() == "d1581f"
    st, dst, size = lib_pack(cp, frame)
    assert st == N.OK and size == 48
    assert dst[:size].tobytes().hex() == "02000000" * 3 + "01000000" * 3 + "a8aa000000000000" * 3
    assert dst[:size].tobytes() == ref_encode(planes, (3, 3, 3))
    # the second: 3 x 1 at 5/5/5
    cp = _c_params(3, 1, 4, 4, (5, 5, 5), 1, CSQ)
    planes = [np.array([0x1F, 0, 0x15], dtype=np.int64)] * 3
    frame = _frame_buffer(_layout(cp), [plane_bytes(c, 5) for c in planes], CANARY)
    assert frame[:2].tobytes().hex() == "1f54"
    st, dst, size = lib_pack(cp, frame)
    assert st == N.OK and size == 12 + 12 + 3 * 20 and dst[:4].tobytes().hex() == "05000000" and dst[12:16].tobytes().hex() == "1f000000"
    assert dst[24:44].tobytes() == np.packbits(((np.array([0, 2, 21] + [0] * 29)[:, None] >> np.arange(5)) & 1).astype(np.uint8).reshape(-1),
                                               bitorder="little").tobytes()
    check_frame(cp, planes, (5, 5, 5))


# ---- random parameters ---------------------------------------------------------------------------------
def test_random_sets_match_the_reference_byte_for_byte(oracle):
    seen_bits, seen_w = set(), set()
    for (W, H, a, b, bits, f, op, rounding, avg, _, rng) in _random_sets(60, 9100):
        cp = _c_params(W, H, a, b, bits, f, op, rounding, avg)
        argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        if rng.random() < 0.5:                                # smooth content: widths below q
            argb = (np.arange(W * H, dtype=np.uint32) // 3 * np.uint32(0x010101)) | np.uint32(0xFF000000)
        planes = codes_of(oracle, W, H, a, b, bits, f, op, rounding, avg, argb)
        lay = _layout(cp)
        assert [c.size for c in planes] == [lay.geometry.y_width * lay.geometry.y_height] + [lay.geometry.chroma_samples] * 2
        check_frame(cp, planes, bits)
        seen_bits |= set(bits)
        for c, q in zip(planes, bits):
            seen_w |= set(ref_groups(c, q)[0].tolist())
    assert seen_bits == set(range(1, 9)) and seen_w == set(range(0, 9))


def test_layout_matches_the_formulas(oracle):
    for (W, H, a, b, bits, f, op, rounding, avg, _, rng) in _random_sets(60, 9200):
        for fmt in (N.FMT_PLANAR_BITS, N.FMT_ARGB8888):        # out_format is ignored
            cp = _c_params(W, H, a, b, bits, f, op, rounding, avg, out_format=fmt)
            lay, pl = _layout(cp), lib_layout(cp)
            ns = [lay.geometry.y_width * lay.geometry.y_height] + [lay.geometry.chroma_samples] * 2
            G, woff, aoff, fixed, bound = ref_layout(ns, bits)
            assert list(pl.groups) == G and list(pl.widths_offset) == woff and list(pl.anchors_offset) == aoff
            assert pl.payload_offset == pl.fixed_bytes == fixed and pl.bound_bytes == bound and bound % 256 == 0
            assert _fields_equal(csic.pack_layout(cp), pl)


def _fields_equal(a, b):
    return bytes(a) == bytes(b)


def test_constant_and_noise_frames():
    rng = np.random.default_rng(9300)
    W, H = 70, 33
    for bits in ((8, 8, 8), (6, 5, 5), (1, 1, 1)):
        cp = _c_params(W, H, 2, 0, bits, 1, CSQ)
        lay, pl = _layout(cp), lib_layout(cp)
        ns = [lay.geometry.y_width * lay.geometry.y_height] + [lay.geometry.chroma_samples] * 2
        const = [np.full(n, (1 << q) - 1, dtype=np.int64) for n, q in zip(ns, bits)]
        assert check_frame(cp, const, bits) == pl.fixed_bytes          # every width 0: no payload at all
    cp = _c_params(W, H, 4, 4, (8, 8, 8), 1, CSQ)
    pl = lib_layout(cp)
    noise = [rng.integers(0, 256, W * H).astype(np.int64) for _ in range(3)]
    size = check_frame(cp, noise, (8, 8, 8))
    assert pl.fixed_bytes < size <= pl.bound_bytes
    # the worst case: every group at w = q (the residual -2^(q-1) in each) reaches fixed_bytes + 4 sum G q, still within the bound
    worst = [np.tile(np.array([0, 128], dtype=np.int64), (W * H + 1) // 2)[:W * H] for _ in range(3)]
    assert check_frame(cp, worst, (8, 8, 8)) == pl.fixed_bytes + 4 * sum(g * 8 for g in pl.groups) <= pl.bound_bytes


@pytest.mark.parametrize("n", [1, 31, 32, 33])
def test_planes_of_a_group_and_its_neighbours(n):
    """n x 1 at 4:4:4: every plane has exactly n samples -- one sample, a group less one, a whole group, a group and one."""
    rng = np.random.default_rng(9400 + n)
    for bits in ((8, 8, 8), (6, 5, 5), (3, 3, 2), (1, 7, 4)):
        cp = _c_params(n, 1, 4, 4, bits, 1, CSQ)
        assert list(lib_layout(cp).groups) == [(n + 31) // 32] * 3
        check_frame(cp, [rng.integers(0, 1 << q, n).astype(np.int64) for q in bits], bits)
        check_frame(cp, [np.arange(n, dtype=np.int64) % (1 << q) for q in bits], bits)


# ---- refusals ------------------------------------------------------------------------------------------------
@pytest.fixture()
def coded_frame():
    """A valid coded frame with widths in every plane: (c_params, frame buffer, coded bytes as a numpy array, layout)."""
    rng = np.random.default_rng(9500)
    W, H, bits = 45, 7, (5, 4, 3)                           # 315 samples: 10 groups, the anchors and the nibbles both end in padding
    cp = _c_params(W, H, 4, 4, bits, 1, CSQ)
    planes = [rng.integers(0, 1 << q, W * H).astype(np.int64) for q in bits]
    frame = _frame_buffer(_layout(cp), [plane_bytes(c, q) for c, q in zip(planes, bits)], CANARY)
    st, dst, size = lib_pack(cp, frame)
    assert st == N.OK
    return cp, frame, dst[:size].copy(), lib_layout(cp)


def _refused(cp, coded, status=None):
    st, out = lib_unpack(cp, coded)
    assert st == (N.EFORMAT if status is None else status), st
    assert N.lib().csic_last_error().decode() != ""
    assert np.all(out == CANARY)                               # a refused frame writes nothing
    if st == N.EFORMAT:
        with pytest.raises(csic.CsicIOError):
            csic.unpack_frame_host(cp, coded)


def test_unpack_refuses_damaged_input(coded_frame):
    cp, frame, coded, pl = coded_frame
    q = (5, 4, 3)
    assert lib_unpack(cp, coded)[0] == N.OK
    for p in range(3):
        bad = coded.copy()                                     # a nibble > q
        bad[pl.widths_offset[p]] = (bad[pl.widths_offset[p]] & 0xF0) | (q[p] + 1)
        _refused(cp, bad)
        bad = coded.copy()                                     # a nibble behind the last group (10 groups: nibbles 10 .. 15 are padding)
        bad[pl.widths_offset[p] + 7] |= 0x10
        _refused(cp, bad)
        bad = coded.copy()                                     # the last bit of the anchors section (10 q bits: 50 / 64, 40 / 64, 30 / 32)
        bad[pl.anchors_offset[p] + 4 * ((10 * q[p] + 31) // 32) - 1] |= 0x80
        _refused(cp, bad)
    _refused(cp, np.concatenate([coded, np.zeros(4, dtype=np.uint8)]))       # sizes off by +- 4, and not in dwords
    _refused(cp, coded[:-4])
    _refused(cp, coded[:-1])
    _refused(cp, coded[:pl.fixed_bytes - 4])
    _refused(cp, coded[:0])
    lower = coded.copy()                                       # a smaller width: the size no longer fits the widths
    w0 = lower[pl.widths_offset[0]] & 15
    assert w0 > 0
    lower[pl.widths_offset[0]] -= 1
    _refused(cp, lower)
    st, out = lib_unpack(cp, lower[:-4])                       # ... and with the size corrected it decodes to SOME valid frame
    assert st == N.OK
    st2, dst, size = lib_pack(cp, out)
    assert st2 == N.OK and size <= pl.bound_bytes


def test_pack_and_unpack_argument_refusals(coded_frame):
    cp, frame, coded, pl = coded_frame
    L = N.lib()
    size = coded.size
    for cap in (0, pl.fixed_bytes - 1, pl.fixed_bytes, size - 4, size - 1):
        st, dst, need = lib_pack(cp, frame, capacity=cap)
        assert st == N.EINVAL_SIZE, cap
        assert np.all(dst[cap:] == CANARY)
        if cap >= pl.fixed_bytes:
            assert need == size                                # the size that was needed
    st, dst, need = lib_pack(cp, frame, capacity=size)
    assert st == N.OK and need == size and np.array_equal(dst[:size], coded)
    n = C.c_uint64()
    pf, pc = frame.ctypes.data_as(C.c_void_p), coded.ctypes.data_as(C.c_void_p)
    assert L.csic_pack_host(None, pf, pc, size, C.byref(n)) == N.EINVAL_NULL
    assert L.csic_pack_host(C.byref(cp), None, pc, size, C.byref(n)) == N.EINVAL_NULL
    assert L.csic_pack_host(C.byref(cp), pf, None, size, C.byref(n)) == N.EINVAL_NULL
    assert L.csic_pack_host(C.byref(cp), pf, pc, size, None) == N.EINVAL_NULL
    assert L.csic_unpack_host(None, pc, size, pf) == N.EINVAL_NULL
    assert L.csic_unpack_host(C.byref(cp), None, size, pf) == N.EINVAL_NULL
    assert L.csic_unpack_host(C.byref(cp), pc, size, None) == N.EINVAL_NULL
    assert L.csic_pack_layout_of(None, C.byref(N.CsicPackLayout())) == N.EINVAL_NULL
    assert L.csic_pack_layout_of(C.byref(cp), None) == N.EINVAL_NULL
    # the statuses of csic_container_write: csic_validate's, and a YCbCr input stream cannot be PLANAR_BITS
    bad = _c_params(45, 7, 3, 3, (5, 4, 3), 1, CSQ)
    assert L.csic_pack_layout_of(C.byref(bad), C.byref(N.CsicPackLayout())) == N.EINVAL_CHROMA_A
    assert L.csic_pack_host(C.byref(bad), pf, pc, size, C.byref(n)) == N.EINVAL_CHROMA_A
    assert L.csic_unpack_host(C.byref(bad), pc, size, pf) == N.EINVAL_CHROMA_A
    bad = _c_params(45, 7, 4, 4, (5, 9, 3), 1, CSQ)
    assert L.csic_pack_host(C.byref(bad), pf, pc, size, C.byref(n)) == N.EINVAL_BITS
    ycc = csic.make_c_params(45, 7, 4, 4, 5, 4, 3, 1, CSQ, in_format=N.FMT_YCBCR888X, out_format=N.FMT_ARGB8888)
    assert L.csic_pack_host(C.byref(ycc), pf, pc, size, C.byref(n)) == N.EINVAL_FORMAT


# ---- the reference's image ---------------------------------------------------------------------------------
IN512_SETS = [  # a, b, bits, f, avg
    (2, 0, (6, 5, 5), 1, False), (2, 0, (6, 5, 5), 1, True), (2, 0, (6, 5, 5), 2, False), (2, 0, (3, 3, 2), 2, False), (4, 4, (8, 8, 8), 1, False),
]


def test_in512_codes_smaller_than_raw(oracle, capsys):
    """in512.png at five parameter sets: the library's size equals the numpy reference's and is below the raw planes'.  The printed
    sizes are the ones DESIGN.md 4.7 quotes."""
    rgb = load_png_rgb(os.path.join(GOLDEN, "inputs", "in512.png"))
    argb = oracle.rgb_to_argb(rgb).reshape(-1)
    lines = []
    for a, b, bits, f, avg in IN512_SETS:
        cp = _c_params(512, 512, a, b, bits, f, CSQ, 0, avg)
        lay = _layout(cp)
        planes = codes_of(oracle, 512, 512, a, b, bits, f, CSQ, 0, avg, argb)
        frame = _frame_buffer(lay, [plane_bytes(c, q) for c, q in zip(planes, bits)], CANARY)
        want = ref_encode(planes, bits)
        st, dst, size = lib_pack(cp, frame)
        assert st == N.OK and size == len(want) and dst[:size].tobytes() == want
        assert size < lay.payload_bytes
        st, back = lib_unpack(cp, dst[:size])
        assert st == N.OK and np.array_equal(back, frame)
        lines.append(f"4:{a}:{b} {bits[0]}/{bits[1]}/{bits[2]} f={f} {'AVG' if avg else 'HOLD'}: raw {lay.payload_bytes} coded {size} "
                     f"ratio {size / lay.payload_bytes:.3f}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
