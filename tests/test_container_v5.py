""".csic version 5 (a sequence through the temporal layer; include/csic.h) without a GPU: files written by the library against files
assembled independently with struct.pack + zlib.crc32 from the numpy delta of tests/delta_ref.py and the numpy encoders of
tests/test_pack_host.py / tests/test_rice_host.py, for both codings; the read side (frames, gop, stored sizes, inter groups); a committed
file that pins the format; every way a version-5 file can be damaged; and versions 1, 3 and 4 reading as before."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, load_png_rgb
from delta_ref import frame_buffers, map_buffers, ref_delta, ref_map_layout
from test_container import CANARY, CSQ, FIXTURE, _c_params, _fields, _layout, _random_sets
from test_container_v3 import FIXTURE_V3, _read_status, _stored
from test_pack_host import codes_of, lib_layout, ref_encode
from test_rice_host import ref_encode_rice, rice_layout

import csic_amd as csic

N = csic._native
FIXTURE_V5 = os.path.join(GOLDEN, "container_v5_16x16.csic")
CODINGS = {"groups": (N.CODING_GROUPS, ref_encode, lambda cp: lib_layout(cp).bound_bytes),
           "rice": (N.CODING_RICE, ref_encode_rice, lambda cp: rice_layout(cp).bound_bytes)}


def build_v5(fields, coding, gop, records, version=5, nframes=None, sizes=None):
    """A version-5 file from its parts, the CRC made right: only the defect a test puts into the parts remains."""
    sizes = [len(r) for r in records] if sizes is None else sizes
    body = struct.pack("<16i", *fields) + struct.pack("<II", coding, gop) + b"".join(struct.pack("<Q", s) for s in sizes) + b"".join(records)
    return b"CSIC" + struct.pack("<III", version, len(sizes) if nframes is None else nframes, zlib.crc32(body) & 0xFFFFFFFF) + body


def ref_records(frames, bits, gop, encode):
    """-> (the records, the coded difference frames, the maps, t per frame and plane)"""
    diffs, maps, ts = ref_delta(frames, bits, gop)
    coded = [encode(d, bits) for d in diffs]
    return [c if k % gop == 0 else maps[k] + c for k, c in enumerate(coded)], coded, maps, ts


def _sequence(oracle, rng, W, H, a, b, bits, f, op, rounding, avg, nframes):
    """Frames that share most of their pixels: each is the one before with a third redrawn."""
    argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
    frames = []
    for _ in range(nframes):
        frames.append(codes_of(oracle, W, H, a, b, bits, f, op, rounding, avg, argb))
        argb = argb.copy()
        lo = int(rng.integers(0, W * H))
        argb[lo:lo + W * H // 3 + 1] = rng.integers(0, 1 << 32, argb[lo:lo + W * H // 3 + 1].size, dtype=np.uint32)
    return frames


def _inter_counts(ts, nframes):
    return [[0, 0, 0] if ts[k] is None else [int(t.sum()) for t in ts[k]] for k in range(nframes)]


def test_both_codings_are_byte_identical_to_the_independent_assembly(oracle, tmp_path):
    seen = set()
    for i, (W, H, a, b, bits, f, op, rounding, avg, _, rng) in enumerate(_random_sets(24, 16800)):
        nframes = 1 + i % 5
        gop = (1, 2, 3, nframes + 1)[i % 4]
        name = ("groups", "rice")[i // 4 % 2]
        coding, encode, bound_of = CODINGS[name]
        cp = _c_params(W, H, a, b, bits, f, op, rounding, avg)
        lay, tag = _layout(cp), (W, H, a, b, bits, f, op, rounding, avg, nframes, gop, name)
        frames = _sequence(oracle, rng, W, H, a, b, bits, f, op, rounding, avg, nframes)
        records, coded, maps, ts = ref_records(frames, bits, gop, encode)
        want = build_v5(_fields(_stored(cp)), coding, gop, records)
        src, clean = frame_buffers(lay, frames, bits, CANARY), frame_buffers(lay, frames, bits, 0)
        path = str(tmp_path / f"s{i}.csic")
        csic.write_container(path, cp, src, coding=name, gop=gop)
        got = open(path, "rb").read()
        assert got == want, tag
        assert got[4:8] == struct.pack("<I", 5) and got[80:88] == struct.pack("<II", coding, gop), tag
        N.check(N.lib().csic_container_write_seq(os.fsencode(path + ".c"), C.byref(cp), src.ctypes.data_as(C.c_void_p), nframes, coding, gop))
        assert open(path + ".c", "rb").read() == want, tag
        # from coded difference frames and maps, as the device leaves them: rows of a stride, canaries behind the bytes that count
        stride, ms = bound_of(cp), ref_map_layout([c.size for c in frames[0]])[3]
        rows = np.full((nframes, stride), CANARY, dtype=np.uint8)
        for k, c in enumerate(coded):
            rows[k, :len(c)] = np.frombuffer(c, dtype=np.uint8)
        csic.write_container_coded(path + ".coded", cp, rows, [len(c) for c in coded], coding=name, maps=map_buffers(maps, ms, CANARY), gop=gop)
        assert open(path + ".coded", "rb").read() == want, tag
        # read side
        info = csic.container_info(path)
        assert (info.version, info.nframes, info.payload_bytes, info.file_bytes, info.gop) == (5, nframes, lay.payload_bytes, len(got), gop), tag
        assert _fields(info.params) == _fields(_stored(cp)), tag
        assert csic.container_coded_sizes(path).tolist() == [len(r) for r in records], tag
        assert csic.container_inter_groups(path).tolist() == _inter_counts(ts, nframes), tag
        rp, rn, rframes = csic.read_container(path)
        assert rn == nframes and _fields(rp) == _fields(_stored(cp)) and np.array_equal(rframes, clean), tag
        dirty = np.full(nframes * lay.frame_bytes, 0x5A, dtype=np.uint8)       # every byte outside the payload ranges is zeroed
        N.check(N.lib().csic_container_read(os.fsencode(path), dirty.ctypes.data_as(C.c_void_p), dirty.size))
        assert np.array_equal(dirty.reshape(nframes, -1), clean), tag
        seen.add((nframes > gop, name))
    assert seen == {(False, "groups"), (True, "groups"), (False, "rice"), (True, "rice")}


def _fixture_frames(oracle):
    """in16.png at 4:2:0, 6/5/5, factor 1 (what the version-1 and version-3 fixtures hold), then the same with a 4 x 4 patch inverted,
    then the first upside down: key, delta, key at gop 2."""
    rgb = load_png_rgb(os.path.join(GOLDEN, "inputs", "in16.png"))
    patched = rgb.copy()
    patched[4:8, 4:8] ^= 0xFF
    bits = (6, 5, 5)
    return bits, [codes_of(oracle, 16, 16, 2, 0, bits, 1, CSQ, 0, False, oracle.rgb_to_argb(np.ascontiguousarray(x)).reshape(-1))
                  for x in (rgb, patched, rgb[::-1])]


def test_committed_version_5_file(oracle, tmp_path):
    """tests/golden/container_v5_16x16.csic pins the format: three frames at gop 2 -- key, delta, key -- Rice-coded."""
    bits, frames = _fixture_frames(oracle)
    cp = _c_params(16, 16, 2, 0, bits, 1, CSQ)
    records, coded, maps, ts = ref_records(frames, bits, 2, ref_encode_rice)
    want = build_v5(_fields(cp), N.CODING_RICE, 2, records)
    data = open(FIXTURE_V5, "rb").read()
    assert data == want and len(data) < 1000
    assert data[:12] == b"CSIC" + struct.pack("<II", 5, 3) and data[80:88] == struct.pack("<II", 3, 2)
    assert struct.unpack("<3Q", data[88:112]) == tuple(len(r) for r in records) and len(data) == 112 + sum(len(r) for r in records)
    assert len(records[1]) == len(maps[1]) + len(coded[1]) and len(maps[1]) == 12 and any(maps[1])
    p5, n5, f5 = csic.read_container(FIXTURE_V5)
    assert n5 == 3 and _fields(p5) == _fields(cp) and np.array_equal(f5, frame_buffers(_layout(cp), frames, bits, 0))
    assert np.array_equal(f5[0], csic.read_container(FIXTURE)[2][0]) and np.array_equal(f5[0], csic.read_container(FIXTURE_V3)[2][0])
    info = csic.container_info(FIXTURE_V5)
    assert (info.version, info.nframes, info.gop, info.payload_bytes, info.file_bytes) == (5, 3, 2, 272, len(data))
    assert csic.container_inter_groups(FIXTURE_V5).tolist() == _inter_counts(ts, 3)
    assert len(records[1]) < len(records[0])                                    # the delta frame is the smaller record
    csic.write_container(str(tmp_path / "again.csic"), p5, f5, coding="rice", gop=2)
    assert open(tmp_path / "again.csic", "rb").read() == data


def test_versions_1_3_and_4_read_as_before(oracle, tmp_path):
    for path, version in ((FIXTURE, 1), (FIXTURE_V3, 3)):
        info = csic.container_info(path)
        assert (info.version, info.gop) == (version, 1)
        assert csic.container_inter_groups(path).tolist() == [[0, 0, 0]]
    _, _, frames = csic.read_container(FIXTURE)
    cp = csic.container_info(FIXTURE).params
    v4 = str(tmp_path / "v4.csic")
    csic.write_container(v4, cp, frames, coding="rice")
    assert csic.container_info(v4).version == 4 and csic.container_info(v4).gop == 1 and np.array_equal(csic.read_container(v4)[2], frames)
    gop = C.c_int32(7)
    assert N.lib().csic_container_gop(os.fsencode(v4), C.byref(gop)) == N.OK and gop.value == 1
    # the three existing writers give the bytes they gave: no gop means no version 5
    for name, fixture in (("raw", FIXTURE), ("groups", FIXTURE_V3)):
        csic.write_container(str(tmp_path / "w.csic"), cp, frames, coding=name)
        assert open(tmp_path / "w.csic", "rb").read() == open(fixture, "rb").read()


@pytest.fixture()
def good(oracle, tmp_path):
    """A valid four-frame version-5 file at gop 3, Rice-coded: (path, bytes, c_params, layout, records, coded frames, maps)."""
    rng = np.random.default_rng(16900)
    W, H, bits = 45, 7, (5, 4, 3)
    cp = _c_params(W, H, 4, 4, bits, 1, CSQ)
    frames = _sequence(oracle, rng, W, H, 4, 4, bits, 1, CSQ, 0, False, 4)
    records, coded, maps, _ = ref_records(frames, bits, 3, ref_encode_rice)
    path = str(tmp_path / "good.csic")
    csic.write_container(path, cp, frame_buffers(_layout(cp), frames, bits, 0), coding="rice", gop=3)
    data = open(path, "rb").read()
    assert data == build_v5(_fields(_stored(cp)), 3, 3, records)
    return path, data, cp, _layout(cp), records, coded, maps


DEFECTS = ["coding0", "coding2", "coding4", "gop0", "gop65536", "gop_other", "delta_record_short", "key_record_with_map", "size_above_bound",
           "size_not_dwords", "longer", "truncated", "table_cut", "crc", "map_pad_bit", "map_pad_bit_last", "nibble", "frame_sizes_swapped",
           "version6", "v5_header_v4_body"]


@pytest.mark.parametrize("defect", DEFECTS)
def test_read_refuses_a_damaged_file(good, tmp_path, defect):
    path, data, cp, lay, records, coded, maps = good
    fields = _fields(_stored(cp))
    rl, ml = rice_layout(cp), csic.delta_layout(cp)
    mb = ml.map_bytes
    top = rl.fixed_bytes + 4 * sum(b * (248 * q + 1) for b, q in zip(rl.blocks, (5, 4, 3)))
    assert list(ml.groups) == [10, 10, 10] and mb == 12 and len(records[1]) == mb + len(coded[1])

    def patched(k, at, fn):
        r = [bytearray(x) for x in records]
        r[k][at] = fn(r[k][at])
        return build_v5(fields, 3, 3, [bytes(x) for x in r])
    sizes = [len(r) for r in records]
    assert sizes[1] != sizes[2]
    bad = {
        "coding0": lambda: build_v5(fields, 0, 3, records),
        "coding2": lambda: build_v5(fields, 2, 3, records),
        "coding4": lambda: build_v5(fields, 4, 3, records),
        "gop0": lambda: build_v5(fields, 3, 0, records),
        "gop65536": lambda: build_v5(fields, 3, 65536, records),
        "gop_other": lambda: build_v5(fields, 3, 2, records),                    # frame 2 becomes a key frame whose record begins with a map
        "delta_record_short": lambda: build_v5(fields, 3, 3, [records[0], records[1][:mb + rl.fixed_bytes - 4]] + records[2:]),
        "key_record_with_map": lambda: build_v5(fields, 3, 3, [maps[1] + records[0]] + records[1:]),
        "size_above_bound": lambda: build_v5(fields, 3, 3, [records[0], records[1] + bytes(mb + top + 4 - sizes[1])] + records[2:]),
        "size_not_dwords": lambda: build_v5(fields, 3, 3, [records[0], records[1] + b"\0\0"] + records[2:]),
        "longer": lambda: build_v5(fields, 3, 3, records + [b"\0\0\0\0"], sizes=sizes),
        "truncated": lambda: build_v5(fields, 3, 3, records[:3] + [records[3][:-4]], sizes=sizes),
        "table_cut": lambda: data[:100],
        "crc": lambda: data[:-3] + bytes([data[-3] ^ 0x10]) + data[-2:],
        "map_pad_bit": lambda: patched(1, ml.map_offset[0] + 1, lambda v: v | 0x04),      # 10 groups: bit 10 of a section is padding
        "map_pad_bit_last": lambda: patched(2, mb - 1, lambda v: v | 0x80),
        "nibble": lambda: patched(1, mb + rl.modes_offset[1], lambda v: (v & 0xF0) | 5),  # Cb has 4 bits per code
        "frame_sizes_swapped": lambda: build_v5(fields, 3, 3, records, sizes=[sizes[0], sizes[2], sizes[1], sizes[3]]),
        "version6": lambda: build_v5(fields, 3, 3, records, version=6),
        "v5_header_v4_body": lambda: build_v5(fields, 3, 0, coded),                       # what version 4 holds behind a version-5 header
    }[defect]()
    p = str(tmp_path / (defect + ".csic"))
    open(p, "wb").write(bad)
    st, buf = _read_status(p, 4 * lay.frame_bytes)
    assert st == N.EFORMAT and N.lib().csic_last_error().decode() != ""
    assert np.all(buf == 0x5A) or np.all(buf == 0)                             # nothing of a refused file stays in the buffers
    with pytest.raises(csic.CsicIOError) as ei:
        csic.read_container(p)
    assert ei.value.status == N.EFORMAT
    info_st = N.lib().csic_container_info_of(os.fsencode(p), C.byref(N.CsicContainerInfo()))
    sizes_st = N.lib().csic_container_coded_sizes(os.fsencode(p), (C.c_uint64 * 4)(), 4)
    gop_st = N.lib().csic_container_gop(os.fsencode(p), C.byref(C.c_int32()))
    inter_st = N.lib().csic_container_inter_groups(os.fsencode(p), (C.c_uint64 * 12)(), 12)
    if defect in ("crc", "nibble", "frame_sizes_swapped"):                      # the CRC and the coded frames are csic_container_read's to check
        assert info_st == sizes_st == gop_st == N.OK and inter_st in (N.OK, N.EFORMAT)
    elif defect in ("map_pad_bit", "map_pad_bit_last"):                         # and the maps csic_container_inter_groups' as well
        assert info_st == sizes_st == gop_st == N.OK and inter_st == N.EFORMAT
    elif defect in ("gop_other", "key_record_with_map"):                        # a header that is consistent when the sizes happen to fit
        assert info_st in (N.OK, N.EFORMAT) and sizes_st == gop_st == info_st
    else:
        assert info_st == sizes_st == gop_st == inter_st == N.EFORMAT


def test_write_and_size_refusals(good, tmp_path):
    path, data, cp, lay, records, coded, maps = good
    L = N.lib()
    assert _read_status(path, 4 * lay.frame_bytes)[0] == N.OK
    for wrong in (4 * lay.frame_bytes - 1, lay.frame_bytes, 0):
        assert _read_status(path, wrong)[0] == N.EINVAL_SIZE
    frames = np.zeros((4, lay.frame_bytes), dtype=np.uint8)
    pf = frames.ctypes.data_as(C.c_void_p)
    out = os.fsencode(str(tmp_path / "w.csic"))
    seq = L.csic_container_write_seq
    assert seq(None, C.byref(cp), pf, 4, 3, 3) == N.EINVAL_NULL and seq(out, None, pf, 4, 3, 3) == N.EINVAL_NULL and seq(out, C.byref(cp), None, 4, 3, 3) == N.EINVAL_NULL
    for coding in (0, 2, 4, -1):
        assert seq(out, C.byref(cp), pf, 4, coding, 3) == N.EINVAL_FORMAT
    for gop in (0, -1, 65536):
        assert seq(out, C.byref(cp), pf, 4, 3, gop) == N.EINVAL_SIZE
    for nf in (0, -1, 65536):
        assert seq(out, C.byref(cp), pf, nf, 3, 3) == N.EINVAL_SIZE
    assert seq(out, C.byref(_c_params(45, 7, 3, 3, (5, 4, 3), 1, CSQ)), pf, 1, 3, 3) == N.EINVAL_CHROMA_A
    assert seq(os.fsencode(str(tmp_path / "no_such_dir" / "w.csic")), C.byref(cp), pf, 4, 3, 3) == N.EIO
    # write_coded_seq: NULLs, coding, gop, the strides, and every coded frame and every map validated before anything is written
    rl, ml = rice_layout(cp), csic.delta_layout(cp)
    stride, ms = rl.bound_bytes, ml.map_stride
    rows = np.zeros((4, stride), dtype=np.uint8)
    for k, c in enumerate(coded):
        rows[k, :len(c)] = np.frombuffer(c, dtype=np.uint8)
    mrows = map_buffers(maps, ms, 0)
    sizes = (C.c_uint64 * 4)(*[len(c) for c in coded])
    pr, pm = rows.ctypes.data_as(C.c_void_p), mrows.ctypes.data_as(C.c_void_p)
    cs = L.csic_container_write_coded_seq
    assert cs(out, C.byref(cp), pr, stride, sizes, pm, ms, 4, 3, 3) == N.OK and open(out, "rb").read() == data
    os.remove(out)
    for args in ((None, C.byref(cp), pr, stride, sizes, pm, ms), (out, None, pr, stride, sizes, pm, ms), (out, C.byref(cp), None, stride, sizes, pm, ms),
                 (out, C.byref(cp), pr, stride, None, pm, ms), (out, C.byref(cp), pr, stride, sizes, None, ms)):
        assert cs(*args, 4, 3, 3) == N.EINVAL_NULL
    assert cs(out, C.byref(cp), pr, stride, sizes, pm, ms, 4, 1, 3) == N.EFORMAT               # Rice-coded frames are no group-coded frames
    assert cs(out, C.byref(cp), pr, stride, sizes, pm, ms, 4, 2, 3) == N.EINVAL_FORMAT
    assert cs(out, C.byref(cp), pr, stride, sizes, pm, ms, 4, 3, 0) == N.EINVAL_SIZE
    assert cs(out, C.byref(cp), pr, stride, sizes, pm, ms, 0, 3, 3) == N.EINVAL_SIZE
    assert cs(out, C.byref(cp), pr, len(coded[0]) - 4, sizes, pm, ms, 4, 3, 3) == N.EINVAL_SIZE
    assert cs(out, C.byref(cp), pr, stride, sizes, pm, ml.map_bytes - 4, 4, 3, 3) == N.EINVAL_SIZE
    for frame, byte, bit in ((1, 1, 2), (0, 0, 0), (3, 4, 1)):                  # a padding bit; bits in the maps of the key frames 0 and 3
        m = mrows.copy()
        m[frame, byte] |= 1 << bit
        assert cs(out, C.byref(cp), pr, stride, sizes, m.ctypes.data_as(C.c_void_p), ms, 4, 3, 3) == N.EFORMAT
    rows[2, rl.modes_offset[0]] = (rows[2, rl.modes_offset[0]] & 0xF0) | 0x0E
    assert cs(out, C.byref(cp), pr, stride, sizes, pm, ms, 4, 3, 3) == N.EFORMAT
    assert not os.path.exists(out)
    with pytest.raises(csic.IllegalArgumentException):
        csic.write_container_coded(str(tmp_path / "w.csic"), cp, rows, [len(c) for c in coded], coding="rice", maps=mrows)      # maps without a gop
    # gop and inter_groups: NULLs, the wrong count, a missing file
    counts = (C.c_uint64 * 12)()
    assert L.csic_container_gop(None, C.byref(C.c_int32())) == N.EINVAL_NULL and L.csic_container_gop(os.fsencode(path), None) == N.EINVAL_NULL
    assert L.csic_container_inter_groups(None, counts, 12) == N.EINVAL_NULL and L.csic_container_inter_groups(os.fsencode(path), None, 12) == N.EINVAL_NULL
    assert L.csic_container_inter_groups(os.fsencode(path), counts, 4) == N.EINVAL_SIZE
    assert L.csic_container_inter_groups(os.fsencode(str(tmp_path / "missing.csic")), counts, 12) == N.EIO
    assert L.csic_container_gop(os.fsencode(str(tmp_path / "missing.csic")), C.byref(C.c_int32())) == N.EIO
