""".csic version 6 (a sequence through the motion-compensated layer; include/csic.h) without a GPU: files written by the library against
files assembled independently with struct.pack + zlib.crc32 from the numpy statement of tests/mc_ref.py and the numpy encoders of
tests/test_pack_host.py / tests/test_rice_host.py, for both codings and every range; the read side (frames, gop, range, stored sizes,
inter groups); every field's defect refused; and the fixtures of versions 1, 3, 4 and 5 reading as before."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from delta_ref import frame_buffers, map_buffers
from mc_ref import ref_mc_delta, ref_mc_layout
from test_container import CANARY, CSQ, FIXTURE, _c_params, _fields, _layout, _random_sets
from test_container_v3 import FIXTURE_V3, _read_status, _stored
from test_container_v5 import CODINGS, FIXTURE_V5, build_v5
from test_pack_host import codes_of
from test_rice_host import ref_encode_rice, rice_layout

import csic_amd as csic

N = csic._native


def build_v6(fields, coding, R, gop, records, **kw):
    """A version-6 file from its parts: version 5's layout, the word at 80 is coding | (R + 1) << 8."""
    return build_v5(fields, coding | (R + 1) << 8, gop, records, version=kw.pop("version", 6), **kw)


def _widths(lay):
    return [lay.geometry.y_width, lay.geometry.chroma_width, lay.geometry.chroma_width]


def ref_records(frames, bits, widths, gop, R, encode):
    """-> (the records, the coded difference frames, the maps, (table, nibbles) per frame and plane)"""
    diffs, maps, info = ref_mc_delta(frames, bits, widths, gop, R)
    coded = [encode(d, bits) for d in diffs]
    return [c if k % gop == 0 else maps[k] + c for k, c in enumerate(coded)], coded, maps, info


def _pan(oracle, rng, W, H, a, b, bits, f, op, rounding, avg, nframes):
    """A picture panned by (1, 2) pixels per frame, the edges repeated, a band of it redrawn in every frame."""
    argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32).reshape(H, W)
    frames = []
    for k in range(nframes):
        x = argb[np.clip(np.arange(H) + k, 0, H - 1)][:, np.clip(np.arange(W) + 2 * k, 0, W - 1)].copy()
        x[(k * 3) % H] = rng.integers(0, 1 << 32, W, dtype=np.uint32)
        frames.append(codes_of(oracle, W, H, a, b, bits, f, op, rounding, avg, np.ascontiguousarray(x).reshape(-1)))
    return frames


def _inter_counts(info, nframes):
    return [[0, 0, 0] if info[k] is None else [int(np.count_nonzero(nib)) for _, nib in info[k]] for k in range(nframes)]


def test_both_codings_are_byte_identical_to_the_independent_assembly(oracle, tmp_path):
    seen = set()
    for i, (W, H, a, b, bits, f, op, rounding, avg, _, rng) in enumerate(_random_sets(24, 18800)):
        nframes = 1 + i % 5
        gop = (1, 2, 3, nframes + 1)[i % 4]
        R = (2, 0, 1, 7, 3)[i % 5]
        name = ("groups", "rice")[i // 4 % 2]
        coding, encode, bound_of = CODINGS[name]
        cp = _c_params(W, H, a, b, bits, f, op, rounding, avg)
        lay, tag = _layout(cp), (W, H, a, b, bits, f, op, rounding, avg, nframes, gop, R, name)
        frames = _pan(oracle, rng, W, H, a, b, bits, f, op, rounding, avg, nframes)
        records, coded, maps, minfo = ref_records(frames, bits, _widths(lay), gop, R, encode)
        want = build_v6(_fields(_stored(cp)), coding, R, gop, records)
        src, clean = frame_buffers(lay, frames, bits, CANARY), frame_buffers(lay, frames, bits, 0)
        path = str(tmp_path / f"s{i}.csic")
        csic.write_container(path, cp, src, coding=name, gop=gop, motion=R)
        got = open(path, "rb").read()
        assert got == want, tag
        assert got[4:8] == struct.pack("<I", 6) and got[80:88] == struct.pack("<II", coding | (R + 1) << 8, gop), tag
        N.check(N.lib().csic_container_write_seq_ex(os.fsencode(path + ".c"), C.byref(cp), src.ctypes.data_as(C.c_void_p), nframes, coding, gop, R))
        assert open(path + ".c", "rb").read() == want, tag
        # from coded difference frames and maps, as the device leaves them: rows of a stride, canaries behind the bytes that count
        stride, ms = bound_of(cp), ref_mc_layout([c.size for c in frames[0]])[4]
        rows = np.full((nframes, stride), CANARY, dtype=np.uint8)
        for k, c in enumerate(coded):
            rows[k, :len(c)] = np.frombuffer(c, dtype=np.uint8)
        csic.write_container_coded(path + ".coded", cp, rows, [len(c) for c in coded], coding=name, maps=map_buffers(maps, ms, CANARY), gop=gop, motion=R)
        assert open(path + ".coded", "rb").read() == want, tag
        # read side
        info = csic.container_info(path)
        assert (info.version, info.nframes, info.payload_bytes, info.file_bytes, info.gop, info.motion, info.coding) == \
            (6, nframes, lay.payload_bytes, len(got), gop, R, coding), tag
        assert _fields(info.params) == _fields(_stored(cp)), tag
        assert csic.container_coded_sizes(path).tolist() == [len(r) for r in records], tag
        assert csic.container_inter_groups(path).tolist() == _inter_counts(minfo, nframes), tag
        rp, rn, rframes = csic.read_container(path)
        assert rn == nframes and _fields(rp) == _fields(_stored(cp)) and np.array_equal(rframes, clean), tag
        dirty = np.full(nframes * lay.frame_bytes, 0x5A, dtype=np.uint8)       # every byte outside the payload ranges is zeroed
        N.check(N.lib().csic_container_read(os.fsencode(path), dirty.ctypes.data_as(C.c_void_p), dirty.size))
        assert np.array_equal(dirty.reshape(nframes, -1), clean), tag
        seen.add((nframes > gop, name))
    assert seen == {(False, "groups"), (True, "groups"), (False, "rice"), (True, "rice")}


def test_versions_1_3_4_and_5_read_as_before(tmp_path):
    for path, version, gop in ((FIXTURE, 1, 1), (FIXTURE_V3, 3, 1), (FIXTURE_V5, 5, 2)):
        info = csic.container_info(path)
        assert (info.version, info.gop, info.motion) == (version, gop, -1)
        motion = C.c_int32(7)
        assert N.lib().csic_container_motion(os.fsencode(path), C.byref(motion)) == N.OK and motion.value == -1
    _, _, frames = csic.read_container(FIXTURE)
    cp = csic.container_info(FIXTURE).params
    v4 = str(tmp_path / "v4.csic")
    csic.write_container(v4, cp, frames, coding="rice")
    assert csic.container_info(v4).version == 4 and csic.container_info(v4).motion == -1 and np.array_equal(csic.read_container(v4)[2], frames)
    # the existing writers give the bytes they gave: no motion means no version 6
    p5, _, f5 = csic.read_container(FIXTURE_V5)
    csic.write_container(str(tmp_path / "w5.csic"), p5, f5, coding="rice", gop=2)
    assert open(tmp_path / "w5.csic", "rb").read() == open(FIXTURE_V5, "rb").read()
    for name, fixture in (("raw", FIXTURE), ("groups", FIXTURE_V3)):
        csic.write_container(str(tmp_path / "w.csic"), cp, frames, coding=name)
        assert open(tmp_path / "w.csic", "rb").read() == open(fixture, "rb").read()
    # the same frames at range 0 make the choices of version 5, in version 6's maps
    csic.write_container(str(tmp_path / "w6.csic"), p5, f5, coding="rice", gop=2, motion=0)
    assert csic.container_info(str(tmp_path / "w6.csic")).version == 6
    assert csic.container_inter_groups(str(tmp_path / "w6.csic")).tolist() == csic.container_inter_groups(FIXTURE_V5).tolist()
    assert np.array_equal(csic.read_container(str(tmp_path / "w6.csic"))[2], f5)


@pytest.fixture()
def good(oracle, tmp_path):
    """A valid four-frame version-6 file at gop 3 and range 2, Rice-coded: (path, bytes, c_params, layout, records, coded frames, maps)."""
    rng = np.random.default_rng(18900)
    W, H, bits = 45, 7, (5, 4, 3)
    cp = _c_params(W, H, 4, 4, bits, 1, CSQ)
    frames = _pan(oracle, rng, W, H, 4, 4, bits, 1, CSQ, 0, False, 4)
    records, coded, maps, _ = ref_records(frames, bits, [W] * 3, 3, 2, ref_encode_rice)
    path = str(tmp_path / "good.csic")
    csic.write_container(path, cp, frame_buffers(_layout(cp), frames, bits, 0), coding="rice", gop=3, motion=2)
    data = open(path, "rb").read()
    assert data == build_v6(_fields(_stored(cp)), 3, 2, 3, records)
    return path, data, cp, _layout(cp), records, coded, maps


DEFECTS = ["motion0", "motion9", "high_bit", "coding0", "coding2", "gop0", "gop65536", "gop_other", "delta_record_short", "key_record_with_map",
           "size_above_bound", "size_not_dwords", "longer", "truncated", "table_cut", "crc", "table_size", "table_word1", "table_unused",
           "nibble_above", "pad_nibble", "pad_nibble_last", "coded_nibble", "frame_sizes_swapped", "version7", "v6_header_v5_maps"]


@pytest.mark.parametrize("defect", DEFECTS)
def test_read_refuses_a_damaged_file(good, tmp_path, defect):
    path, data, cp, lay, records, coded, maps = good
    fields = _fields(_stored(cp))
    rl, ml = rice_layout(cp), csic.mc_layout(cp)
    mb = ml.map_bytes
    top = rl.fixed_bytes + 4 * sum(b * (248 * q + 1) for b, q in zip(rl.blocks, (5, 4, 3)))
    assert list(ml.groups) == [10, 10, 10] and mb == 192 + 3 * 8 and len(records[1]) == mb + len(coded[1])
    T = maps[1][0]
    assert 1 <= T < 15

    def patched(k, at, fn):
        r = [bytearray(x) for x in records]
        r[k][at] = fn(r[k][at])
        return build_v6(fields, 3, 2, 3, [bytes(x) for x in r])
    sizes = [len(r) for r in records]
    assert sizes[1] != sizes[2]
    bad = {
        "motion0": lambda: build_v5(fields, 3, 3, records, version=6),            # the word a version-5 body has there
        "motion9": lambda: build_v5(fields, 3 | 9 << 8, 3, records, version=6),
        "high_bit": lambda: build_v5(fields, 3 | 3 << 8 | 1 << 16, 3, records, version=6),
        "coding0": lambda: build_v6(fields, 0, 2, 3, records),
        "coding2": lambda: build_v6(fields, 2, 2, 3, records),
        "gop0": lambda: build_v6(fields, 3, 2, 0, records),
        "gop65536": lambda: build_v6(fields, 3, 2, 65536, records),
        "gop_other": lambda: build_v6(fields, 3, 2, 2, records),                  # frame 2 becomes a key frame whose record begins with a map
        "delta_record_short": lambda: build_v6(fields, 3, 2, 3, [records[0], records[1][:mb + rl.fixed_bytes - 4]] + records[2:]),
        "key_record_with_map": lambda: build_v6(fields, 3, 2, 3, [maps[1] + records[0]] + records[1:]),
        "size_above_bound": lambda: build_v6(fields, 3, 2, 3, [records[0], records[1] + bytes(mb + top + 4 - sizes[1])] + records[2:]),
        "size_not_dwords": lambda: build_v6(fields, 3, 2, 3, [records[0], records[1] + b"\0\0"] + records[2:]),
        "longer": lambda: build_v6(fields, 3, 2, 3, records + [b"\0\0\0\0"], sizes=sizes),
        "truncated": lambda: build_v6(fields, 3, 2, 3, records[:3] + [records[3][:-4]], sizes=sizes),
        "table_cut": lambda: data[:100],
        "crc": lambda: data[:-3] + bytes([data[-3] ^ 0x10]) + data[-2:],
        "table_size": lambda: patched(1, 64, lambda v: 16),                       # T of the Cb table
        "table_word1": lambda: patched(2, 4, lambda v: 1),                        # the zero vector's word
        "table_unused": lambda: patched(1, 128 + 4 * 15, lambda v: 1),            # the last word of the Cr table: T < 15
        "nibble_above": lambda: patched(1, ml.map_offset[0], lambda v: (v & 0xF0) | (T + 1)),
        "pad_nibble": lambda: patched(1, ml.map_offset[0] + 5, lambda v: v | 0x01),        # 10 groups: nibble 10 of a section is padding
        "pad_nibble_last": lambda: patched(2, mb - 1, lambda v: v | 0x80),
        "coded_nibble": lambda: patched(1, mb + rl.modes_offset[1], lambda v: (v & 0xF0) | 5),   # Cb has 4 bits per code
        "frame_sizes_swapped": lambda: build_v6(fields, 3, 2, 3, records, sizes=[sizes[0], sizes[2], sizes[1], sizes[3]]),
        "version7": lambda: build_v6(fields, 3, 2, 3, records, version=7),
        "v6_header_v5_maps": lambda: build_v6(fields, 3, 2, 3, [records[0], bytes(12) + coded[1], bytes(12) + coded[2], records[3]]),
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
    motion_st = N.lib().csic_container_motion(os.fsencode(p), C.byref(C.c_int32()))
    inter_st = N.lib().csic_container_inter_groups(os.fsencode(p), (C.c_uint64 * 12)(), 12)
    assert motion_st == gop_st
    if defect in ("crc", "coded_nibble", "frame_sizes_swapped"):                # the CRC and the coded frames are csic_container_read's to check
        assert info_st == sizes_st == gop_st == N.OK and inter_st in (N.OK, N.EFORMAT)
    elif defect in ("table_size", "table_word1", "table_unused", "nibble_above", "pad_nibble", "pad_nibble_last"):
        assert info_st == sizes_st == gop_st == N.OK and inter_st == N.EFORMAT  # and the maps csic_container_inter_groups' as well
    elif defect in ("gop_other", "key_record_with_map", "v6_header_v5_maps"):   # a header that is consistent when the sizes happen to fit
        assert info_st in (N.OK, N.EFORMAT) and sizes_st == gop_st == info_st
    else:
        assert info_st == sizes_st == gop_st == inter_st == N.EFORMAT


def test_write_refusals(good, tmp_path):
    path, data, cp, lay, records, coded, maps = good
    L = N.lib()
    _, _, frames = csic.read_container(path)
    out = str(tmp_path / "x.csic")
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for R in (-1, 8):
        assert L.csic_container_write_seq_ex(os.fsencode(out), C.byref(cp), p(frames), 4, 3, 3, R) == N.EINVAL_SIZE
    assert L.csic_container_write_seq_ex(os.fsencode(out), C.byref(cp), p(frames), 4, 0, 3, 2) == N.EINVAL_FORMAT
    assert L.csic_container_write_seq_ex(os.fsencode(out), C.byref(cp), p(frames), 4, 3, 0, 2) == N.EINVAL_SIZE
    assert L.csic_container_write_seq_ex(None, C.byref(cp), p(frames), 4, 3, 3, 2) == N.EINVAL_NULL
    assert L.csic_container_motion(os.fsencode(path), None) == N.EINVAL_NULL
    assert not os.path.exists(out)
    with pytest.raises(csic.IllegalArgumentException):
        csic.write_container(out, cp, frames, coding="rice", motion=2)           # motion needs a gop
    # coded frames with maps that csic_mc_undelta_host would refuse are refused before anything is written
    ml = csic.mc_layout(cp)
    stride = rice_layout(cp).bound_bytes
    rows = np.zeros((4, stride), dtype=np.uint8)
    for k, c in enumerate(coded):
        rows[k, :len(c)] = np.frombuffer(c, dtype=np.uint8)
    good_maps = map_buffers(maps, ml.map_stride, 0)
    csic.write_container_coded(out, cp, rows, [len(c) for c in coded], coding="rice", maps=good_maps, gop=3, motion=2)
    assert open(out, "rb").read() == data
    os.remove(out)
    for frame, at, v in ((1, 0, 16), (0, 3, 1), (1, ml.map_offset[2] + 7, 0x10)):
        m = good_maps.copy()
        m[frame, at] = v
        with pytest.raises(csic.CsicIOError):
            csic.write_container_coded(out, cp, rows, [len(c) for c in coded], coding="rice", maps=m, gop=3, motion=2)
        assert not os.path.exists(out)
    sz = (C.c_uint64 * 4)(*[len(c) for c in coded])
    assert L.csic_container_write_coded_seq_ex(os.fsencode(out), C.byref(cp), p(rows), stride, sz, p(good_maps), ml.map_bytes - 1, 4, 3, 3, 2) == N.EINVAL_SIZE
    assert L.csic_container_write_coded_seq_ex(os.fsencode(out), C.byref(cp), p(rows), stride, sz, p(good_maps), ml.map_stride, 4, 3, 3, 9) == N.EINVAL_SIZE


def test_inspect_names_the_lowest_ranked_vector_of_an_offset():
    """`inspect` prints a table word as the candidate the encoder meant: in a plane narrower than twice the range several (dy, dx) have
    the same flat offset, and the one of lowest rank got the votes."""
    from csic_amd.app import _vector_of
    from mc_ref import candidates
    for w, R in ((512, 2), (45, 7), (8, 7), (4, 2), (3, 7), (1, 1)):
        seen = {}
        for dy, dx in candidates(R):                         # rank order: the first of an offset is the lowest-ranked
            seen.setdefault(dy * w + dx, f"({dy}, {dx})")
        for s, want in seen.items():
            assert _vector_of(s, w, R) == want, (w, R, s)
        assert _vector_of(R * w + R + 1, w, R) == f"offset {R * w + R + 1}"
