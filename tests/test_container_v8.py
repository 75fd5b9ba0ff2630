""".csic version 8 (frames that stand alone, each through the row-prediction layer csic_rows_* and one of the three codings;
include/csic.h) without a GPU: files written by the library against files assembled independently with struct.pack + zlib.crc32 from
the numpy statement of tests/rows_ref.py and the reference encoders; the read side; the committed fixture; every field's defect refused
by name; the write refusals; versions 1 to 7 as before; `inspect`."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from conftest import load_png_rgb
from delta_ref import frame_buffers, map_buffers, ref_map_layout
from rows_ref import ref_rows
from test_container import CANARY, CSQ, FIXTURE, _c_params, _fields, _layout, _random_sets
from test_container_v3 import FIXTURE_V3, _read_status, _stored
from test_container_v5 import FIXTURE_V5, build_v5
from test_container_v7 import FIXTURE_V7, FIXTURE_V7_SEQ
from test_pack_host import codes_of, ref_encode
from test_rans_host import ref_encode_rans
from test_rice_host import ref_encode_rice
from test_rows_host import plane_widths

import csic_amd as csic

N = csic._native
GOLDEN = os.path.dirname(FIXTURE)
FIXTURE_V8 = os.path.join(GOLDEN, "container_v8_32x4.csic")
ENCODERS = {"groups": (N.CODING_GROUPS, ref_encode), "rice": (N.CODING_RICE, ref_encode_rice), "rans": (N.CODING_RANS, ref_encode_rans)}
FLAG = 1 << 16


def build_v8(fields, coding, records, word84=0, **kw):
    """A version-8 file from its parts: version 3's layout, the word at 80 is coding | 1 << 16, the word at 84 is 0, and every record is
    the frame's map followed by its coded difference frame."""
    return build_v5(fields, coding, word84, records, version=kw.pop("version", 8), **kw)


def ref_records(frames, widths, bits, encode):
    """-> (the records, the coded difference frames, the maps, t per frame and plane)"""
    out = [ref_rows(f, widths, bits) for f in frames]
    coded = [encode(d, bits) for d, _, _ in out]
    return [m + c for (_, m, _), c in zip(out, coded)], coded, [m for _, m, _ in out], [t for _, _, t in out]


def _smooth(oracle, rng, W, H, a, b, bits, f, op, rounding, avg, nframes):
    """Frames with rows that resemble the row above, so that both choices occur."""
    frames = []
    for _ in range(nframes):
        base = (np.cumsum(rng.integers(-3, 4, W)) % 256).astype(np.uint32)[None, :] + (np.arange(H, dtype=np.uint32) // 2)[:, None]
        argb = ((base % 256) * np.uint32(0x010101)).reshape(-1) ^ (rng.integers(0, 1 << 32, W * H, dtype=np.uint32) & np.uint32(0x00030101))
        frames.append(codes_of(oracle, W, H, a, b, bits, f, op, rounding, avg, argb))
    return frames


def test_files_are_byte_identical_to_the_independent_assembly(oracle, tmp_path):
    seen = set()
    for i, (W, H, a, b, bits, f, op, rounding, avg, _, rng) in enumerate(_random_sets(18, 23500)):
        W, H = 2 * W + 24, H + 6
        nframes = 1 + i % 3
        name = ("groups", "rice", "rans")[i % 3]
        coding, encode = ENCODERS[name]
        cp = _c_params(W, H, a, b, bits, f, op, rounding, avg)
        lay, tag = _layout(cp), (W, H, a, b, bits, f, op, rounding, avg, nframes, name)
        frames = _smooth(oracle, rng, W, H, a, b, bits, f, op, rounding, avg, nframes)
        records, coded, maps, ts = ref_records(frames, plane_widths(cp), bits, encode)
        want = build_v8(_fields(_stored(cp)), coding | FLAG, records)
        src, clean = frame_buffers(lay, frames, bits, CANARY), frame_buffers(lay, frames, bits, 0)
        path = str(tmp_path / f"s{i}.csic")
        csic.write_container(path, cp, src, coding=name, rows=True)
        got = open(path, "rb").read()
        assert got == want, tag
        assert got[4:8] == struct.pack("<I", 8) and got[80:88] == struct.pack("<II", coding | FLAG, 0), tag
        # from coded frames and maps as the device leaves them: rows of a stride, canaries behind the bytes that count
        bound = {"groups": csic.pack_layout, "rice": csic.rice_layout, "rans": csic.rans_layout}[name](cp).bound_bytes
        rows = np.full((nframes, bound), CANARY, dtype=np.uint8)
        for k, c in enumerate(coded):
            rows[k, :len(c)] = np.frombuffer(c, dtype=np.uint8)
        ms = ref_map_layout([c.size for c in frames[0]])[3]
        csic.write_container_coded(path + ".coded", cp, rows, [len(c) for c in coded], coding=name, maps=map_buffers(maps, ms, CANARY), rows=True)
        assert open(path + ".coded", "rb").read() == want, tag
        # read side
        info = csic.container_info(path)
        assert (info.version, info.nframes, info.payload_bytes, info.file_bytes, info.gop, info.motion, info.coding, info.rows) == \
            (8, nframes, lay.payload_bytes, len(got), 1, -1, coding, True), tag
        assert _fields(info.params) == _fields(_stored(cp)), tag
        assert csic.container_coded_sizes(path).tolist() == [len(r) for r in records], tag
        assert csic.container_inter_groups(path).tolist() == [[int(t.sum()) for t in fr] for fr in ts], tag
        rp, rn, rframes = csic.read_container(path)
        assert rn == nframes and _fields(rp) == _fields(_stored(cp)) and np.array_equal(rframes, clean), tag
        dirty = np.full(nframes * lay.frame_bytes, 0x5A, dtype=np.uint8)       # every byte outside the payload ranges is zeroed
        N.check(N.lib().csic_container_read(os.fsencode(path), dirty.ctypes.data_as(C.c_void_p), dirty.size))
        assert np.array_equal(dirty.reshape(nframes, -1), clean), tag
        seen |= {name} | {bool(t.any()) for fr in ts for t in fr}
    assert seen == {"groups", "rice", "rans", False, True}


def _fixture_frame(oracle):
    """The top four rows of in16.png twice side by side, the third row the second again: 32 x 4 at 4:2:0, 6/5/5, factor 1 -- Y rows of
    32 samples (K = 1), chroma rows of 16 (K = 0)."""
    rgb = np.tile(load_png_rgb(os.path.join(GOLDEN, "inputs", "in16.png"))[:4], (1, 2, 1))
    rgb[2] = rgb[1]
    bits = (6, 5, 5)
    return bits, codes_of(oracle, 32, 4, 2, 0, bits, 1, CSQ, 0, False, oracle.rgb_to_argb(np.ascontiguousarray(rgb)).reshape(-1))


def test_committed_version_8_file(oracle, tmp_path):
    """tests/golden/container_v8_32x4.csic pins the format: one frame, rANS-coded behind the layer."""
    bits, frame = _fixture_frame(oracle)
    cp = _c_params(32, 4, 2, 0, bits, 1, CSQ)
    records, coded, maps, ts = ref_records([frame], [32, 16, 16], bits, ref_encode_rans)
    data = open(FIXTURE_V8, "rb").read()
    assert data == build_v8(_fields(cp), N.CODING_RANS | FLAG, records) and len(data) < 1000
    assert data[:12] == b"CSIC" + struct.pack("<II", 8, 1) and data[80:88] == struct.pack("<II", 5 | FLAG, 0)
    assert struct.unpack("<Q", data[88:96]) == (len(maps[0]) + len(coded[0]),) and len(data) == 96 + len(records[0])
    assert len(maps[0]) == 12 and ts[0][0].tolist() == [False, False, True, False] and data[96:108] == b"\x04" + bytes(11)
    p8, n8, f8 = csic.read_container(FIXTURE_V8)
    assert n8 == 1 and _fields(p8) == _fields(cp) and np.array_equal(f8, frame_buffers(_layout(cp), [frame], bits, 0))
    info = csic.container_info(FIXTURE_V8)
    assert (info.version, info.nframes, info.gop, info.motion, info.coding, info.rows, info.file_bytes) == (8, 1, 1, -1, N.CODING_RANS, True, len(data))
    assert csic.container_inter_groups(FIXTURE_V8).tolist() == [[1, 0, 0]]
    csic.write_container(str(tmp_path / "again.csic"), p8, f8, coding="rans", rows=True)
    assert open(tmp_path / "again.csic", "rb").read() == data


def test_earlier_versions_read_and_write_as_before(tmp_path):
    for path, version, gop in ((FIXTURE, 1, 1), (FIXTURE_V3, 3, 1), (FIXTURE_V5, 5, 2), (FIXTURE_V7, 7, 1), (FIXTURE_V7_SEQ, 7, 2)):
        info = csic.container_info(path)
        assert (info.version, info.gop, info.rows) == (version, gop, False)
    cp, _, frames = csic.read_container(FIXTURE)
    for name, fixture in (("raw", FIXTURE), ("groups", FIXTURE_V3), ("rans", FIXTURE_V7)):
        csic.write_container(str(tmp_path / "w.csic"), cp, frames, coding=name)
        assert open(tmp_path / "w.csic", "rb").read() == open(fixture, "rb").read()
    p5, _, f5 = csic.read_container(FIXTURE_V5)
    csic.write_container(str(tmp_path / "w5.csic"), p5, f5, coding="rice", gop=2)
    assert open(tmp_path / "w5.csic", "rb").read() == open(FIXTURE_V5, "rb").read()
    ps, _, fs = csic.read_container(FIXTURE_V7_SEQ)
    csic.write_container(str(tmp_path / "w7.csic"), ps, fs, coding="rans", gop=2, motion=1)
    assert open(tmp_path / "w7.csic", "rb").read() == open(FIXTURE_V7_SEQ, "rb").read()


@pytest.fixture()
def good(oracle, tmp_path):
    """A valid two-frame version-8 file, Rice-coded, 40 x 10 at 4:2:0: Y has 13 groups in rows of 40 (K = 1), the chroma planes rows of
    20 (K = 0).  -> (path, bytes, c_params, layout, records, coded frames, maps)"""
    rng = np.random.default_rng(23600)
    W, H, bits = 40, 10, (5, 4, 3)
    cp = _c_params(W, H, 2, 0, bits, 1, CSQ)
    frames = _smooth(oracle, rng, W, H, 2, 0, bits, 1, CSQ, 0, False, 1)
    frames.append(codes_of(oracle, W, H, 2, 0, bits, 1, CSQ, 0, False, rng.integers(0, 1 << 32, W * H, dtype=np.uint32)))     # noise: another size
    records, coded, maps, ts = ref_records(frames, [40, 20, 20], bits, ref_encode_rice)
    assert ts[0][0].any()
    path = str(tmp_path / "good.csic")
    csic.write_container(path, cp, frame_buffers(_layout(cp), frames, bits, 0), coding="rice", rows=True)
    data = open(path, "rb").read()
    assert data == build_v8(_fields(_stored(cp)), N.CODING_RICE | FLAG, records)
    return path, data, cp, _layout(cp), records, coded, maps


DEFECTS = ["flag_bit_17", "flag_bit_8", "flag_missing", "word84", "coding0", "coding2", "coding4", "padding_bit", "bit_in_k0_plane", "truncated", "longer",
           "frame_sizes_swapped", "crc", "rans_word_rice_body", "v7_body", "v3_header"]


@pytest.mark.parametrize("defect", DEFECTS)
def test_read_refuses_a_damaged_file(good, tmp_path, defect):
    path, data, cp, lay, records, coded, maps = good
    fields = _fields(_stored(cp))
    ml = csic.rows_layout(cp)
    sizes = [len(r) for r in records]
    rice = N.CODING_RICE
    assert _read_status(path, 2 * lay.frame_bytes)[0] == N.OK and sizes[0] != sizes[1] and list(ml.groups) == [13, 4, 4]

    def patched(k, at, fn):
        r = [bytearray(x) for x in records]
        r[k][at] = fn(r[k][at])
        return build_v8(fields, rice | FLAG, [bytes(x) for x in r])
    bad = {
        "flag_bit_17": lambda: build_v8(fields, rice | FLAG | 1 << 17, records),
        "flag_bit_8": lambda: build_v8(fields, rice | FLAG | 1 << 8, records),                  # where versions 6 and 7 keep a motion range
        "flag_missing": lambda: build_v8(fields, rice, records),
        "word84": lambda: build_v8(fields, rice | FLAG, records, word84=1),
        "coding0": lambda: build_v8(fields, 0 | FLAG, records),
        "coding2": lambda: build_v8(fields, 2 | FLAG, records),
        "coding4": lambda: build_v8(fields, 4 | FLAG, records),
        "padding_bit": lambda: patched(1, ml.map_offset[0] + 1, lambda v: v | 0x20),          # bit 13 of Y's section: 13 groups
        "bit_in_k0_plane": lambda: patched(0, ml.map_offset[1], lambda v: v | 1),             # Cb rows are shorter than a group
        "truncated": lambda: build_v8(fields, rice | FLAG, [records[0], records[1][:-4]], sizes=sizes),
        "longer": lambda: build_v8(fields, rice | FLAG, records + [b"\0\0\0\0"], sizes=sizes),
        "frame_sizes_swapped": lambda: build_v8(fields, rice | FLAG, records, sizes=sizes[::-1]),
        "crc": lambda: data[:-3] + bytes([data[-3] ^ 0x10]) + data[-2:],
        "rans_word_rice_body": lambda: build_v8(fields, N.CODING_RANS | FLAG, records),
        "v7_body": lambda: build_v5(fields, 5 | 3 << 8, 3, records, version=8),               # a version-7 header's words under an 8
        "v3_header": lambda: build_v8(fields, rice | FLAG, records, version=4),               # the layer's word under a version without it
    }[defect]()
    p = str(tmp_path / (defect + ".csic"))
    open(p, "wb").write(bad)
    st, buf = _read_status(p, 2 * lay.frame_bytes)
    assert st == N.EFORMAT and N.lib().csic_last_error().decode() != ""
    assert np.all(buf == 0x5A) or np.all(buf == 0)                             # nothing of a refused file stays in the buffers
    with pytest.raises(csic.CsicIOError) as ei:
        csic.read_container(p)
    assert ei.value.status == N.EFORMAT
    info_st = N.lib().csic_container_info_of(os.fsencode(p), C.byref(N.CsicContainerInfo()))
    rows_st = N.lib().csic_container_rows(os.fsencode(p), C.byref(C.c_int32()))
    assert rows_st == info_st
    if defect in ("flag_bit_17", "flag_bit_8", "flag_missing", "word84", "coding0", "coding2", "coding4", "truncated", "longer", "v7_body", "v3_header"):
        assert info_st == N.EFORMAT                                             # the header alone says so
    elif defect in ("padding_bit", "bit_in_k0_plane", "crc", "frame_sizes_swapped"):
        assert info_st == N.OK                                                  # the CRC, the coded frames and the maps are csic_container_read's to check
    if defect in ("padding_bit", "bit_in_k0_plane"):
        assert N.lib().csic_container_inter_groups(os.fsencode(p), (C.c_uint64 * 6)(), 6) == N.EFORMAT


def test_write_refusals(good, tmp_path):
    path, data, cp, lay, records, coded, maps = good
    L = N.lib()
    _, _, frames = csic.read_container(path)
    out = str(tmp_path / "x.csic")
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for coding in (0, 2, 4, 6):                                                  # raw: the layer gains nothing without a coder
        assert L.csic_container_write_rows(os.fsencode(out), C.byref(cp), p(frames), 2, coding) == N.EINVAL_FORMAT
    assert L.csic_container_write_rows(None, C.byref(cp), p(frames), 2, 3) == N.EINVAL_NULL
    assert L.csic_container_write_rows(os.fsencode(out), C.byref(cp), None, 2, 3) == N.EINVAL_NULL
    assert L.csic_container_write_rows(os.fsencode(out), C.byref(cp), p(frames), 0, 3) == N.EINVAL_SIZE
    assert L.csic_container_rows(os.fsencode(path), None) == N.EINVAL_NULL
    assert not os.path.exists(out)
    for kw in ({"gop": 2}, {"gop": 2, "motion": 1}):                             # out of scope: refused, not half-built
        with pytest.raises(csic.IllegalArgumentException):
            csic.write_container(out, cp, frames, coding="rice", rows=True, **kw)
    with pytest.raises(csic.IllegalArgumentException):
        csic.write_container(out, cp, frames, coding="raw", rows=True)
    # from the device's output: every coded frame and every map is validated before anything is written
    ml, stride = csic.rows_layout(cp), csic.rice_layout(cp).bound_bytes
    rows = np.zeros((2, stride), dtype=np.uint8)
    for k, c in enumerate(coded):
        rows[k, :len(c)] = np.frombuffer(c, dtype=np.uint8)
    sizes = [len(c) for c in coded]
    mbuf = map_buffers(maps, ml.map_stride, CANARY)
    csic.write_container_coded(out, cp, rows, sizes, coding="rice", maps=mbuf, rows=True)
    assert open(out, "rb").read() == data
    os.remove(out)
    for frame, at, bit in ((1, ml.map_offset[0] + 1, 5), (0, ml.map_offset[2], 0)):      # a padding bit; a bit of a K = 0 plane
        m = mbuf.copy()
        m[frame, at] |= 1 << bit
        with pytest.raises(csic.CsicIOError):
            csic.write_container_coded(out, cp, rows, sizes, coding="rice", maps=m, rows=True)
        assert not os.path.exists(out)
    r = rows.copy()
    r[1, csic.rice_layout(cp).anchors_offset[0] + 8] ^= 0x80                     # an anchors padding bit (13 groups of 5 bits)
    with pytest.raises(csic.CsicIOError):
        csic.write_container_coded(out, cp, r, sizes, coding="rice", maps=mbuf, rows=True)
    with pytest.raises(csic.IllegalArgumentException):
        csic.write_container_coded(out, cp, rows, sizes, coding="rice", rows=True)            # no maps
    with pytest.raises(csic.IllegalArgumentException):
        csic.write_container_coded(out, cp, rows, sizes, coding="rice", maps=mbuf, gop=2, rows=True)
    sz = (C.c_uint64 * 2)(*sizes)
    assert L.csic_container_write_coded_rows(os.fsencode(out), C.byref(cp), p(rows), stride, sz, p(mbuf), ml.map_stride, 2, 0) == N.EINVAL_FORMAT
    assert L.csic_container_write_coded_rows(os.fsencode(out), C.byref(cp), p(rows), stride, sz, p(mbuf), ml.map_bytes - 1, 2, 3) == N.EINVAL_SIZE
    assert L.csic_container_write_coded_rows(os.fsencode(out), C.byref(cp), p(rows), sizes[0] - 1, sz, p(mbuf), ml.map_stride, 2, 3) == N.EINVAL_SIZE
    assert L.csic_container_write_coded_rows(os.fsencode(out), C.byref(cp), p(rows), stride, sz, None, ml.map_stride, 2, 3) == N.EINVAL_NULL
    assert not os.path.exists(out)


def test_inspect_names_the_layer_and_the_share_taken_from_above(capsys):
    assert csic.app.main(["inspect", "--input", FIXTURE_V8]) == 0
    text = capsys.readouterr().out
    assert "version 8" in text and "coding: rans, row prediction" in text
    assert "frame 0, Y: 1 of 4 groups (25.0%) predicted from the row above" in text
    assert "frame 0, Cb: 0 of 1 groups (0.0%) predicted from the row above" in text
