""".csic version 7 (everything that is rANS-coded: frames that stand alone, sequences through the temporal layer and through the
motion-compensated layer; include/csic.h) without a GPU: files written by the library against files assembled independently with
struct.pack + zlib.crc32 from the numpy statements of tests/delta_ref.py, tests/mc_ref.py and tests/test_rans_host.py; the read side;
the committed fixtures; every field's defect refused; the write refusals; `inspect`."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from delta_ref import frame_buffers, map_buffers, ref_map_layout
from mc_ref import ref_mc_layout
from test_container import CANARY, CSQ, FIXTURE, _c_params, _fields, _layout, _random_sets
from test_container_v3 import FIXTURE_V3, _read_status, _stored
from test_container_v5 import FIXTURE_V5, _fixture_frames, _sequence, build_v5
from test_container_v5 import ref_records as delta_records
from test_container_v6 import _pan, _widths
from test_container_v6 import ref_records as mc_records
from test_rans_host import rans_layout, ref_encode_rans
from test_rice_host import ref_encode_rice

import csic_amd as csic

N = csic._native
GOLDEN = os.path.dirname(FIXTURE)
FIXTURE_V7 = os.path.join(GOLDEN, "container_v7_16x16.csic")
FIXTURE_V7_SEQ = os.path.join(GOLDEN, "container_v7_seq_16x16.csic")
RANS = N.CODING_RANS


def build_v7(fields, R, gop, records, coding=RANS, **kw):
    """A version-7 file from its parts: version 6's layout, the word at 80 is 5 | (R + 1) << 8 (R = -1: no motion layer), then the gop
    (0: every frame stands alone)."""
    return build_v5(fields, coding | (R + 1) << 8, gop, records, version=kw.pop("version", 7), **kw)


def test_three_layers_are_byte_identical_to_the_independent_assembly(oracle, tmp_path):
    seen = set()
    for i, (W, H, a, b, bits, f, op, rounding, avg, _, rng) in enumerate(_random_sets(18, 23800)):
        nframes = 1 + i % 5
        kind = ("alone", "delta", "mc")[i % 3]
        gop = 0 if kind == "alone" else (1, 2, 3, nframes + 1)[i // 3 % 4]
        R = (2, 0, 7)[i // 3 % 3] if kind == "mc" else -1
        cp = _c_params(W, H, a, b, bits, f, op, rounding, avg)
        lay, tag = _layout(cp), (W, H, a, b, bits, f, op, rounding, avg, nframes, kind, gop, R)
        if kind == "mc":
            frames = _pan(oracle, rng, W, H, a, b, bits, f, op, rounding, avg, nframes)
            records, coded, maps, _ = mc_records(frames, bits, _widths(lay), gop, R, ref_encode_rans)
            ms = ref_mc_layout([c.size for c in frames[0]])[4]
        else:
            frames = _sequence(oracle, rng, W, H, a, b, bits, f, op, rounding, avg, nframes)
            if kind == "delta":
                records, coded, maps, _ = delta_records(frames, bits, gop, ref_encode_rans)
                ms = ref_map_layout([c.size for c in frames[0]])[3]
            else:
                records = coded = [ref_encode_rans(fr, bits) for fr in frames]
        want = build_v7(_fields(_stored(cp)), R, gop, records)
        src, clean = frame_buffers(lay, frames, bits, CANARY), frame_buffers(lay, frames, bits, 0)
        path = str(tmp_path / f"s{i}.csic")
        layer = {} if kind == "alone" else {"gop": gop} if kind == "delta" else {"gop": gop, "motion": R}
        csic.write_container(path, cp, src, coding="rans", **layer)
        got = open(path, "rb").read()
        assert got == want, tag
        assert got[4:8] == struct.pack("<I", 7) and got[80:88] == struct.pack("<II", RANS | (R + 1) << 8, gop), tag
        # from coded frames (and maps) as the device leaves them: rows of a stride, canaries behind the bytes that count
        rows = np.full((nframes, rans_layout(cp).bound_bytes), CANARY, dtype=np.uint8)
        for k, c in enumerate(coded):
            rows[k, :len(c)] = np.frombuffer(c, dtype=np.uint8)
        if kind != "alone":
            layer["maps"] = map_buffers(maps, ms, CANARY)
        csic.write_container_coded(path + ".coded", cp, rows, [len(c) for c in coded], coding="rans", **layer)
        assert open(path + ".coded", "rb").read() == want, tag
        # read side
        info = csic.container_info(path)
        assert (info.version, info.nframes, info.payload_bytes, info.file_bytes, info.gop, info.motion, info.coding) == \
            (7, nframes, lay.payload_bytes, len(got), max(gop, 1), R, RANS), tag
        assert _fields(info.params) == _fields(_stored(cp)), tag
        assert csic.container_coded_sizes(path).tolist() == [len(r) for r in records], tag
        if kind == "alone":
            assert csic.container_inter_groups(path).tolist() == [[0, 0, 0]] * nframes, tag
        rp, rn, rframes = csic.read_container(path)
        assert rn == nframes and _fields(rp) == _fields(_stored(cp)) and np.array_equal(rframes, clean), tag
        dirty = np.full(nframes * lay.frame_bytes, 0x5A, dtype=np.uint8)       # every byte outside the payload ranges is zeroed
        N.check(N.lib().csic_container_read(os.fsencode(path), dirty.ctypes.data_as(C.c_void_p), dirty.size))
        assert np.array_equal(dirty.reshape(nframes, -1), clean), tag
        seen.add(kind)
    assert seen == {"alone", "delta", "mc"}


def test_committed_version_7_files(oracle, tmp_path):
    """tests/golden/container_v7_16x16.csic pins the format for a frame that stands alone -- the frame of the version-1 and version-3
    fixtures --, container_v7_seq_16x16.csic for a sequence: the three frames of the version-5 fixture at gop 2, range 1."""
    bits, frames = _fixture_frames(oracle)
    cp = _c_params(16, 16, 2, 0, bits, 1, CSQ)
    coded = ref_encode_rans(frames[0], bits)
    data = open(FIXTURE_V7, "rb").read()
    assert data == build_v7(_fields(cp), -1, 0, [coded]) and len(data) < 1000
    assert data[:12] == b"CSIC" + struct.pack("<II", 7, 1) and data[80:88] == struct.pack("<II", 5, 0)
    assert struct.unpack("<Q", data[88:96]) == (len(coded),) and len(data) == 96 + len(coded)
    p7, n7, f7 = csic.read_container(FIXTURE_V7)
    assert n7 == 1 and _fields(p7) == _fields(cp) and np.array_equal(f7[0], csic.read_container(FIXTURE)[2][0])
    info = csic.container_info(FIXTURE_V7)
    assert (info.version, info.nframes, info.gop, info.motion, info.coding, info.file_bytes) == (7, 1, 1, -1, RANS, len(data))
    csic.write_container(str(tmp_path / "again.csic"), p7, f7, coding="rans")
    assert open(tmp_path / "again.csic", "rb").read() == data
    # the sequence
    records, _, maps, _ = mc_records(frames, bits, [16, 8, 8], 2, 1, ref_encode_rans)
    seq = open(FIXTURE_V7_SEQ, "rb").read()
    assert seq == build_v7(_fields(cp), 1, 2, records) and len(seq) < 4000
    assert seq[80:88] == struct.pack("<II", 5 | 2 << 8, 2) and records[1][:len(maps[1])] == maps[1]
    ps, ns, fs = csic.read_container(FIXTURE_V7_SEQ)
    assert ns == 3 and np.array_equal(fs, csic.read_container(FIXTURE_V5)[2])
    info = csic.container_info(FIXTURE_V7_SEQ)
    assert (info.version, info.nframes, info.gop, info.motion, info.coding) == (7, 3, 2, 1, RANS)
    csic.write_container(str(tmp_path / "again_seq.csic"), ps, fs, coding="rans", gop=2, motion=1)
    assert open(tmp_path / "again_seq.csic", "rb").read() == seq


def test_earlier_versions_read_and_write_as_before(tmp_path):
    for path, version, gop in ((FIXTURE, 1, 1), (FIXTURE_V3, 3, 1), (FIXTURE_V5, 5, 2)):
        info = csic.container_info(path)
        assert (info.version, info.gop, info.motion) == (version, gop, -1)
    cp, _, frames = csic.read_container(FIXTURE)
    for name, fixture in (("raw", FIXTURE), ("groups", FIXTURE_V3)):
        csic.write_container(str(tmp_path / "w.csic"), cp, frames, coding=name)
        assert open(tmp_path / "w.csic", "rb").read() == open(fixture, "rb").read()
    p5, _, f5 = csic.read_container(FIXTURE_V5)
    csic.write_container(str(tmp_path / "w5.csic"), p5, f5, coding="rice", gop=2)
    assert open(tmp_path / "w5.csic", "rb").read() == open(FIXTURE_V5, "rb").read()
    csic.write_container(str(tmp_path / "w6.csic"), p5, f5, coding="rice", gop=2, motion=1)
    assert csic.container_info(str(tmp_path / "w6.csic")).version == 6


@pytest.fixture()
def good(oracle, tmp_path):
    """A valid four-frame version-7 file at gop 3 and range 2: (path, bytes, c_params, layout, records, coded frames, maps), and the
    same frames standing alone."""
    rng = np.random.default_rng(23900)
    W, H, bits = 45, 7, (5, 4, 3)
    cp = _c_params(W, H, 4, 4, bits, 1, CSQ)
    frames = _pan(oracle, rng, W, H, 4, 4, bits, 1, CSQ, 0, False, 4)
    records, coded, maps, _ = mc_records(frames, bits, [W] * 3, 3, 2, ref_encode_rans)
    path = str(tmp_path / "good.csic")
    csic.write_container(path, cp, frame_buffers(_layout(cp), frames, bits, 0), coding="rans", gop=3, motion=2)
    data = open(path, "rb").read()
    assert data == build_v7(_fields(_stored(cp)), 2, 3, records)
    alone = [ref_encode_rans(fr, bits) for fr in frames]
    rice = mc_records(frames, bits, [W] * 3, 3, 2, ref_encode_rice)[0]
    return path, data, cp, _layout(cp), records, coded, maps, alone, rice


DEFECTS = ["coding1", "coding3", "coding4", "coding0", "v3_coding5", "v4_coding5", "v5_coding5", "v6_coding5", "gop0_with_maps", "range_without_gop",
           "motion9", "high_bit", "gop65536", "gop_other", "alone_with_gop", "size_above_bound", "size_not_dwords", "longer", "truncated", "table_cut",
           "crc", "coded_table", "coded_state", "map_table", "frame_sizes_swapped", "version8", "rice_body"]


@pytest.mark.parametrize("defect", DEFECTS)
def test_read_refuses_a_damaged_file(good, tmp_path, defect):
    path, data, cp, lay, records, coded, maps, alone, rice = good
    fields = _fields(_stored(cp))
    rl, ml = rans_layout(cp), csic.mc_layout(cp)
    mb = ml.map_bytes
    top = ml.map_bytes + rl.fixed_bytes + 4 * sum((g * 31 * q + 31) // 32 for g, q in zip(rl.groups, (5, 4, 3)))
    sizes = [len(r) for r in records]
    assert st_ok(path, lay) and sizes[1] != sizes[2] and list(rl.blocks) == [1, 1, 1]

    def patched(k, at, fn):
        r = [bytearray(x) for x in records]
        r[k][at] = fn(r[k][at])
        return build_v7(fields, 2, 3, [bytes(x) for x in r])
    bad = {
        "coding1": lambda: build_v7(fields, 2, 3, records, coding=1),
        "coding3": lambda: build_v7(fields, 2, 3, rice, coding=3),                # a whole version-6 body under the new version
        "coding4": lambda: build_v7(fields, 2, 3, records, coding=4),
        "coding0": lambda: build_v7(fields, 2, 3, records, coding=0),
        "v3_coding5": lambda: build_v7(fields, -1, 0, alone, version=3),
        "v4_coding5": lambda: build_v7(fields, -1, 0, alone, version=4),
        "v5_coding5": lambda: build_v7(fields, -1, 3, records, version=5),
        "v6_coding5": lambda: build_v7(fields, 2, 3, records, version=6),
        "gop0_with_maps": lambda: build_v7(fields, -1, 0, records),               # frames that stand alone have no maps in front
        "range_without_gop": lambda: build_v7(fields, 2, 0, alone),
        "motion9": lambda: build_v7(fields, 9, 3, records),
        "high_bit": lambda: build_v5(fields, 5 | 3 << 8 | 1 << 16, 3, records, version=7),
        "gop65536": lambda: build_v7(fields, 2, 65536, records),
        "gop_other": lambda: build_v7(fields, 2, 2, records),                     # frame 2 becomes a key frame whose record begins with a map
        "alone_with_gop": lambda: build_v7(fields, 2, 3, alone),                  # delta records without their maps
        "size_above_bound": lambda: build_v7(fields, 2, 3, [records[0], records[1] + bytes(top + 4 - sizes[1])] + records[2:]),
        "size_not_dwords": lambda: build_v7(fields, 2, 3, [records[0], records[1] + b"\0\0"] + records[2:]),
        "longer": lambda: build_v7(fields, 2, 3, records + [b"\0\0\0\0"], sizes=sizes),
        "truncated": lambda: build_v7(fields, 2, 3, records[:3] + [records[3][:-4]], sizes=sizes),
        "table_cut": lambda: data[:100],
        "crc": lambda: data[:-3] + bytes([data[-3] ^ 0x10]) + data[-2:],
        "coded_table": lambda: patched(0, rl.tables_offset[1], lambda v: v ^ 1),  # the Cb table no longer sums to M
        "coded_state": lambda: patched(1, mb + rl.payload_offset + 2, lambda v: v ^ 0x40),
        "map_table": lambda: patched(1, 64, lambda v: 16),                        # T of the Cb table of the motion map
        "frame_sizes_swapped": lambda: build_v7(fields, 2, 3, records, sizes=[sizes[0], sizes[2], sizes[1], sizes[3]]),
        "version8": lambda: build_v7(fields, 2, 3, records, version=8),
        "rice_body": lambda: build_v7(fields, 2, 3, rice),                        # coding 5 in the word, Rice-coded frames behind it
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
    gop_st = N.lib().csic_container_gop(os.fsencode(p), C.byref(C.c_int32()))
    motion_st = N.lib().csic_container_motion(os.fsencode(p), C.byref(C.c_int32()))
    assert motion_st == gop_st == info_st
    if defect in ("coding1", "coding3", "coding4", "coding0", "v3_coding5", "v4_coding5", "v5_coding5", "v6_coding5", "range_without_gop", "motion9",
                  "high_bit", "gop65536", "size_above_bound", "size_not_dwords", "longer", "truncated", "table_cut", "version8"):
        assert info_st == N.EFORMAT                                             # the header alone says so
    elif defect in ("crc", "coded_table", "coded_state", "map_table", "frame_sizes_swapped"):
        assert info_st == N.OK                                                  # the CRC, the coded frames and the maps are csic_container_read's to check


def st_ok(path, lay):
    return _read_status(path, 4 * lay.frame_bytes)[0] == N.OK


def test_write_refusals(good, tmp_path):
    path, data, cp, lay, records, coded, maps, alone, rice = good
    L = N.lib()
    _, _, frames = csic.read_container(path)
    out = str(tmp_path / "x.csic")
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for coding in (2, 4, 6):                                                     # ids 2 and 4 were never written
        assert L.csic_container_write_ex(os.fsencode(out), C.byref(cp), p(frames), 4, coding) == N.EINVAL_FORMAT
        assert L.csic_container_write_seq(os.fsencode(out), C.byref(cp), p(frames), 4, coding, 3) == N.EINVAL_FORMAT
        assert L.csic_container_write_seq_ex(os.fsencode(out), C.byref(cp), p(frames), 4, coding, 3, 2) == N.EINVAL_FORMAT
    for R in (-1, 8):
        assert L.csic_container_write_seq_ex(os.fsencode(out), C.byref(cp), p(frames), 4, RANS, 3, R) == N.EINVAL_SIZE
    assert L.csic_container_write_seq(os.fsencode(out), C.byref(cp), p(frames), 4, RANS, 0) == N.EINVAL_SIZE
    assert L.csic_container_write_ex(None, C.byref(cp), p(frames), 4, RANS) == N.EINVAL_NULL
    assert not os.path.exists(out)
    with pytest.raises(csic.IllegalArgumentException):
        csic.write_container(out, cp, frames, coding="rans", motion=2)           # motion needs a gop
    with pytest.raises(csic.IllegalArgumentException):
        csic.write_container(out, cp, frames, coding="ans")
    # coded frames that csic_rans_unpack_host would refuse are refused before anything is written
    stride = rans_layout(cp).bound_bytes
    rows = np.zeros((4, stride), dtype=np.uint8)
    for k, c in enumerate(alone):
        rows[k, :len(c)] = np.frombuffer(c, dtype=np.uint8)
    sizes = [len(c) for c in alone]
    csic.write_container_coded(out, cp, rows, sizes, coding="rans")
    assert open(out, "rb").read() == build_v7(_fields(_stored(cp)), -1, 0, alone)
    os.remove(out)
    rl = rans_layout(cp)                                                         # a table's sum, an anchors padding bit (10 groups of 5 bits), a flag on dir[NB]
    for frame, at in ((0, 0), (3, rl.anchors_offset[0] + 7), (2, rl.directory_offset + 4 * 3 + 3)):
        r = rows.copy()
        r[frame, at] ^= 0x80
        with pytest.raises(csic.CsicIOError):
            csic.write_container_coded(out, cp, r, sizes, coding="rans")
        assert not os.path.exists(out)
    with pytest.raises(csic.CsicIOError):                                        # Rice-coded frames handed in as rANS-coded ones
        csic.write_container_coded(out, cp, rows, sizes, coding="rice")
    sz = (C.c_uint64 * 4)(*sizes)
    assert L.csic_container_write_coded_ex(os.fsencode(out), C.byref(cp), p(rows), stride, sz, 4, 4) == N.EINVAL_FORMAT
    assert L.csic_container_write_coded_ex(os.fsencode(out), C.byref(cp), p(rows), sizes[0] - 1, sz, 4, RANS) == N.EINVAL_SIZE
    assert not os.path.exists(out)


def test_inspect_prints_the_coding_the_stored_bytes_and_the_raw_blocks(capsys):
    assert csic.app.main(["inspect", "--input", FIXTURE_V7]) == 0
    text = capsys.readouterr().out
    size = int(csic.container_coded_sizes(FIXTURE_V7)[0])
    assert "version 7" in text and "coding: rans" in text and f"frame 0: stored in {size} bytes" in text
    for name in ("Y", "Cb", "Cr"):
        assert f"frame 0, {name}: " in text and "of 1 blocks raw" in text
    assert csic.app.main(["inspect", "--input", FIXTURE_V7_SEQ]) == 0
    text = capsys.readouterr().out
    assert "coding: rans, motion-compensated delta with gop 2, range 1" in text and "frame 1 (delta): stored in" in text
