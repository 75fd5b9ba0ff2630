""".csic version 4 (Rice-coded frames; include/csic.h) without a GPU: files written by the library against files assembled independently
here (struct.pack + zlib.crc32 around the numpy encoder of tests/test_rice_host.py), read back, the version-3 defect list on a version-4
file plus the version / coding mismatches, versions 1 and 3 untouched, and the CLI as far as it runs without a device."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from test_container import CANARY, CSQ, _c_params, _fields, _frame_buffer, _layout, _random_sets
from test_container_v3 import _read_status, _stored, assemble_v3, build_v3
from test_pack_host import codes_of, plane_bytes, ref_encode
from test_rice_host import ref_encode_rice, rice_layout

import csic_amd as csic

N = csic._native


def build_v4(fields, sizes, blob, coding=3, reserved=0, version=4, nframes=None):
    """Version 4 is version 3's layout with version = 4 and coding = 3."""
    return build_v3(fields, sizes, blob, coding=coding, reserved=reserved, version=version, nframes=nframes)


def _make(oracle, rng, W, H, a, b, bits, f, op, rounding, avg, nframes):
    """-> (c_params, layout, frame buffers with a canary in the padding, the same zero-padded, the frames Rice-coded and group-coded by numpy)"""
    cp = _c_params(W, H, a, b, bits, f, op, rounding, avg)
    lay = _layout(cp)
    dirty, clean, rice, groups = [], [], [], []
    for k in range(nframes):
        argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        if k % 2:
            argb = (np.arange(W * H, dtype=np.uint32) // 3 * np.uint32(0x010101)) | np.uint32(0xFF000000)
        planes = codes_of(oracle, W, H, a, b, bits, f, op, rounding, avg, argb)
        pb = [plane_bytes(c, q) for c, q in zip(planes, bits)]
        dirty.append(_frame_buffer(lay, pb, CANARY))
        clean.append(_frame_buffer(lay, pb, 0))
        rice.append(ref_encode_rice(planes, bits))
        groups.append(ref_encode(planes, bits))
    return cp, lay, np.stack(dirty), np.stack(clean), rice, groups


def test_rice_coding_is_byte_identical_to_the_independent_assembly(oracle, tmp_path):
    seen = set()
    for k, (W, H, a, b, bits, f, op, rounding, avg, nframes, rng) in enumerate(_random_sets(24, 11600)):
        cp, lay, frames, clean, coded, _ = _make(oracle, rng, W, H, a, b, bits, f, op, rounding, avg, nframes)
        tag = (W, H, a, b, bits, f, op, rounding, avg, nframes)
        want = build_v4(_fields(_stored(cp)), [len(c) for c in coded], b"".join(coded))
        path = str(tmp_path / f"r{k}.csic")
        csic.write_container(path, cp, frames, coding="rice")
        got = open(path, "rb").read()
        assert got == want, tag
        assert len(got) == 88 + 8 * nframes + sum(len(c) for c in coded) and got[4:8] == struct.pack("<I", 4) and got[80:88] == struct.pack("<II", 3, 0), tag
        N.check(N.lib().csic_container_write_ex(os.fsencode(path + ".ex"), C.byref(cp), frames.ctypes.data_as(C.c_void_p), nframes, N.CODING_RICE))
        assert open(path + ".ex", "rb").read() == want, tag
        # from frames that are packed already: the same file (rows of a common stride, then a list)
        stride = rice_layout(cp).bound_bytes
        rows = np.full((nframes, stride), CANARY, dtype=np.uint8)
        for i, c in enumerate(coded):
            rows[i, :len(c)] = np.frombuffer(c, dtype=np.uint8)
        csic.write_container_coded(path + ".coded", cp, rows, [len(c) for c in coded], coding="rice")
        assert open(path + ".coded", "rb").read() == want, tag
        csic.write_container_coded(path + ".list", cp, [np.frombuffer(c, dtype=np.uint8) for c in coded], [len(c) for c in coded], coding=N.CODING_RICE)
        assert open(path + ".list", "rb").read() == want, tag
        # read side
        info = csic.container_info(path)
        assert (info.version, info.nframes, info.payload_bytes, info.file_bytes) == (4, nframes, lay.payload_bytes, len(got)), tag
        assert _fields(info.params) == _fields(_stored(cp)), tag
        assert csic.container_coded_sizes(path).tolist() == [len(c) for c in coded], tag
        rp, rn, rframes = csic.read_container(path)
        assert rn == nframes and _fields(rp) == _fields(_stored(cp)) and np.array_equal(rframes, clean), tag
        dirty = np.full(nframes * lay.frame_bytes, 0x5A, dtype=np.uint8)       # every byte outside the payload ranges is zeroed
        N.check(N.lib().csic_container_read(os.fsencode(path), dirty.ctypes.data_as(C.c_void_p), dirty.size))
        assert np.array_equal(dirty.reshape(nframes, -1), clean), tag
        seen.add(nframes)
    assert seen == {1, 3}


def test_codings_0_and_1_write_what_they_wrote(oracle, tmp_path):
    """write_ex(..., 0) is the version-1 writer and write_ex(..., 1) the version-3 writer, byte for byte against the independent
    assemblies of tests/test_container.py and tests/test_container_v3.py; csic_container_write_coded keeps meaning the group coding."""
    from test_container import assemble
    for k, (W, H, a, b, bits, f, op, rounding, avg, nframes, rng) in enumerate(_random_sets(12, 11700)):
        cp, lay, frames, clean, _, groups = _make(oracle, rng, W, H, a, b, bits, f, op, rounding, avg, nframes)
        p0, p1, p2 = (str(tmp_path / f"{n}{k}.csic") for n in "abc")
        pf = frames.ctypes.data_as(C.c_void_p)
        N.check(N.lib().csic_container_write_ex(os.fsencode(p0), C.byref(cp), pf, nframes, N.CODING_RAW))
        N.check(N.lib().csic_container_write_ex(os.fsencode(p1), C.byref(cp), pf, nframes, N.CODING_GROUPS))
        payloads = [np.concatenate([fr[o:o + n] for o, n in ((lay.y_offset, lay.y_bytes), (lay.cb_offset, lay.cb_bytes), (lay.cr_offset, lay.cr_bytes))])
                    for fr in clean]
        assert open(p0, "rb").read() == assemble(_fields(_stored(cp)), payloads)
        want3 = assemble_v3(_fields(_stored(cp)), groups)
        assert open(p1, "rb").read() == want3
        csic.write_container_coded(p2, cp, [np.frombuffer(c, dtype=np.uint8) for c in groups], [len(c) for c in groups])
        assert open(p2, "rb").read() == want3


@pytest.fixture()
def good(oracle, tmp_path):
    """A valid two-frame version-4 file: (path, bytes, c_params, layout, rice layout, the coded frames, the same frames group-coded)."""
    rng = np.random.default_rng(11800)
    W, H, bits = 45, 7, (5, 4, 3)
    cp, lay, frames, _, coded, groups = _make(oracle, rng, W, H, 4, 4, bits, 1, CSQ, 0, False, 2)
    path = str(tmp_path / "good.csic")
    csic.write_container(path, cp, frames, coding="rice")
    data = open(path, "rb").read()
    assert data == build_v4(_fields(_stored(cp)), [len(c) for c in coded], b"".join(coded))
    return path, data, cp, lay, rice_layout(cp), coded, groups


DEFECTS = ["coding0", "coding1", "coding2", "v3_with_coding3", "v3_header_rice_body", "v4_header_groups_body", "reserved", "size_below_fixed",
           "size_above_bound", "size_not_dwords", "longer", "truncated", "table_cut", "crc", "nibble", "pad_bit", "directory", "terminator",
           "frame_sizes_swapped", "version2", "version5", "v4_header_v1_body"]


@pytest.mark.parametrize("defect", DEFECTS)
def test_read_refuses_a_damaged_file(good, tmp_path, defect):
    path, data, cp, lay, rl, coded, groups = good
    fields = _fields(_stored(cp))
    sizes, blob = [len(c) for c in coded], b"".join(coded)
    top = rl.fixed_bytes + 4 * sum(b * (248 * q + 1) for b, q in zip(rl.blocks, (5, 4, 3)))
    v1 = str(tmp_path / "v1.csic")
    csic.write_container(v1, cp, np.zeros((2, lay.frame_bytes), dtype=np.uint8))
    v1data = open(v1, "rb").read()

    def patched(k, at, fn):
        c = bytearray(coded[k])
        c[at] = fn(c[at])
        return build_v4(fields, sizes, bytes(c) + coded[1] if k == 0 else coded[0] + bytes(c))
    assert sizes[0] != sizes[1]
    bad = {
        "coding0": lambda: build_v4(fields, sizes, blob, coding=0),
        "coding1": lambda: build_v4(fields, sizes, blob, coding=1),                      # version 4 with the group coding's id
        "coding2": lambda: build_v4(fields, sizes, blob, coding=2),
        "v3_with_coding3": lambda: build_v4(fields, sizes, blob, version=3),              # version 3 with the Rice coding's id
        "v3_header_rice_body": lambda: build_v3(fields, sizes, blob),                     # 3 / 1 in front of Rice-coded frames
        "v4_header_groups_body": lambda: build_v4(fields, [len(g) for g in groups], b"".join(groups)),
        "reserved": lambda: build_v4(fields, sizes, blob, reserved=1),
        "size_below_fixed": lambda: build_v4(fields, [rl.fixed_bytes - 4, sizes[1]], blob[:rl.fixed_bytes - 4] + coded[1]),
        "size_above_bound": lambda: build_v4(fields, [top + 4, sizes[1]], coded[0] + bytes(top + 4 - sizes[0]) + coded[1]),
        "size_not_dwords": lambda: build_v4(fields, [sizes[0] + 2, sizes[1]], coded[0] + b"\0\0" + coded[1]),
        "longer": lambda: build_v4(fields, sizes, blob + b"\0\0\0\0"),
        "truncated": lambda: build_v4(fields, sizes, blob[:-4]),
        "table_cut": lambda: data[:92],
        "crc": lambda: data[:-3] + bytes([data[-3] ^ 0x10]) + data[-2:],
        "nibble": lambda: patched(0, rl.modes_offset[1], lambda v: (v & 0xF0) | 5),       # Cb has 4 bits per code
        "pad_bit": lambda: patched(1, rl.modes_offset[2] + 7, lambda v: v | 0x80),        # 10 groups: nibble 15 is padding
        "directory": lambda: patched(0, rl.directory_offset + 4, lambda v: v ^ 1),        # dir[1] off by one dword
        "terminator": lambda: patched(1, sizes[1] - 1, lambda v: v | 0x80),                # one more one bit at the end of the last U
        "frame_sizes_swapped": lambda: build_v4(fields, sizes[::-1], blob),               # the right total, the wrong cut
        "version2": lambda: build_v4(fields, sizes, blob, version=2),
        "version5": lambda: build_v4(fields, sizes, blob, version=5),
        "v4_header_v1_body": lambda: v1data[:4] + struct.pack("<I", 4) + v1data[8:],
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
    sizes_st = N.lib().csic_container_coded_sizes(os.fsencode(p), (C.c_uint64 * 2)(), 2)
    if defect in ("crc", "nibble", "pad_bit", "directory", "terminator", "frame_sizes_swapped"):    # the CRC and the frames are csic_container_read's to check
        assert info_st == N.OK and sizes_st == N.OK
    elif defect in ("v3_header_rice_body", "v4_header_groups_body"):           # a consistent header: the sizes may or may not fit the other coding
        assert info_st in (N.OK, N.EFORMAT) and sizes_st == info_st
    else:
        assert info_st == N.EFORMAT and sizes_st == N.EFORMAT


def test_write_and_size_refusals(good, tmp_path):
    path, data, cp, lay, rl, coded, groups = good
    L = N.lib()
    assert _read_status(path, 2 * lay.frame_bytes)[0] == N.OK
    for wrong in (2 * lay.frame_bytes - 1, lay.frame_bytes, 0):
        assert _read_status(path, wrong)[0] == N.EINVAL_SIZE
    frames = np.zeros((2, lay.frame_bytes), dtype=np.uint8)
    pf = frames.ctypes.data_as(C.c_void_p)
    out = os.fsencode(str(tmp_path / "w.csic"))
    assert L.csic_container_write_ex(None, C.byref(cp), pf, 2, 3) == N.EINVAL_NULL
    assert L.csic_container_write_ex(out, None, pf, 2, 3) == N.EINVAL_NULL
    assert L.csic_container_write_ex(out, C.byref(cp), None, 2, 3) == N.EINVAL_NULL
    assert L.csic_container_write_ex(out, C.byref(cp), pf, 2, 2) == N.EINVAL_FORMAT          # id 2 stays refused
    assert L.csic_container_write_ex(out, C.byref(cp), pf, 2, 4) == N.EINVAL_FORMAT
    for nf in (0, -1, 65536):
        assert L.csic_container_write_ex(out, C.byref(cp), pf, nf, 3) == N.EINVAL_SIZE
    assert L.csic_container_write_ex(os.fsencode(str(tmp_path / "no_such_dir" / "w.csic")), C.byref(cp), pf, 2, 3) == N.EIO
    with pytest.raises(csic.IllegalArgumentException) as ei:
        csic.write_container(str(tmp_path / "w.csic"), cp, frames, coding="zip")
    assert all(name in str(ei.value) for name in ("'raw'", "'groups'", "'rice'"))
    # write_coded_ex: NULLs, the coding, a size beyond the stride, and every frame validated before anything is written
    stride = rl.bound_bytes
    rows = np.zeros((2, stride), dtype=np.uint8)
    for i, c in enumerate(coded):
        rows[i, :len(c)] = np.frombuffer(c, dtype=np.uint8)
    sizes = (C.c_uint64 * 2)(*[len(c) for c in coded])
    pr = rows.ctypes.data_as(C.c_void_p)
    assert L.csic_container_write_coded_ex(None, C.byref(cp), pr, stride, sizes, 2, 3) == N.EINVAL_NULL
    assert L.csic_container_write_coded_ex(out, None, pr, stride, sizes, 2, 3) == N.EINVAL_NULL
    assert L.csic_container_write_coded_ex(out, C.byref(cp), None, stride, sizes, 2, 3) == N.EINVAL_NULL
    assert L.csic_container_write_coded_ex(out, C.byref(cp), pr, stride, None, 2, 3) == N.EINVAL_NULL
    for coding in (0, 2, 4, -1):
        assert L.csic_container_write_coded_ex(out, C.byref(cp), pr, stride, sizes, 2, coding) == N.EINVAL_FORMAT
    assert L.csic_container_write_coded_ex(out, C.byref(cp), pr, stride, sizes, 0, 3) == N.EINVAL_SIZE
    assert L.csic_container_write_coded_ex(out, C.byref(cp), pr, len(coded[0]) - 4, sizes, 2, 3) == N.EINVAL_SIZE
    assert L.csic_container_write_coded_ex(out, C.byref(cp), pr, stride, sizes, 2, 1) == N.EFORMAT       # Rice-coded frames are no group-coded frames
    assert L.csic_container_write_coded(out, C.byref(cp), pr, stride, sizes, 2) == N.EFORMAT
    for off in (+4, -4):
        wrong = (C.c_uint64 * 2)(len(coded[0]), len(coded[1]) + off)
        assert L.csic_container_write_coded_ex(out, C.byref(cp), pr, stride, wrong, 2, 3) == N.EFORMAT
    rows[1, rl.modes_offset[0]] = (rows[1, rl.modes_offset[0]] & 0xF0) | 0x0E
    assert L.csic_container_write_coded_ex(out, C.byref(cp), pr, stride, sizes, 2, 3) == N.EFORMAT
    assert not os.path.exists(out)
    assert L.csic_container_coded_sizes(os.fsencode(path), sizes, 1) == N.EINVAL_SIZE


def test_cli_reads_version_4_and_knows_the_coding(good, tmp_path, capsys):
    """inspect prints a version-4 file's header, coding and stored sizes without a device; compress knows --coding rice (it needs a
    device from there on: tests/test_gpu_rice.py runs compress and decompress end to end)."""
    path, data, cp, lay, rl, coded, _ = good
    assert csic.app.main(["inspect", "--input", path]) == 0
    text = capsys.readouterr().out
    assert "version 4" in text and "Frame coding: rice" in text
    for c in coded:
        assert f"stored in {len(c)} bytes" in text
    png = os.path.join(os.path.dirname(__file__), "golden", "inputs", "in16.png")
    assert csic.app.main(["compress", "--input", png, "--output", str(tmp_path / "x.csic"), "--coding", "zip"]) == 2
    assert "raw, groups or rice" in capsys.readouterr().out
    with pytest.raises(csic.IllegalArgumentException) as ei:
        csic.ImageCompressionApp.compressImage(png, str(tmp_path / "x.csic"), 2, 0, 6, 5, 5, 1, csic.ProcessingStep.ChromaSubsampling,
                                               csic.ProcessingStep.SpatialSampling, csic.ProcessingStep.ColorQuantization, coding="zip")
    assert "rice" in str(ei.value)
