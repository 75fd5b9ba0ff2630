""".csic version 3 (group-coded frames; include/csic.h) without a GPU: files written by the library against files assembled independently
here (struct.pack + zlib.crc32 around the numpy encoder of tests/test_pack_host.py), read back, every refusal with its status, version 1
untouched, and a committed version-3 file that pins the format.  Every comparison is exact."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, load_png_rgb
from test_container import CANARY, CSQ, FIXTURE, _c_params, _fields, _frame_buffer, _layout, _random_sets
from test_pack_host import codes_of, lib_layout, plane_bytes, ref_encode

import csic_amd as csic

N = csic._native
FIXTURE_V3 = os.path.join(GOLDEN, "container_v3_16x16.csic")


def build_v3(fields, sizes, blob, coding=1, reserved=0, version=3, nframes=None):
    """A version-3 file from its parts, the CRC made right: only the defect a test puts into the parts remains."""
    body = struct.pack("<16i", *fields) + struct.pack("<II", coding, reserved) + b"".join(struct.pack("<Q", s) for s in sizes) + blob
    return b"CSIC" + struct.pack("<III", version, len(sizes) if nframes is None else nframes, zlib.crc32(body) & 0xFFFFFFFF) + body


def assemble_v3(fields, coded_frames):
    return build_v3(fields, [len(c) for c in coded_frames], b"".join(coded_frames))


def _stored(cp):
    q = N.CsicParams.from_buffer_copy(cp)
    q.out_format = N.FMT_PLANAR_BITS
    return q


def _make(oracle, rng, W, H, a, b, bits, f, op, rounding, avg, nframes, smooth=False):
    """-> (c_params, layout, frame buffers with a canary in the padding, the same zero-padded, the coded frames by numpy)"""
    cp = _c_params(W, H, a, b, bits, f, op, rounding, avg)
    lay = _layout(cp)
    dirty, clean, coded = [], [], []
    for k in range(nframes):
        argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        if smooth or k % 2:
            argb = (np.arange(W * H, dtype=np.uint32) // 3 * np.uint32(0x010101)) | np.uint32(0xFF000000)
        planes = codes_of(oracle, W, H, a, b, bits, f, op, rounding, avg, argb)
        pb = [plane_bytes(c, q) for c, q in zip(planes, bits)]
        dirty.append(_frame_buffer(lay, pb, CANARY))
        clean.append(_frame_buffer(lay, pb, 0))
        coded.append(ref_encode(planes, bits))
    return cp, lay, np.stack(dirty), np.stack(clean), coded


def test_raw_coding_is_the_version_1_writer(oracle, tmp_path):
    for k, (W, H, a, b, bits, f, op, rounding, avg, nframes, rng) in enumerate(_random_sets(12, 9110)):
        cp, lay, frames, _, _ = _make(oracle, rng, W, H, a, b, bits, f, op, rounding, avg, nframes)
        p1, p2, p3 = (str(tmp_path / f"{n}{k}.csic") for n in "abc")
        N.check(N.lib().csic_container_write(os.fsencode(p1), C.byref(cp), frames.ctypes.data_as(C.c_void_p), nframes))
        N.check(N.lib().csic_container_write_ex(os.fsencode(p2), C.byref(cp), frames.ctypes.data_as(C.c_void_p), nframes, N.CODING_RAW))
        csic.write_container(p3, cp, frames, coding="raw")
        data = open(p1, "rb").read()
        assert open(p2, "rb").read() == data and open(p3, "rb").read() == data and data[4:8] == struct.pack("<I", 1)
        assert csic.container_coded_sizes(p1).tolist() == [lay.payload_bytes] * nframes


def test_groups_coding_is_byte_identical_to_the_independent_assembly(oracle, tmp_path):
    seen = set()
    for k, (W, H, a, b, bits, f, op, rounding, avg, nframes, rng) in enumerate(_random_sets(36, 9120)):
        cp, lay, frames, clean, coded = _make(oracle, rng, W, H, a, b, bits, f, op, rounding, avg, nframes)
        tag = (W, H, a, b, bits, f, op, rounding, avg, nframes)
        want = assemble_v3(_fields(_stored(cp)), coded)
        path = str(tmp_path / f"g{k}.csic")
        csic.write_container(path, cp, frames, coding="groups")
        got = open(path, "rb").read()
        assert got == want, tag
        assert len(got) == 88 + 8 * nframes + sum(len(c) for c in coded), tag
        # from frames that are packed already: the same file (rows of a common stride, then a list)
        stride = lib_layout(cp).bound_bytes
        rows = np.full((nframes, stride), CANARY, dtype=np.uint8)
        for i, c in enumerate(coded):
            rows[i, :len(c)] = np.frombuffer(c, dtype=np.uint8)
        csic.write_container_coded(path + ".coded", cp, rows, [len(c) for c in coded])
        assert open(path + ".coded", "rb").read() == want, tag
        csic.write_container_coded(path + ".list", cp, [np.frombuffer(c, dtype=np.uint8) for c in coded], [len(c) for c in coded])
        assert open(path + ".list", "rb").read() == want, tag
        # read side
        info = csic.container_info(path)
        assert (info.version, info.nframes, info.payload_bytes, info.file_bytes) == (3, nframes, lay.payload_bytes, len(got)), tag
        assert _fields(info.params) == _fields(_stored(cp)), tag
        assert csic.container_coded_sizes(path).tolist() == [len(c) for c in coded], tag
        rp, rn, rframes = csic.read_container(path)
        assert rn == nframes and _fields(rp) == _fields(_stored(cp)) and np.array_equal(rframes, clean), tag
        dirty = np.full(nframes * lay.frame_bytes, 0x5A, dtype=np.uint8)       # every byte outside the payload ranges is zeroed
        N.check(N.lib().csic_container_read(os.fsencode(path), dirty.ctypes.data_as(C.c_void_p), dirty.size))
        assert np.array_equal(dirty.reshape(nframes, -1), clean), tag
        seen.add(nframes)
    assert seen == {1, 3}


@pytest.fixture()
def good(oracle, tmp_path):
    """A valid two-frame version-3 file: (path, bytes, c_params, layout, pack layout, the coded frames)."""
    rng = np.random.default_rng(9130)
    W, H, bits = 45, 7, (5, 4, 3)
    cp, lay, frames, _, coded = _make(oracle, rng, W, H, 4, 4, bits, 1, CSQ, 0, False, 2)
    path = str(tmp_path / "good.csic")
    csic.write_container(path, cp, frames, coding="groups")
    data = open(path, "rb").read()
    assert data == assemble_v3(_fields(_stored(cp)), coded)
    return path, data, cp, lay, lib_layout(cp), coded


def _read_status(path, nbytes):
    buf = np.full(max(nbytes, 1), 0x5A, dtype=np.uint8)
    st = N.lib().csic_container_read(os.fsencode(path), buf.ctypes.data_as(C.c_void_p), nbytes)
    return st, buf


DEFECTS = ["coding0", "coding2", "reserved", "size_below_fixed", "size_above_bound", "size_not_dwords", "longer", "truncated", "table_cut",
           "crc", "nibble", "pad_bit", "frame_sizes_swapped", "version2", "v3_header_v1_body"]


@pytest.mark.parametrize("defect", DEFECTS)
def test_read_refuses_a_damaged_file(good, tmp_path, defect):
    path, data, cp, lay, pl, coded = good
    fields = _fields(_stored(cp))
    sizes, blob = [len(c) for c in coded], b"".join(coded)
    top = pl.fixed_bytes + 4 * sum(g * q for g, q in zip(pl.groups, (5, 4, 3)))
    v1 = str(tmp_path / "v1.csic")
    csic.write_container(v1, cp, np.zeros((2, lay.frame_bytes), dtype=np.uint8))
    v1data = open(v1, "rb").read()

    def nibble():
        c = bytearray(coded[0])
        c[pl.widths_offset[1]] = (c[pl.widths_offset[1]] & 0xF0) | 5          # Cb has 4 bits per code
        return build_v3(fields, sizes, bytes(c) + coded[1])

    def pad_bit():
        c = bytearray(coded[1])
        c[pl.widths_offset[2] + 7] |= 0x80                                     # 10 groups: nibble 15 is padding
        return build_v3(fields, sizes, coded[0] + bytes(c))
    assert sizes[0] != sizes[1]
    bad = {
        "coding0": lambda: build_v3(fields, sizes, blob, coding=0),
        "coding2": lambda: build_v3(fields, sizes, blob, coding=2),
        "reserved": lambda: build_v3(fields, sizes, blob, reserved=1),
        "size_below_fixed": lambda: build_v3(fields, [pl.fixed_bytes - 4, sizes[1]], blob[:pl.fixed_bytes - 4] + coded[1]),
        "size_above_bound": lambda: build_v3(fields, [top + 4, sizes[1]], coded[0] + bytes(top + 4 - sizes[0]) + coded[1]),
        "size_not_dwords": lambda: build_v3(fields, [sizes[0] + 2, sizes[1]], coded[0] + b"\0\0" + coded[1]),
        "longer": lambda: build_v3(fields, sizes, blob + b"\0\0\0\0"),
        "truncated": lambda: build_v3(fields, sizes, blob[:-4]),
        "table_cut": lambda: data[:92],
        "crc": lambda: data[:-3] + bytes([data[-3] ^ 0x10]) + data[-2:],
        "nibble": nibble,
        "pad_bit": pad_bit,
        "frame_sizes_swapped": lambda: build_v3(fields, sizes[::-1], blob),        # the right total, the wrong cut
        "version2": lambda: build_v3(fields, sizes, blob, version=2),
        "v3_header_v1_body": lambda: v1data[:4] + struct.pack("<I", 3) + v1data[8:],
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
    if defect in ("crc", "nibble", "pad_bit", "frame_sizes_swapped"):           # the CRC and the frames are csic_container_read's to check
        assert info_st == N.OK and sizes_st == N.OK
    else:
        assert info_st == N.EFORMAT and sizes_st == N.EFORMAT


def test_write_and_size_refusals(good, tmp_path):
    path, data, cp, lay, pl, coded = good
    L = N.lib()
    st, buf = _read_status(path, 2 * lay.frame_bytes)
    assert st == N.OK
    for wrong in (2 * lay.frame_bytes - 1, lay.frame_bytes, 0):
        assert _read_status(path, wrong)[0] == N.EINVAL_SIZE
    frames = np.zeros((2, lay.frame_bytes), dtype=np.uint8)
    pf = frames.ctypes.data_as(C.c_void_p)
    out = os.fsencode(str(tmp_path / "w.csic"))
    assert L.csic_container_write_ex(None, C.byref(cp), pf, 2, 1) == N.EINVAL_NULL
    assert L.csic_container_write_ex(out, None, pf, 2, 1) == N.EINVAL_NULL
    assert L.csic_container_write_ex(out, C.byref(cp), None, 2, 1) == N.EINVAL_NULL
    assert L.csic_container_write_ex(out, C.byref(cp), pf, 2, 2) == N.EINVAL_FORMAT
    assert L.csic_container_write_ex(out, C.byref(cp), pf, 2, -1) == N.EINVAL_FORMAT
    for nf in (0, -1, 65536):
        assert L.csic_container_write_ex(out, C.byref(cp), pf, nf, 1) == N.EINVAL_SIZE
    bad = _c_params(45, 7, 3, 3, (5, 4, 3), 1, CSQ)
    assert L.csic_container_write_ex(out, C.byref(bad), pf, 1, 1) == N.EINVAL_CHROMA_A
    assert L.csic_container_write_ex(os.fsencode(str(tmp_path / "no_such_dir" / "w.csic")), C.byref(cp), pf, 2, 1) == N.EIO
    with pytest.raises(csic.IllegalArgumentException):
        csic.write_container(str(tmp_path / "w.csic"), cp, frames, coding="zip")
    # write_coded: NULLs, a size beyond the stride, and every frame validated before anything is written
    stride = pl.bound_bytes
    rows = np.zeros((2, stride), dtype=np.uint8)
    for i, c in enumerate(coded):
        rows[i, :len(c)] = np.frombuffer(c, dtype=np.uint8)
    sizes = (C.c_uint64 * 2)(*[len(c) for c in coded])
    pr = rows.ctypes.data_as(C.c_void_p)
    assert L.csic_container_write_coded(None, C.byref(cp), pr, stride, sizes, 2) == N.EINVAL_NULL
    assert L.csic_container_write_coded(out, None, pr, stride, sizes, 2) == N.EINVAL_NULL
    assert L.csic_container_write_coded(out, C.byref(cp), None, stride, sizes, 2) == N.EINVAL_NULL
    assert L.csic_container_write_coded(out, C.byref(cp), pr, stride, None, 2) == N.EINVAL_NULL
    assert L.csic_container_write_coded(out, C.byref(cp), pr, stride, sizes, 0) == N.EINVAL_SIZE
    assert L.csic_container_write_coded(out, C.byref(cp), pr, len(coded[0]) - 4, sizes, 2) == N.EINVAL_SIZE
    for off in (+4, -4):
        wrong = (C.c_uint64 * 2)(len(coded[0]), len(coded[1]) + off)
        assert L.csic_container_write_coded(out, C.byref(cp), pr, stride, wrong, 2) == N.EFORMAT
    rows[1, pl.widths_offset[0]] |= 0x0F
    assert L.csic_container_write_coded(out, C.byref(cp), pr, stride, sizes, 2) == N.EFORMAT
    assert not os.path.exists(out)
    # coded_sizes: NULLs, the wrong count
    assert L.csic_container_coded_sizes(None, sizes, 2) == N.EINVAL_NULL
    assert L.csic_container_coded_sizes(os.fsencode(path), None, 2) == N.EINVAL_NULL
    assert L.csic_container_coded_sizes(os.fsencode(path), sizes, 1) == N.EINVAL_SIZE
    assert L.csic_container_coded_sizes(os.fsencode(str(tmp_path / "missing.csic")), sizes, 2) == N.EIO


def test_committed_files_of_both_versions(oracle, tmp_path):
    """tests/golden/container_v3_16x16.csic holds what container_v1_16x16.csic holds (in16.png at 4:2:0, 6/5/5, factor 1), group-coded:
    pinned byte for byte against the numpy encoder, read to the same frames as version 1, and written again to the same bytes."""
    rgb = load_png_rgb(os.path.join(GOLDEN, "inputs", "in16.png"))
    argb = oracle.rgb_to_argb(rgb).reshape(-1)
    bits = (6, 5, 5)
    cp = _c_params(16, 16, 2, 0, bits, 1, CSQ)
    planes = codes_of(oracle, 16, 16, 2, 0, bits, 1, CSQ, 0, False, argb)
    want = assemble_v3(_fields(cp), [ref_encode(planes, bits)])
    data = open(FIXTURE_V3, "rb").read()
    assert data == want
    assert data[:12] == b"CSIC" + struct.pack("<II", 3, 1) and data[80:88] == struct.pack("<II", 1, 0)
    assert struct.unpack("<Q", data[88:96])[0] == len(data) - 96
    p1, n1, f1 = csic.read_container(FIXTURE)
    p3, n3, f3 = csic.read_container(FIXTURE_V3)
    assert n1 == n3 == 1 and _fields(p1) == _fields(p3) and np.array_equal(f1, f3)
    i1, i3 = csic.container_info(FIXTURE), csic.container_info(FIXTURE_V3)
    assert (i1.version, i3.version) == (1, 3) and i1.payload_bytes == i3.payload_bytes == 272 and i3.file_bytes == len(data)
    assert csic.container_coded_sizes(FIXTURE).tolist() == [272] and csic.container_coded_sizes(FIXTURE_V3).tolist() == [len(data) - 96]
    csic.write_container(str(tmp_path / "again.csic"), p3, f3, coding="groups")
    assert open(tmp_path / "again.csic", "rb").read() == data
