""".csic files: CSIC_FMT_PLANAR_BITS frames on disk (csic_container_*; byte layout in include/csic.h), raw (version 1), group-coded
(version 3), Rice-coded (version 4), rANS-coded (version 7) or as a sequence through the temporal layer (versions 5, 6, 7), the host
codecs of the three codings (csic_pack_host / csic_unpack_host, csic_rice_*_host, csic_rans_*_host) and the host codec of the temporal layer
(csic_delta_host / csic_undelta_host) and of the row-prediction layer (csic_rows_host / csic_unrows_host; version 8).  Host only: nothing
here needs a GPU."""
from __future__ import annotations

import ctypes as C
import os
from typing import Tuple

import numpy as np

from . import _native as N


def container_info(path: str) -> N.CsicContainerInfo:
    """Header, parameters and length of a .csic file (csic_container_info_of; everything read_container checks but the CRC), and as
    plain attributes its `gop` (csic_container_gop) and the `coding` of its frames."""
    info = N.CsicContainerInfo()
    N.check(N.lib().csic_container_info_of(os.fsencode(path), C.byref(info)))
    gop = C.c_int32()
    N.check(N.lib().csic_container_gop(os.fsencode(path), C.byref(gop)))
    info.gop = gop.value                              # csic_container_gop: 1 below version 5 (every frame stands alone)
    info.coding = {1: N.CODING_RAW, 3: N.CODING_GROUPS, 4: N.CODING_RICE}.get(info.version)
    if info.coding is None:                           # versions 5 to 8 name their coding in the word behind the parameters (checked by the library)
        with open(path, "rb") as fh:
            fh.seek(80)
            info.coding = int.from_bytes(fh.read(4), "little") & 0xFF      # (version 6 keeps its range + 1 in bits 8.., version 8 its flag in bit 16)
    motion = C.c_int32()
    N.check(N.lib().csic_container_motion(os.fsencode(path), C.byref(motion)))
    info.motion = motion.value                        # csic_container_motion: the range of a version-6 file, -1 otherwise
    rows = C.c_int32()
    N.check(N.lib().csic_container_rows(os.fsencode(path), C.byref(rows)))
    info.rows = bool(rows.value)                      # csic_container_rows: version 8, every frame through the row-prediction layer
    return info


def _bits_params(c_params: N.CsicParams):
    """-> (the parameters a container stores, their PLANAR_BITS layout); raises what csic_validate refuses."""
    lay = N.CsicPlanarBitsLayout()
    q = N.CsicParams.from_buffer_copy(c_params)
    q.out_format = N.FMT_PLANAR_BITS
    N.check(N.lib().csic_validate(C.byref(q)))
    N.check(N.lib().csic_planar_bits_layout_of(C.byref(q), C.byref(lay)))
    return q, lay


def _coding(coding) -> int:
    if isinstance(coding, str):
        names = {"raw": N.CODING_RAW, "groups": N.CODING_GROUPS, "rice": N.CODING_RICE, "rans": N.CODING_RANS}
        if coding.lower() not in names:
            raise N.IllegalArgumentException(N.EINVAL_FORMAT, f"requirement failed: coding must be 'raw', 'groups', 'rice' or 'rans', got {coding!r}")
        return names[coding.lower()]
    return int(coding)


def pack_layout(c_params: N.CsicParams) -> N.CsicPackLayout:
    """csic_pack_layout_of: groups, section offsets, fixed_bytes and bound_bytes of a coded frame of these parameters."""
    lay = N.CsicPackLayout()
    N.check(N.lib().csic_pack_layout_of(C.byref(c_params), C.byref(lay)))
    return lay


def _pack_host(c_params: N.CsicParams, bits_frame, layout_of, pack) -> np.ndarray:
    """One PLANAR_BITS frame buffer -> its coded bytes through a coding's `layout_of` (pack_layout, rice_layout) and `*_pack_host`."""
    q, lay = _bits_params(c_params)
    a = np.ascontiguousarray(bits_frame).reshape(-1).view(np.uint8)
    if a.size != lay.frame_bytes:
        raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: a frame buffer of these parameters has {lay.frame_bytes} bytes, got {a.size}")
    coded = np.empty(layout_of(q).bound_bytes, dtype=np.uint8)
    n = C.c_uint64()
    N.check(pack(C.byref(q), a.ctypes.data_as(C.c_void_p), coded.ctypes.data_as(C.c_void_p), coded.size, C.byref(n)))
    return coded[:n.value].copy()


def _unpack_host(c_params: N.CsicParams, coded, out, unpack) -> np.ndarray:
    """Coded bytes -> a PLANAR_BITS frame buffer through a coding's `*_unpack_host`.  Empty input goes in as a one-byte buffer of
    length 0, so that the library refuses its size (CsicIOError) rather than a NULL pointer."""
    q, lay = _bits_params(c_params)
    a = np.ascontiguousarray(coded).reshape(-1).view(np.uint8)
    if out is None:
        out = np.zeros(lay.frame_bytes, dtype=np.uint8)
    elif out.dtype != np.uint8 or out.size != lay.frame_bytes or not out.flags.c_contiguous:
        raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: out must be a contiguous uint8 buffer of {lay.frame_bytes} bytes")
    src = a if a.size else np.zeros(1, dtype=np.uint8)
    N.check(unpack(C.byref(q), src.ctypes.data_as(C.c_void_p), a.size, out.ctypes.data_as(C.c_void_p)))
    return out


def pack_frame_host(c_params: N.CsicParams, bits_frame) -> np.ndarray:
    """csic_pack_host: one PLANAR_BITS frame buffer (frame_bytes) -> its coded bytes, a uint8 array of coded_bytes."""
    return _pack_host(c_params, bits_frame, pack_layout, N.lib().csic_pack_host)


def unpack_frame_host(c_params: N.CsicParams, coded, out=None) -> np.ndarray:
    """csic_unpack_host: coded bytes -> a PLANAR_BITS frame buffer.  `out` (uint8, frame_bytes) keeps its bytes outside the three
    payload ranges; without it the buffer is zero there.  Damaged input raises CsicIOError (CSIC_EFORMAT)."""
    return _unpack_host(c_params, coded, out, N.lib().csic_unpack_host)


def rice_layout(c_params: N.CsicParams) -> N.CsicRiceLayout:
    """csic_rice_layout_of: groups, blocks, section offsets, fixed_bytes and bound_bytes of a Rice-coded frame of these parameters."""
    lay = N.CsicRiceLayout()
    N.check(N.lib().csic_rice_layout_of(C.byref(c_params), C.byref(lay)))
    return lay


def rice_pack_host(c_params: N.CsicParams, bits_frame) -> np.ndarray:
    """csic_rice_pack_host: one PLANAR_BITS frame buffer (frame_bytes) -> its Rice-coded bytes, a uint8 array of coded_bytes."""
    return _pack_host(c_params, bits_frame, rice_layout, N.lib().csic_rice_pack_host)


def rice_unpack_host(c_params: N.CsicParams, coded, out=None) -> np.ndarray:
    """csic_rice_unpack_host: Rice-coded bytes -> a PLANAR_BITS frame buffer, as unpack_frame_host.  Damaged input raises CsicIOError."""
    return _unpack_host(c_params, coded, out, N.lib().csic_rice_unpack_host)


def rans_layout(c_params: N.CsicParams) -> N.CsicRansLayout:
    """csic_rans_layout_of: groups, blocks, section offsets, fixed_bytes and bound_bytes of a rANS-coded frame of these parameters."""
    lay = N.CsicRansLayout()
    N.check(N.lib().csic_rans_layout_of(C.byref(c_params), C.byref(lay)))
    return lay


def rans_pack_host(c_params: N.CsicParams, bits_frame) -> np.ndarray:
    """csic_rans_pack_host: one PLANAR_BITS frame buffer (frame_bytes) -> its rANS-coded bytes, a uint8 array of coded_bytes."""
    return _pack_host(c_params, bits_frame, rans_layout, N.lib().csic_rans_pack_host)


def rans_unpack_host(c_params: N.CsicParams, coded, out=None) -> np.ndarray:
    """csic_rans_unpack_host: rANS-coded bytes -> a PLANAR_BITS frame buffer, as unpack_frame_host.  Damaged input raises CsicIOError."""
    return _unpack_host(c_params, coded, out, N.lib().csic_rans_unpack_host)


def delta_layout(c_params: N.CsicParams) -> N.CsicDeltaLayout:
    """csic_delta_layout_of: groups, the sections' offsets, map_bytes and map_stride of a frame's map."""
    lay = N.CsicDeltaLayout()
    N.check(N.lib().csic_delta_layout_of(C.byref(c_params), C.byref(lay)))
    return lay


def _frames_2d(frames, frame_bytes: int) -> np.ndarray:
    if isinstance(frames, (list, tuple)):
        frames = np.stack([np.ascontiguousarray(f).reshape(-1).view(np.uint8) for f in frames])
    a = np.ascontiguousarray(frames).reshape(-1).view(np.uint8)
    if a.size == 0 or a.size % frame_bytes != 0:
        raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: frames must hold whole frame buffers of {frame_bytes} bytes, got {a.size}")
    return a.reshape(-1, frame_bytes)


def _temporal_forward(c_params: N.CsicParams, frames, out, layout_of, entry, *args):
    """Both layers' `*_delta_host`: `entry(params, frames, nframes, *args, diff, maps)` with the maps of `layout_of`."""
    q, lay = _bits_params(c_params)
    ml = layout_of(q)
    a = _frames_2d(frames, lay.frame_bytes)
    diff = np.zeros_like(a) if out is None else out
    maps = np.zeros((a.shape[0], ml.map_stride), dtype=np.uint8)
    N.check(entry(C.byref(q), a.ctypes.data_as(C.c_void_p), a.shape[0], *args, diff.ctypes.data_as(C.c_void_p), maps.ctypes.data_as(C.c_void_p)))
    return diff, maps


def _temporal_inverse(c_params: N.CsicParams, diff, maps, gop, out, layout_of, entry) -> np.ndarray:
    """Both layers' `*_undelta_host`: `entry(params, diff, maps, nframes, gop, frames)` with the maps of `layout_of`."""
    q, lay = _bits_params(c_params)
    ml = layout_of(q)
    d = _frames_2d(diff, lay.frame_bytes)
    m = np.ascontiguousarray(maps).view(np.uint8).reshape(d.shape[0], -1)
    if m.shape[1] != ml.map_stride:
        raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: maps must be (nframes, {ml.map_stride}), got {m.shape}")
    frames = np.zeros_like(d) if out is None else out
    N.check(entry(C.byref(q), d.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), d.shape[0], *([] if gop is None else [int(gop)]),
                  frames.ctypes.data_as(C.c_void_p)))
    return frames


def delta_host(c_params: N.CsicParams, frames, gop: int, out=None):
    """csic_delta_host: PLANAR_BITS frame buffers (nframes, frame_bytes) -> (diff, maps): the difference frames, an array of the same
    shape (zero outside the payload ranges, or `out` -- which may be `frames` itself, in place), and the maps, uint8 (nframes,
    map_stride) with map_bytes of each row written."""
    return _temporal_forward(c_params, frames, out, delta_layout, N.lib().csic_delta_host, int(gop))


def undelta_host(c_params: N.CsicParams, diff, maps, gop: int, out=None) -> np.ndarray:
    """csic_undelta_host: the inverse of delta_host.  The maps are untrusted: a set padding bit or a non-zero map of a key frame raises
    CsicIOError (CSIC_EFORMAT) and nothing is written."""
    return _temporal_inverse(c_params, diff, maps, gop, out, delta_layout, N.lib().csic_undelta_host)


def mc_layout(c_params: N.CsicParams) -> N.CsicMcLayout:
    """csic_mc_layout_of: groups, row widths, the tables' and the nibble sections' offsets, map_bytes, map_stride and the device codec's
    workspace bytes per frame."""
    lay = N.CsicMcLayout()
    N.check(N.lib().csic_mc_layout_of(C.byref(c_params), C.byref(lay)))
    return lay


def mc_delta_host(c_params: N.CsicParams, frames, gop: int, motion: int, out=None):
    """csic_mc_delta_host: PLANAR_BITS frame buffers (nframes, frame_bytes) -> (diff, maps) with displacements of up to `motion`
    samples either way: the difference frames, an array of the same shape (zero outside the payload ranges, or `out` -- not `frames`:
    there is no in-place form), and the maps, uint8 (nframes, map_stride) with map_bytes of each row written."""
    return _temporal_forward(c_params, frames, out, mc_layout, N.lib().csic_mc_delta_host, int(gop), int(motion))


def mc_undelta_host(c_params: N.CsicParams, diff, maps, gop: int, out=None) -> np.ndarray:
    """csic_mc_undelta_host: the inverse of mc_delta_host.  The maps are untrusted: a damaged table, a nibble above its table, a set
    padding nibble or a non-zero map of a key frame raises CsicIOError (CSIC_EFORMAT) and nothing is written."""
    return _temporal_inverse(c_params, diff, maps, gop, out, mc_layout, N.lib().csic_mc_undelta_host)


def rows_layout(c_params: N.CsicParams) -> N.CsicRowsLayout:
    """csic_rows_layout_of: groups, row widths, K, the band length S, the sections' offsets, map_bytes and map_stride of a frame's map."""
    lay = N.CsicRowsLayout()
    N.check(N.lib().csic_rows_layout_of(C.byref(c_params), C.byref(lay)))
    return lay


def rows_host(c_params: N.CsicParams, frames, out=None):
    """csic_rows_host: PLANAR_BITS frame buffers (nframes, frame_bytes) -> (diff, maps): the difference frames, an array of the same
    shape (zero outside the payload ranges, or `out` -- not `frames`: there is no in-place form), and the maps, uint8 (nframes,
    map_stride) with map_bytes of each row written."""
    return _temporal_forward(c_params, frames, out, rows_layout, N.lib().csic_rows_host)


def unrows_host(c_params: N.CsicParams, diff, maps, out=None) -> np.ndarray:
    """csic_unrows_host: the inverse of rows_host (`out` may be `diff`, in place).  The maps are untrusted: a set padding bit, or a set
    bit of a plane whose rows are shorter than a group, raises CsicIOError (CSIC_EFORMAT) and nothing is written."""
    return _temporal_inverse(c_params, diff, maps, None, out, rows_layout, N.lib().csic_unrows_host)


def _seq_entry(plain, ex, gop, motion):
    """-> (the writer of a sequence file, its arguments behind the coding): version 5, or with a `motion` range the _ex form, version 6."""
    return (plain, (int(gop),)) if motion is None else (ex, (int(gop), int(motion)))


def write_container(path: str, c_params: N.CsicParams, frames, coding="raw", gop=None, motion=None, rows=False) -> None:
    """frames: the PLANAR_BITS frame buffers of `c_params` (its out_format does not matter), frame_bytes each -- one buffer, an
    array (nframes, frame_bytes), or a list of buffers.  Only the planes' payload bytes reach the file.  coding = "raw" (version 1,
    the bytes as they are), "groups" (version 3, every frame group-coded on the host: csic_container_write_ex) or "rice" (version 4,
    every frame Rice-coded on the host) or "rans" (version 7, every frame rANS-coded on the host).  With a `gop` the frames are a sequence: version 5, delta and packing on the host
    (csic_container_write_seq; coding "groups" or "rice"); with a `motion` range (0..7) as well, version 6 through the
    motion-compensated layer (csic_container_write_seq_ex); a sequence coded with "rans" is version 7 with either layer.  rows=True:
    version 8, every frame through the row-prediction layer and then the coding, on the host (csic_container_write_rows); it takes a
    coding other than "raw" and neither gop nor motion."""
    q, lay = _bits_params(c_params)
    coding = _coding(coding)
    if rows:
        if gop is not None or motion is not None:
            raise N.IllegalArgumentException(N.EINVAL_FORMAT, "requirement failed: the row-prediction layer does not combine with gop or motion")
        a = _frames_2d(frames, lay.frame_bytes)
        N.check(N.lib().csic_container_write_rows(os.fsencode(path), C.byref(q), a.ctypes.data_as(C.c_void_p), a.shape[0], coding))
        return
    if motion is not None and gop is None:
        raise N.IllegalArgumentException(N.EINVAL_NULL, "requirement failed: motion needs a gop")
    if gop is not None:
        a = _frames_2d(frames, lay.frame_bytes)
        write, layer = _seq_entry(N.lib().csic_container_write_seq, N.lib().csic_container_write_seq_ex, gop, motion)
        N.check(write(os.fsencode(path), C.byref(q), a.ctypes.data_as(C.c_void_p), a.shape[0], coding, *layer))
        return
    if isinstance(frames, (list, tuple)):
        frames = np.stack([np.ascontiguousarray(f).reshape(-1).view(np.uint8) for f in frames])
    a = np.ascontiguousarray(frames).reshape(-1).view(np.uint8)
    if a.size == 0 or a.size % lay.frame_bytes != 0:
        raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: frames must hold whole frame buffers of {lay.frame_bytes} bytes, got {a.size}")
    if coding == N.CODING_RAW:
        N.check(N.lib().csic_container_write(os.fsencode(path), C.byref(q), a.ctypes.data_as(C.c_void_p), a.size // lay.frame_bytes))
    else:
        N.check(N.lib().csic_container_write_ex(os.fsencode(path), C.byref(q), a.ctypes.data_as(C.c_void_p), a.size // lay.frame_bytes, coding))


def write_container_coded(path: str, c_params: N.CsicParams, coded, sizes, coding="groups", maps=None, gop=None, motion=None, rows=False) -> None:
    """Version 3 (coding "groups"), 4 ("rice") or 7 ("rans") from frames that are packed already (csic_container_write_coded_ex): `coded` is an
    array (nframes, stride) -- what Plan.pack_device / Plan.rice_pack_device returns, copied to the host -- or a list of coded frames;
    sizes[k] is frame k's coded_bytes.  Every frame is validated before anything is written.  With `maps` and `gop` -- what
    Plan.delta_device returned, copied to the host: uint8 (nframes, map_stride) -- the coded frames are difference frames and the file is
    version 5 (csic_container_write_coded_seq); with `motion` too the maps are Plan.mc_delta_device's and the file is version 6
    (csic_container_write_coded_seq_ex).  rows=True: `maps` are Plan.rows_device's, there is no gop, and the file is version 8
    (csic_container_write_coded_rows)."""
    if rows and (maps is None or gop is not None or motion is not None):
        raise N.IllegalArgumentException(N.EINVAL_FORMAT, "requirement failed: the row-prediction layer takes maps, and neither gop nor motion")
    if not rows and (maps is None) != (gop is None):
        raise N.IllegalArgumentException(N.EINVAL_NULL, "requirement failed: maps and gop go together")
    q, _ = _bits_params(c_params)
    coding = _coding(coding)
    sz = np.ascontiguousarray(np.asarray(sizes).reshape(-1), dtype=np.uint64)
    if isinstance(coded, (list, tuple)):
        rows = [np.ascontiguousarray(f).reshape(-1).view(np.uint8) for f in coded]
        stride = max([r.size for r in rows] + [1])
        a = np.zeros((len(rows), stride), dtype=np.uint8)
        for k, r in enumerate(rows):
            a[k, :r.size] = r
    else:
        a = np.ascontiguousarray(coded).view(np.uint8)
        a = a.reshape(sz.size, -1) if sz.size and a.size % sz.size == 0 else a.reshape(1, -1)
    if sz.size == 0 or a.shape[0] != sz.size:
        raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: {a.shape[0]} coded frames but {sz.size} sizes")
    if maps is not None:
        m = np.ascontiguousarray(maps).view(np.uint8)
        if m.size == 0 or m.size % sz.size != 0:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: {m.size} bytes of maps for {sz.size} frames")
        write, layer = (N.lib().csic_container_write_coded_rows, ()) if rows else \
            _seq_entry(N.lib().csic_container_write_coded_seq, N.lib().csic_container_write_coded_seq_ex, gop, motion)
        N.check(write(os.fsencode(path), C.byref(q), a.ctypes.data_as(C.c_void_p), a.shape[1], sz.ctypes.data_as(C.POINTER(C.c_uint64)),
                      m.ctypes.data_as(C.c_void_p), m.size // sz.size, int(sz.size), coding, *layer))
        return
    N.check(N.lib().csic_container_write_coded_ex(os.fsencode(path), C.byref(q), a.ctypes.data_as(C.c_void_p), a.shape[1],
                                                  sz.ctypes.data_as(C.POINTER(C.c_uint64)), int(sz.size), coding))


def container_coded_sizes(path: str) -> np.ndarray:
    """The stored bytes of each frame (csic_container_coded_sizes): a version-3 or version-4 file's table, payload_bytes per frame for
    version 1."""
    info = container_info(path)
    sizes = np.zeros(info.nframes, dtype=np.uint64)
    N.check(N.lib().csic_container_coded_sizes(os.fsencode(path), sizes.ctypes.data_as(C.POINTER(C.c_uint64)), info.nframes))
    return sizes


def container_inter_groups(path: str) -> np.ndarray:
    """csic_container_inter_groups: uint64 (nframes, 3), the inter groups of each frame and plane (the popcounts of a version-5 file's
    maps; zeros for key frames and for versions 1, 3 and 4; for version 8 the groups predicted from the row above)."""
    info = container_info(path)
    counts = np.zeros((info.nframes, 3), dtype=np.uint64)
    N.check(N.lib().csic_container_inter_groups(os.fsencode(path), counts.ctypes.data_as(C.POINTER(C.c_uint64)), 3 * info.nframes))
    return counts


def read_container(path: str) -> Tuple[N.CsicParams, int, np.ndarray]:
    """-> (c_params, nframes, frames): frames is a uint8 array (nframes, frame_bytes), zero outside the planes' payload."""
    info = container_info(path)
    lay = N.CsicPlanarBitsLayout()
    N.check(N.lib().csic_planar_bits_layout_of(C.byref(info.params), C.byref(lay)))
    frames = np.empty((info.nframes, lay.frame_bytes), dtype=np.uint8)
    N.check(N.lib().csic_container_read(os.fsencode(path), frames.ctypes.data_as(C.c_void_p), frames.size))
    return N.CsicParams.from_buffer_copy(info.params), info.nframes, frames
