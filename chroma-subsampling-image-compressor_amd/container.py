""".csic files: CSIC_FMT_PLANAR_BITS frames on disk (csic_container_*; byte layout in include/csic.h).  Host only: nothing here
needs a GPU."""
from __future__ import annotations

import ctypes as C
import os
from typing import Tuple

import numpy as np

from . import _native as N


def container_info(path: str) -> N.CsicContainerInfo:
    """Header, parameters and length of a .csic file (csic_container_info_of; everything read_container checks but the CRC)."""
    info = N.CsicContainerInfo()
    N.check(N.lib().csic_container_info_of(os.fsencode(path), C.byref(info)))
    return info


def write_container(path: str, c_params: N.CsicParams, frames) -> None:
    """frames: the PLANAR_BITS frame buffers of `c_params` (its out_format does not matter), frame_bytes each -- one buffer, an
    array (nframes, frame_bytes), or a list of buffers.  Only the planes' payload bytes reach the file."""
    lay = N.CsicPlanarBitsLayout()
    q = N.CsicParams.from_buffer_copy(c_params)
    q.out_format = N.FMT_PLANAR_BITS
    N.check(N.lib().csic_validate(C.byref(q)))
    N.check(N.lib().csic_planar_bits_layout_of(C.byref(q), C.byref(lay)))
    if isinstance(frames, (list, tuple)):
        frames = np.stack([np.ascontiguousarray(f).reshape(-1).view(np.uint8) for f in frames])
    a = np.ascontiguousarray(frames).reshape(-1).view(np.uint8)
    if a.size == 0 or a.size % lay.frame_bytes != 0:
        raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: frames must hold whole frame buffers of {lay.frame_bytes} bytes, got {a.size}")
    N.check(N.lib().csic_container_write(os.fsencode(path), C.byref(q), a.ctypes.data_as(C.c_void_p), a.size // lay.frame_bytes))


def read_container(path: str) -> Tuple[N.CsicParams, int, np.ndarray]:
    """-> (c_params, nframes, frames): frames is a uint8 array (nframes, frame_bytes), zero outside the planes' payload."""
    info = container_info(path)
    lay = N.CsicPlanarBitsLayout()
    N.check(N.lib().csic_planar_bits_layout_of(C.byref(info.params), C.byref(lay)))
    frames = np.empty((info.nframes, lay.frame_bytes), dtype=np.uint8)
    N.check(N.lib().csic_container_read(os.fsencode(path), frames.ctypes.data_as(C.c_void_p), frames.size))
    return N.CsicParams.from_buffer_copy(info.params), info.nframes, frames
