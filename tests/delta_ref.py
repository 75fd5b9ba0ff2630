"""The temporal layer (csic_delta_*; include/csic.h) stated in numpy, independent of the C++ and of the codecs' reference encoders: key
and delta frames, the per-group choice by the sum of the folded residuals, the difference frames and the maps.  A helper module without
tests: tests/test_delta_host.py checks the host codec against it, tests/test_gpu_delta.py the device codec, tests/test_container_v5.py
and tests/test_delta_sequences.py build files and sizes from it.

A frame is three planes of codes (int64, values < 2^q); a sequence is a list of frames."""
import numpy as np

from test_container import _frame_buffer
from test_pack_host import plane_bytes


def _groups(v):
    """A plane of n values -> (G, 32) with zeros behind the last one, and the mask of the real slots."""
    n = v.size
    G = (n + 31) // 32
    out = np.zeros(32 * G, dtype=np.int64)
    out[:n] = v
    return out.reshape(G, 32), (np.arange(32 * G) < n).reshape(G, 32)


def ref_cost(v, real, q):
    """Per group: the sum over the real slots j >= 1 of the folded, centred left residual of the values v."""
    e = (v[:, 1:] - v[:, :-1]) % (1 << q)
    s = np.where(e < (1 << (q - 1)), e, e - (1 << q))
    u = np.where(s >= 0, 2 * s, -2 * s - 1)
    return (u * real[:, 1:]).sum(axis=1)


def ref_delta_plane(c, r, q):
    """One plane of a delta frame against the previous frame's -> (the difference plane's values, t per group)."""
    cg, real = _groups(np.asarray(c, dtype=np.int64))
    rg, _ = _groups(np.asarray(r, dtype=np.int64))
    d = (cg - rg) % (1 << q)
    t = ref_cost(d, real, q) < ref_cost(cg, real, q)          # a tie is intra
    return np.where(t[:, None], d, cg).reshape(-1)[:c.size], t


def ref_map_layout(ns):
    """-> (groups, section offsets, map_bytes, map_stride)"""
    G = [(n + 31) // 32 for n in ns]
    sec = [4 * ((g + 31) // 32) for g in G]
    return G, [0, sec[0], sec[0] + sec[1]], sum(sec), (sum(sec) + 255) // 256 * 256


def ref_delta(frames, bits, gop):
    """A sequence -> (the difference frames, as frames; the maps, bytes of map_bytes each; t per frame and plane, None for key frames)."""
    diffs, maps, ts = [], [], []
    for k, planes in enumerate(frames):
        if k % gop == 0:
            diffs.append([np.asarray(c, dtype=np.int64) for c in planes])
            maps.append(bytes(ref_map_layout([c.size for c in planes])[2]))
            ts.append(None)
            continue
        out = [ref_delta_plane(c, r, q) for c, r, q in zip(planes, frames[k - 1], bits)]
        diffs.append([d for d, _ in out])
        m = b""
        for _, t in out:
            bitsec = np.zeros((t.size + 31) // 32 * 32, dtype=np.uint8)
            bitsec[:t.size] = t
            m += np.packbits(bitsec, bitorder="little").tobytes()
        maps.append(m)
        ts.append([t for _, t in out])
    return diffs, maps, ts


def ref_undelta(diffs, maps, bits, gop):
    """The inverse, from the maps' bytes."""
    frames = []
    for k, planes in enumerate(diffs):
        if k % gop == 0:
            frames.append([np.asarray(d, dtype=np.int64) for d in planes])
            continue
        G, off, _, _ = ref_map_layout([d.size for d in planes])
        m = np.unpackbits(np.frombuffer(maps[k], dtype=np.uint8), bitorder="little")
        out = []
        for p, (d, q) in enumerate(zip(planes, bits)):
            t = np.repeat(m[8 * off[p]:8 * off[p] + G[p]].astype(bool), 32)[:d.size]
            out.append(np.where(t, (d + frames[k - 1][p]) % (1 << q), d))
        frames.append(out)
    return frames


def frame_buffers(lay, frames, bits, fill):
    """The PLANAR_BITS frame buffers of a sequence: `fill` outside the payload ranges.  uint8 (nframes, frame_bytes)."""
    return np.stack([_frame_buffer(lay, [plane_bytes(c, q) for c, q in zip(planes, bits)], fill) for planes in frames])


def map_buffers(maps, stride, fill):
    """The maps `stride` apart, `fill` behind map_bytes.  uint8 (nframes, stride)."""
    out = np.full((len(maps), stride), fill, dtype=np.uint8)
    for k, m in enumerate(maps):
        out[k, :len(m)] = np.frombuffer(m, dtype=np.uint8)
    return out
