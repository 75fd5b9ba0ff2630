"""The row-prediction layer (csic_rows_*; include/csic.h) stated in numpy, straight from the definition and independent of the C++: the
reference of a sample (the sample one row above inside its band, else 0), the two costs of a group, the choice, the difference planes,
the maps and the inverse.  A helper module without tests: tests/test_rows_host.py checks the host codec against it,
tests/test_gpu_rows.py the device codec, tests/test_container_v8.py and tests/test_rows_sizes.py build files and sizes from it;
tests/rows_planes.py builds planes to order with it (conditions: tests/test_rows_planes_host.py) and tests/test_gpu_rows_planes.py
holds the device codec to it on those planes.

A frame is three planes of codes (int64, values < 2^q); `widths` are the planes' row widths w_p."""
import numpy as np

from delta_ref import ref_map_layout

BAND = 16                                  # CSIC_ROWS_BAND


def ref_fold(e, q):
    """The folded, centred value of e mod 2^q."""
    e = e % (1 << q)
    s = np.where(e < (1 << (q - 1)), e, e - (1 << q))
    return np.where(s >= 0, 2 * s, -2 * s - 1)


def ref_constants(w):
    """-> (K, S) of a plane of row width w."""
    K = w // 32
    return K, 32 * K * BAND


def ref_reference(x, w):
    """ref(i) for every sample of a plane (K >= 1)."""
    _, S = ref_constants(w)
    i = np.arange(x.size)
    ok = i - w >= S * (i // S)
    return np.where(ok, x[np.maximum(i - w, 0)], 0)


def _grouped(v):
    n = v.size
    G = (n + 31) // 32
    out = np.zeros(32 * G, dtype=np.int64)
    out[:n] = v
    return out.reshape(G, 32), (np.arange(32 * G) < n).reshape(G, 32)


def ref_rows_plane(x, w, q):
    """One plane -> (the difference plane's values, t per group)."""
    x = np.asarray(x, dtype=np.int64)
    G = (x.size + 31) // 32
    if ref_constants(w)[0] == 0:
        return x.copy(), np.zeros(G, dtype=bool)
    u = (x - ref_reference(x, w)) % (1 << q)
    xg, real = _grouped(x)
    ug, _ = _grouped(u)
    cost_left = (ref_fold(xg[:, 1:] - xg[:, :-1], q) * real[:, 1:]).sum(axis=1)
    cost_up = (ref_fold(ug[:, 1:], q) * real[:, 1:]).sum(axis=1)
    t = cost_up < cost_left                                   # a tie is 0
    v = np.cumsum(ug * real, axis=1) % (1 << q)
    return np.where(t[:, None], v, xg).reshape(-1)[:x.size], t


def ref_rows(planes, widths, bits):
    """A frame -> (its difference frame, its map as bytes of map_bytes, t per plane)."""
    out = [ref_rows_plane(x, w, q) for x, w, q in zip(planes, widths, bits)]
    m = b""
    for _, t in out:
        sec = np.zeros((t.size + 31) // 32 * 32, dtype=np.uint8)
        sec[:t.size] = t
        m += np.packbits(sec, bitorder="little").tobytes()
    return [d for d, _ in out], m, [t for _, t in out]


def ref_unrows(diff, m, widths, bits):
    """The inverse, from the map's bytes, sample by sample in increasing i."""
    G, off, _, _ = ref_map_layout([d.size for d in diff])
    mb = np.unpackbits(np.frombuffer(m, dtype=np.uint8), bitorder="little")
    frame = []
    for p, (d, w, q) in enumerate(zip(diff, widths, bits)):
        K, S = ref_constants(w)
        x = np.asarray(d, dtype=np.int64).copy()
        for g in np.nonzero(mb[8 * off[p]:8 * off[p] + G[p]])[0] if K else ():
            for i in range(32 * g, min(32 * g + 32, x.size)):
                u = d[i] if i == 32 * g else (d[i] - d[i - 1]) % (1 << q)
                x[i] = (u + (x[i - w] if i - w >= S * (i // S) else 0)) % (1 << q)
        frame.append(x)
    return frame
