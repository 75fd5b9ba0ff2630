"""The motion-compensated temporal layer (csic_mc_*; include/csic.h) stated in numpy, independent of the C++: displacements that clamp,
the candidates and their rank, the vote, the table, the per-group choice, the difference frames and the maps.  A helper module without
tests: tests/test_mc_host.py checks the host codec against it, tests/test_gpu_mc.py the device codec, tests/test_mc_sequences.py takes
sizes from it.  The groups, cost() and the frame buffers are those of tests/delta_ref.py.

A frame is three planes of codes (int64, values < 2^q); a sequence is a list of frames; `widths` are the planes' row widths w_p."""
import numpy as np

from delta_ref import _groups, ref_cost

TABLE_WORDS, TABLE_BYTES = 16, 64


def candidates(R):
    """All (dy, dx) of [-R, R]^2 in rank order: by (|dx| + |dy|, dy, dx); rank 0 is the zero vector."""
    return sorted(((dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)), key=lambda v: (abs(v[0]) + abs(v[1]), v[0], v[1]))


def displaced(r, s):
    """r[clamp(i + s, 0, n - 1)] for every i."""
    r = np.asarray(r, dtype=np.int64)
    return r[np.clip(np.arange(r.size, dtype=np.int64) + int(s), 0, r.size - 1)]


def _cost_of(c, r, s, q):
    """Per group: cost() of d = (c - r displaced by s) mod 2^q -> (cost, d as (G, 32)).  The same arithmetic as delta_ref.ref_cost, in
    16-bit integers (codes have at most 8 bits, a folded residual at most 9): the sequences of 512 x 512 price 81 candidates per plane."""
    c, r = np.asarray(c, dtype=np.int16), np.asarray(r, dtype=np.int16)
    n, mask, half = c.size, np.int16((1 << q) - 1), np.int16(1 << (q - 1))
    G = (n + 31) // 32
    d = np.zeros(32 * G, dtype=np.int16)
    d[:n] = (c - r[np.clip(np.arange(n, dtype=np.int64) + int(s), 0, n - 1)]) & mask
    d = d.reshape(G, 32)
    e = (d[:, 1:] - d[:, :-1]) & mask
    u = np.where(e < half, 2 * e, 2 * (mask + 1 - e) - 1)
    u[(np.arange(32 * G) >= n).reshape(G, 32)[:, 1:]] = 0                   # slots behind the last sample add nothing
    return u.sum(axis=1, dtype=np.int64), d.astype(np.int64)


def ref_mc_plane(c, r, q, w, R):
    """One plane of a delta frame -> (the difference plane's values, the table's 16 words, the nibble per group)."""
    c = np.asarray(c, dtype=np.int64)
    cg, real = _groups(c)
    ss = [dy * w + dx for dy, dx in candidates(R)]
    costs = np.stack([_cost_of(c, r, s, q)[0] for s in ss])                # (K, G)
    votes = np.bincount(np.argmin(costs, axis=0), minlength=len(ss))        # argmin: the first, i.e. the lowest rank, among the cheapest
    voted = sorted((k for k in range(1, len(ss)) if votes[k]), key=lambda k: (-votes[k], k))[:TABLE_WORDS - 2]
    table = [1 + len(voted), 0] + [ss[k] for k in voted]
    T = table[0]
    tc, td = zip(*[_cost_of(c, r, s, q) for s in table[1:]])
    tc = np.stack(tc)                                                       # (T, G)
    t = np.argmin(tc, axis=0)                                               # the lowest t among the cheapest (0-based)
    inter = tc[t, np.arange(t.size)] < ref_cost(cg, real, q)                # a tie is intra
    d = np.stack(td)[t, np.arange(t.size)]
    out = np.where(inter[:, None], d, cg).reshape(-1)[:c.size]
    return out, table + [0] * (TABLE_WORDS - 1 - T), np.where(inter, t + 1, 0)


def ref_mc_layout(ns):
    """-> (groups, table offsets, nibble section offsets, map_bytes, map_stride)"""
    G = [(n + 31) // 32 for n in ns]
    sec = [4 * ((g + 7) // 8) for g in G]
    off = [3 * TABLE_BYTES, 3 * TABLE_BYTES + sec[0], 3 * TABLE_BYTES + sec[0] + sec[1]]
    mb = 3 * TABLE_BYTES + sum(sec)
    return G, [0, TABLE_BYTES, 2 * TABLE_BYTES], off, mb, (mb + 255) // 256 * 256


def map_bytes_of(tables, nibbles):
    """The map of a delta frame from its three tables and its three nibble arrays."""
    m = b"".join(np.array(t, dtype=np.int64).astype(np.int32).astype("<i4").tobytes() for t in tables)
    for nb in nibbles:
        sec = np.zeros((nb.size + 7) // 8 * 8, dtype=np.uint8)
        sec[:nb.size] = nb
        m += (sec[0::2] | (sec[1::2] << 4)).astype(np.uint8).tobytes()
    return m


def ref_mc_delta(frames, bits, widths, gop, R):
    """A sequence -> (the difference frames, as frames; the maps, bytes of map_bytes each; per frame and plane (table, nibbles), None
    for key frames)."""
    diffs, maps, info = [], [], []
    for k, planes in enumerate(frames):
        if k % gop == 0:
            diffs.append([np.asarray(c, dtype=np.int64) for c in planes])
            maps.append(bytes(ref_mc_layout([c.size for c in planes])[3]))
            info.append(None)
            continue
        out = [ref_mc_plane(c, r, q, w, R) for c, r, q, w in zip(planes, frames[k - 1], bits, widths)]
        diffs.append([o[0] for o in out])
        maps.append(map_bytes_of([o[1] for o in out], [o[2] for o in out]))
        info.append([(o[1], o[2]) for o in out])
    return diffs, maps, info


def parse_map(m, ns):
    """A map's bytes -> per plane (the 16 table words as int32, the nibbles of the section, padding included)."""
    G, toff, off, _, _ = ref_mc_layout(ns)
    a = np.frombuffer(bytes(m), dtype=np.uint8)
    out = []
    for p in range(3):
        sec = a[off[p]:off[p] + 4 * ((G[p] + 7) // 8)]
        nib = np.stack([sec & 15, sec >> 4], axis=1).reshape(-1)
        out.append((np.frombuffer(a[toff[p]:toff[p] + TABLE_BYTES].tobytes(), dtype="<i4").astype(np.int64), nib.astype(np.int64)))
    return out


def ref_mc_undelta(diffs, maps, bits, gop):
    """The inverse, from the maps' bytes: any nibble reads one of the 16 words, any word clamps."""
    frames = []
    for k, planes in enumerate(diffs):
        if k % gop == 0:
            frames.append([np.asarray(d, dtype=np.int64) for d in planes])
            continue
        out = []
        for (table, nib), d, r, q in zip(parse_map(maps[k], [d.size for d in planes]), planes, frames[k - 1], bits):
            d = np.asarray(d, dtype=np.int64)
            t = np.repeat(nib, 32)[:d.size]
            at = np.clip(np.arange(d.size, dtype=np.int64) + table[t], 0, d.size - 1)
            out.append(np.where(t > 0, (d + r[at]) % (1 << q), d))
        frames.append(out)
    return frames
