"""Code planes built to order for the two lossless codecs (the group coding and the Rice coding): what a device kernel sees is chosen here
and not left to the colour transform and the quantiser.  A helper module without tests: tests/test_codec_planes_host.py proves every
builder's condition with the numpy reference alone, tests/test_gpu_codec_planes.py feeds the planes to the device codecs.

Every builder returns three planes of codes (int64, values < 2^q, read-only) for an n x 1, 4:4:4, factor-1 plan, where every plane has
exactly n samples.  The three planes of one builder are alike; planes_for() takes plane p from the builder at bits[p], so that a frame
of three different widths is three different planes."""
import functools

import numpy as np

from test_pack_host import ref_encode, ref_groups
import test_rice_host as _rice          # (test_rice_host imports groups_of_mode inside its test: no cycle at import time)

BLOCK = 256
POOL = 8


def reachable_modes(q):
    """The modes an encoder that takes the cheapest k can emit: 15 and every k = 0 .. q but q - 1 (test_every_mode_of_every_width)."""
    return [15] + [k for k in range(q + 1) if k != q - 1]


def groups_of_mode(q, k, rng, count, tries=200):
    """Up to `count` distinct groups of 32 codes whose cheapest mode is k (15: constant groups, of which there are only 2^q): walks with
    steps of about k bits, until k is the cheapest parameter.  Fewer than `count` (none for k = q - 1, which is never the cheapest) when
    `tries` draws per group do not find them."""
    if k == 15:
        return [np.full(32, int(v), dtype=np.int64) for v in rng.permutation(1 << q)[:count]]
    found, seen = [], set()
    mag = 1 << k
    for _ in range(tries * count):
        c = np.cumsum(rng.integers(-mag, mag + 1, 32)) % (1 << q)
        if _rice.ref_modes(ref_groups(c, q)[2], q)[0] == k and c.tobytes() not in seen:
            seen.add(c.tobytes())
            found.append(c.astype(np.int64))
            if len(found) == count:
                break
    return found


def codes_of_residuals(u, q, anchor=0):
    """32 folded residuals (u[0] is ignored) -> the group's codes, by the decode rule."""
    u = np.asarray(u, dtype=np.int64)
    s = np.where(u % 2 == 0, u // 2, -(u + 1) // 2)
    s[0] = anchor
    return np.cumsum(s) % (1 << q)


def group_of_width(q, w, rng):
    """A group whose largest folded residual has exactly w >= 1 significant bits."""
    u = rng.integers(0, 1 << w, 32)
    u[int(rng.integers(1, 32))] |= 1 << (w - 1)
    c = codes_of_residuals(u, q, int(rng.integers(0, 1 << q)))
    assert ref_groups(c, q)[0].tolist() == [w]
    return c


def _frozen(planes):
    for c in planes:
        c.setflags(write=False)
    return tuple(planes)


@functools.lru_cache(maxsize=None)
def pools(q):
    """{mode: at least 8 distinct groups of that mode (mode 15: min(8, 2^q) constant groups)} for every reachable mode of q."""
    rng = np.random.default_rng(13000 + q)
    out = {k: groups_of_mode(q, k, rng, POOL) for k in reachable_modes(q)}
    assert all(len(v) == (min(POOL, 1 << q) if k == 15 else POOL) for k, v in out.items()), q
    return out


@functools.lru_cache(maxsize=None)
def runs_frame(q):
    """One block per mode k = 0 .. q but q - 1, in rising order: 256 consecutive groups of that mode, a pool of 8 distinct groups in a
    cycle.  All lanes of a block then add the same 31 k bits to R, so lane t's bit offset is 31 k t: every residue mod 32, and for
    small k a whole 31 k-bit run strictly inside one dword, between two neighbours' runs.  (Zero mode has no block of its own here, which
    keeps runs_frame(8) at 8 blocks: a block of constant groups is block 1 of full_chunk_frame, and shuffled_frame mixes them in.)"""
    p = pools(q)
    groups = [p[k][i % POOL] for k in reachable_modes(q)[1:] for i in range(BLOCK)]
    c = np.concatenate(groups)
    return _frozen([c, c.copy(), c.copy()])


SHUFFLED_GROUPS = 2 * BLOCK + 37                      # three blocks, the last one ragged
SHUFFLED_N = 32 * SHUFFLED_GROUPS - 13                # and the last group as well


@functools.lru_cache(maxsize=None)
def shuffled_frame(q):
    """The pools of runs_frame, the constant groups and one group of every width w = 1 .. q, in a random order over three blocks: 549
    groups, so the last block is ragged, and n = 32 * 549 - 13, so the last group is."""
    rng = np.random.default_rng(13100 + q)
    every = [g for k in reachable_modes(q) for g in pools(q)[k]] + [group_of_width(q, w, rng) for w in range(1, q + 1)]
    assert len(every) <= SHUFFLED_GROUPS
    order = rng.permutation(SHUFFLED_GROUPS)
    c = np.concatenate([every[i % len(every)] for i in order])[:SHUFFLED_N]
    return _frozen([c, c.copy(), c.copy()])


@functools.lru_cache(maxsize=None)
def long_runs(q):
    """[(k, r, zeros)]: the single positive residuals r (a step of +r inside a constant group: u = 2 r) whose group's cheapest mode k
    has the longest unary run there is, zeros = (2 r) >> k; per k the smallest such r."""
    best = {}
    for r in range(1, 1 << (q - 1)):
        u = np.zeros((1, 32), dtype=np.int64)
        u[0, 5] = 2 * r
        k = int(_rice.ref_modes(u, q)[0])
        if k < q:
            zeros = (2 * r) >> k
            if k not in best or zeros > best[k][1]:
                best[k] = (r, zeros)
    top = max((z for _, z in best.values()), default=0)
    return [(k, r, z) for k, (r, z) in sorted(best.items()) if z == top]


LONG_RUN_SLOTS = (1, 2, 7, 16, 17, 30, 31)


@functools.lru_cache(maxsize=None)
def long_run_groups(q):
    """For every (k, r) of long_runs(q), 64 groups in a row that are constant but for one step of +r, the step at several slots in turn
    and the anchors all different: for q >= 6 the cheapest mode k has a unary run of 62 zeros, which the writer flushes twice and which
    leaves a dword of U without a terminator; for q = 5, 4, 3, 2 the run is 30, 14, 6, 2 zeros; at q = 1 the only step there is."""
    groups = []
    for k, r, _ in long_runs(q) or [(1, 1, 0)]:
        for i in range(64):
            c = np.full(32, (7 * i + 3) % (1 << q), dtype=np.int64)
            c[LONG_RUN_SLOTS[i % len(LONG_RUN_SLOTS)]:] += r
            groups.append(c % (1 << q))
    c = np.concatenate(groups)
    return _frozen([c, c.copy(), c.copy()])


@functools.lru_cache(maxsize=None)
def full_cost_group(q):
    """A group whose cheapest mode is k = q - 2 at a cost of exactly 31 q bits, what a raw group costs (q >= 2): every u >> (q - 2) is
    1, the low bits are drawn until no smaller k costs as little."""
    rng = np.random.default_rng(13200 + q)
    k = q - 2
    for _ in range(1000):
        u = (1 << k) | rng.integers(0, 1 << k, 32)
        c = codes_of_residuals(u, q, int(rng.integers(0, 1 << q)))
        uu = ref_groups(c, q)[2]
        if _rice.ref_modes(uu, q)[0] == k and 31 * k + int(((uu[0, 1:] >> k) + 1).sum()) == 31 * q:
            return c
    raise AssertionError(q)


def full_chunk_dwords(q):
    """The format's longest chunk: 248 q + 1 dwords; q = 1 has no mode below raw and stops at 248."""
    return 248 * q + 1 if q >= 2 else 248


@functools.lru_cache(maxsize=None)
def full_chunk_frame(q):
    """Three blocks of 256 groups.  Blocks 0 and 2 are chunks of the format's maximum: 255 raw groups (31 q bits each) and one group of
    mode q - 2 that costs 31 q bits as well, 62 of them in U -- R takes 248 q - 1 dwords, U two.  Block 1 is all constant groups: an
    empty chunk between two full ones."""
    rng = np.random.default_rng(13300 + q)
    raw = pools(q)[q]
    groups = []
    for at in (100, None, 255):
        if at is None:
            groups += [np.full(32, int(rng.integers(0, 1 << q)), dtype=np.int64) for _ in range(BLOCK)]
        else:
            blk = [raw[i % POOL] for i in rng.integers(0, POOL, BLOCK)]
            if q >= 2:
                blk[at] = full_cost_group(q)
            groups += blk
    c = np.concatenate(groups)
    return _frozen([c, c.copy(), c.copy()])


FOREIGN_N = 32 * 9 + 7


@functools.lru_cache(maxsize=None)
def foreign_frames(q):
    """Valid streams that this project's encoders never write.  The plane of test_unpack_takes_every_mode_the_format_allows (a +-1 walk
    of 32 * 9 + 7 samples with one constant group) with one step of -2^(q - 1), whose u = 2^q - 1 is a run of 2^q - 1 zeros at k = 0.
    -> (planes, [(k, the Rice stream in which every group that is not constant takes mode k) for k = 0 .. q],
                [(w, the group stream in which every group is stored at max(w_g, w)) for w = 0 .. q])."""
    rng = np.random.default_rng(13400 + q)
    steps = rng.integers(-1, 2, FOREIGN_N)
    steps[200] = -(1 << (q - 1))
    c = (np.cumsum(steps) % (1 << q)).astype(np.int64)
    c[64:96] = c[64]                                       # a zero group in between
    assert ref_groups(c, q)[2].max() == (1 << q) - 1
    planes = _frozen([c, c.copy(), c.copy()])
    rice = [(k, _rice.ref_encode_rice(planes, (q, q, q), force=k)) for k in range(q + 1)]
    grp = [(w, ref_encode(planes, (q, q, q), force=w)) for w in range(q + 1)]
    return planes, rice, grp


# ---- three planes of three widths -------------------------------------------------------------------------
TRIPLES = [(q, q % 8 + 1, (q + 1) % 8 + 1) for q in range(1, 9)] + [(8, 8, 8), (5, 5, 3)]


def cycled(c, n):
    """Plane c brought to n samples by repeating its whole groups."""
    if c.size == n:
        return c
    whole = c[:c.size // 32 * 32]
    return np.tile(whole, -(-n // whole.size))[:n] if c.size < n else c[:n]


def planes_for(builder, bits, n=None):
    """Plane p of builder(bits[p]), the shorter planes cycled to the longest one's n samples (or all of them to `n`)."""
    planes = [builder(q)[p] for p, q in enumerate(bits)]
    n = max(c.size for c in planes) if n is None else n
    return [cycled(c, n) for c in planes]


def modes_of(c, q):
    return set(_rice.ref_modes(ref_groups(c, q)[2], q).tolist())


def widths_of(c, q):
    return set(ref_groups(c, q)[0].tolist())
