"""Code planes built to order for the row-prediction layer (csic_rows_*), in the style of tests/rans_planes.py, and the numpy statement
of tests/rows_ref.py once more with one switch per rule, so that a plane can be shown to tell the definition from its near-misses:

    contest_plane       sparse-noise rows, then every group steered to cost_up - cost_left = -1, 0, +1 in turn: a tie, and a choice
                        decided by one; a ragged last group whose choice flips if its phantom slots are counted; the second step of
                        every later band ("up" by the rule, something else if its far slots look into the band before)
    band_second_plane   the same groups on sparse-noise rows without the contest, for planes too large to steer
    extreme_planes      all zero, all 2^q - 1, the two alternations, the wrap
    rows_variant        the definition (no switch: ref_rows_plane exactly) or one WRONG rule of VARIANTS; numpy only, never compiled,
                        never run on a GPU

The conditions are proved with numpy alone in tests/test_rows_planes_host.py; tests/test_gpu_rows_planes.py runs every plane through
the device codec.  A helper module without tests."""
import functools

import numpy as np

from rows_ref import BAND, ref_constants, ref_fold

VARIANTS = {
    "tie_up": dict(tie_up=True),                   # a tie is "up"
    "slot0": dict(slot0=True),                     # slot 0 is counted in both costs (its left neighbour: 0)
    "tail": dict(tail=True),                       # the slots behind the plane's last sample are counted, as code 0
    "no_band": dict(no_band=True),                 # the reference ignores band restarts
    "w_plus_1": dict(off=1),                       # the reference is one sample off
    "w_minus_1": dict(off=-1),
    "far_as_near": dict(far_as_near=True),         # slots j < delta have a reference whenever the near group has one
    "no_far": dict(no_far=True),                   # slots j < delta are always 0
    "no_fold": dict(no_fold=True),                 # the residual is neither centred nor folded
}
TARGETS = (-1, 0, 1)                               # cost_up - cost_left of groups 0, 1, 2, 3, ... of a contest plane, in turn


def rows_costs(x, w, q, slot0=False, tail=False, no_band=False, off=0, far_as_near=False, no_far=False, no_fold=False):
    """One plane with K >= 1 -> (u of the 32 G slots as (G, 32), the codes likewise, cost_up, cost_left per group), under the
    definition or with rules changed."""
    x = np.asarray(x, dtype=np.int64)
    n, M = x.size, 1 << q
    G = (n + 31) // 32
    K, S = ref_constants(w)
    delta = w - 32 * K
    i = np.arange(32 * G)
    xp = np.zeros(32 * G, dtype=np.int64)
    xp[:n] = x
    at = i - (w + off)
    ok = at >= (0 if no_band else S * (i // S))
    j, local = i % 32, (i // 32) % (BAND * K)
    if far_as_near:
        ok |= (j < delta) & (local >= K) & (at >= 0)
    if no_far:
        ok &= j >= delta
    u = ((xp - np.where(ok, xp[np.maximum(at, 0)], 0)) % M).reshape(G, 32)
    xg = xp.reshape(G, 32)
    left = (xg - np.concatenate([np.zeros((G, 1), dtype=np.int64), xg[:, :-1]], axis=1)) % M
    counted = ((i < n) | tail) & ((j > 0) | slot0)
    price = (lambda e: e) if no_fold else (lambda e: ref_fold(e, q))
    cost = lambda e: (price(e) * counted.reshape(G, 32)).sum(axis=1)
    return u, xg, cost(u), cost(left)


def rows_variant(x, w, q, tie_up=False, **rule):
    """ref_rows_plane of tests/rows_ref.py with the rules of `rule` changed: -> (the difference plane's values, t per group)."""
    x = np.asarray(x, dtype=np.int64)
    u, xg, up, left = rows_costs(x, w, q, **rule)
    t = up <= left if tie_up else up < left
    real = (np.arange(xg.size) < x.size).reshape(xg.shape)
    v = np.cumsum(u * real, axis=1) % (1 << q)
    return np.where(t[:, None], v, xg).reshape(-1)[:x.size], t


def relations(x, w, q):
    """cost_up - cost_left per group, by the definition."""
    _, _, up, left = rows_costs(x, w, q)
    return up - left


# ---- content ----------------------------------------------------------------------------------------------------------------------
def sparse_plane(w, H, q, rng):
    """w x H codes: a row of noise, every other row the row above with one sample in twelve stepped by one."""
    rows = [rng.integers(0, 1 << q, w)]
    for _ in range(1, H):
        rows.append((rows[-1] + (rng.integers(0, 12, w) == 0)) % (1 << q))
    return np.concatenate(rows).astype(np.int64)


def band_second_groups(n, w):
    """The whole groups at band-local index K of the bands b >= 1 of a plane with delta >= 1."""
    K, _ = ref_constants(w)
    if K == 0 or w == 32 * K:
        return []
    return [g for g in range(BAND * K + K, n // 32, BAND * K)]


def _pin_band_second(x, w, g, frozen):
    """What group g's far and near reference groups must hold: a non-zero sample under slot delta - 1 (the last sample of the band
    before) and one under slot 31, so that the group is not constant."""
    for at in (32 * g + (w % 32) - 1 - w, 32 * g + 31 - w):
        x[at] = x[at] or 1
        frozen[at] = True


def _set_band_second(x, w, g, frozen):
    """Slots j >= delta copy their reference, slots j < delta are 0: u = 0 throughout and cost_left > 0, the group is "up" -- unless
    slots j < delta take x[i - w] from the band before (has_far for local >= K instead of local > K)."""
    delta = w % 32
    x[32 * g:32 * g + delta] = 0
    x[32 * g + delta:32 * g + 32] = x[32 * g + delta - w:32 * g + 32 - w]
    frozen[32 * g:32 * g + 32] = True


def band_second_plane(w, H, q, rng):
    """sparse_plane with the band-second groups set, in increasing order."""
    x = sparse_plane(w, H, q, rng)
    frozen = np.zeros(x.size, dtype=bool)
    for g in band_second_groups(x.size, w):
        _pin_band_second(x, w, g, frozen)
        _set_band_second(x, w, g, frozen)
    return x


# ---- the contest ------------------------------------------------------------------------------------------------------------------
def _steer(x, w, q, g, miss, frozen, rng, rounds, tries):
    """Change single free samples of group g, the best of `tries` at a time, until miss(d, codes) is 0: d = cost_up - cost_left of
    the group, priced on its own 32 slots."""
    n, M = x.size, 1 << q
    _, S = ref_constants(w)
    r = min(32, n - 32 * g)
    i = np.arange(32 * g, 32 * g + r)
    ref = np.where(i - w >= S * (i // S), x[np.maximum(i - w, 0)], 0)
    free = np.flatnonzero(~frozen[i])
    if free.size == 0:
        return

    def price(c):
        return ref_fold((c - ref) % M, q)[:, 1:].sum(axis=1) - ref_fold(c[:, 1:] - c[:, :-1], q).sum(axis=1)
    cur = x[i].copy()
    now = miss(price(cur[None]), cur[None])[0]
    for _ in range(rounds):
        if now == 0:
            break
        span = int(min(max(now, 3), max(M // 2, 1)))
        cand = np.tile(cur, (tries, 1))
        slot = free[rng.integers(0, free.size, tries)]
        step = rng.integers(1, span + 1, tries) * rng.choice((-1, 1), tries)
        cand[np.arange(tries), slot] = (cur[slot] + step) % M
        score = miss(price(cand), cand)
        best = int(np.argmin(score))
        if score[best] <= now:                     # equal: keep moving
            cur, now = cand[best], score[best]
    x[i] = cur


def contest_seconds(n, w):
    """band_second_groups without those that hold a reference of the ragged tail's phantom slots: those samples stay 0."""
    lo, hi = n - w, n - w + (32 - n % 32) % 32
    return [g for g in band_second_groups(n, w) if 32 * g + 32 <= lo or 32 * g >= hi]


def contest_plane(w, H, q, rng, rounds=48, tries=32):
    """-> the plane.  One forward pass: a change in a group touches its own costs and those of later groups only."""
    x = sparse_plane(w, H, q, rng)
    n, M = x.size, 1 << q
    K, S = ref_constants(w)
    if K == 0:
        return x
    frozen = np.zeros(n, dtype=bool)
    r = n % 32
    if r:
        # the references of the tail's phantom slots -- samples of earlier groups -- are 0: see below
        x[n - w:n - w + 32 - r] = 0
        frozen[n - w:n - w + 32 - r] = True
    seconds = contest_seconds(n, w)
    for g in seconds:
        _pin_band_second(x, w, g, frozen)
    for g in range((n + 31) // 32):
        if g in seconds:
            _set_band_second(x, w, g, frozen)
        elif r and g == n // 32:
            # the ragged tail.  Counted as code 0, its phantom slots add P = A - fold(0 - x_last) to d: A to cost_up, the folded
            # negatives of their references (0 unless a pinned sample is among them), and the step down from the last sample to
            # cost_left.  The last sample is set to 2^(q - 1), the steepest step down, then the other samples steer d to where
            # d < 0 and d + P < 0 differ.  A tail of one sample has d = 0 whatever it holds, and flips because A is 0
            i = np.arange(n, n - r + 32)
            A = int(ref_fold(-np.where(i - w >= S * (i // S), x[i - w], 0), q).sum())
            x[-1] = M // 2 if A != M - 1 else 0
            frozen[-1] = True
            P = A - int(ref_fold(-x[-1:], q)[0])
            lo, hi = (-P, -1) if P > 0 else (0, -P - 1)
            _steer(x, w, q, g, lambda d, c: np.maximum(0, lo - d) + np.maximum(0, d - hi), frozen, rng, rounds, tries)
        else:
            _steer(x, w, q, g, lambda d, c, want=TARGETS[g % 3]: np.abs(d - want), frozen, rng, rounds, tries)
    return x


# ---- extremes ---------------------------------------------------------------------------------------------------------------------
def extreme_planes(w, H, q):
    """name -> plane.  `alternating` is 0 and 2^q - 1 in turn, residuals of +-1 that wrap; `steepest` is 0 and 2^(q - 1) in turn, the
    largest cost there is: 31 folded maxima of 2^q - 1 per group (at q = 1 the two are the same plane); `wrap` has 2^q - 1 above 0."""
    n, top = w * H, (1 << q) - 1
    row = np.where(np.arange(w) % 2 == 0, top, top // 2)
    return {
        "zero": np.zeros(n, dtype=np.int64),
        "full": np.full(n, top, dtype=np.int64),
        "alternating": (np.arange(n) % 2 * top).astype(np.int64),
        "steepest": (np.arange(n) % 2 << (q - 1)).astype(np.int64),
        "wrap": np.concatenate([(row + k % 2) % (top + 1) for k in range(H)]).astype(np.int64),
    }


# ---- the set ----------------------------------------------------------------------------------------------------------------------
HEIGHT = 19                                        # (32 + delta) x 19: K = 1, two or three bands, a ragged tail wherever delta != 0
NAMES = ("contest", "zero", "full", "alternating", "steepest", "wrap")


@functools.lru_cache(maxsize=None)
def built_planes(q, seed=23900):
    """delta -> name -> the (32 + delta) x HEIGHT plane of q-bit codes, delta = 0 .. 31: from one seed, built once per process."""
    rng = np.random.default_rng(seed + q)
    return {delta: dict(extreme_planes(32 + delta, HEIGHT, q), contest=contest_plane(32 + delta, HEIGHT, q, rng)) for delta in range(32)}


def plan_bits(q):
    """The bit widths of the plan that has q in its Y plane: mixed triples, and every q in each of the three planes once."""
    return (q, q % 8 + 1, (q + 1) % 8 + 1)


def built_frames(q, delta):
    """-> (bits, the frames of NAMES): three planes each, of the sets of the three bit widths of plan_bits(q)."""
    bits = plan_bits(q)
    return bits, [[built_planes(b)[delta][name] for b in bits] for name in NAMES]
