"""Code planes built to order for the rANS coding (csic_rans_*), in the style of tests/codec_planes.py: each builder returns (q, codes) of
one plane whose folded residuals meet a stated condition of the format -- a table with one entry, the negative-remainder path of the
scaling rule, a raw block among rANS blocks, a word taken at the first or at the latest possible step.  The conditions are proved with
the numpy statement alone in tests/test_rans_planes_host.py; tests/test_gpu_rans.py runs every plane through the device codec."""
import numpy as np

from test_rans_host import BLOCK, LANES


def codes_of_u(u, q, anchors=None):
    """(G, 32) folded residuals (slot 0 ignored) and the groups' anchors (default: g mod 2^q) -> the plane's 32 G codes."""
    u = np.asarray(u, dtype=np.int64)
    e = np.where(u % 2 == 0, u // 2, -(u + 1) // 2)
    e[:, 0] = np.arange(u.shape[0]) if anchors is None else anchors
    return (np.cumsum(e, axis=1) % (1 << q)).reshape(-1)


def constant_plane(q=5, groups=70, tail=9):
    """Every residual 0: one f_s = M, every symbol codes in zero bits.  The last group is ragged."""
    return q, np.full(32 * groups - tail, (1 << q) - 2, dtype=np.int64)


def two_symbol_plane(rng, q=3, groups=1100):
    """Residuals 0 and 2 only (a code steps up by one with probability 0.2): a table of two entries, more than one block."""
    u = np.where(rng.random((groups, 32)) < 0.2, 2 if q > 1 else 1, 0)
    return q, codes_of_u(u, q)


def skewed_plane(rng, first=()):
    """q = 8, 1024 groups: residual 0 everywhere but 250 slots that hold the values 1 .. 250 once each.  Their floors are 0 and are
    lifted to 1, the sum overshoots M by more than 100 and the excess comes off the dominant f_0.  `first`: the (group, slot) of the
    values 1, 2, ... in turn; the rest go to random slots."""
    u = np.zeros((BLOCK, 32), dtype=np.int64)
    spots = list(first)
    taken = set(spots)
    while len(spots) < 250:
        s = (int(rng.integers(0, BLOCK)), int(rng.integers(1, 32)))
        if s not in taken:
            taken.add(s)
            spots.append(s)
    for v, (g, j) in enumerate(spots, start=1):
        u[g, j] = v
    return 8, codes_of_u(u, 8)


def late_word_plane(rng, lane=5):
    """skewed_plane with two once-seen values in the last two slots of a stream's last group: the encoder codes f = 1 from x = L, stands
    at 2^28 and emits before the next symbol -- the decoder takes that word at step 494, the latest step at which any stream can."""
    return skewed_plane(rng, first=[(LANES * 15 + lane, 31), (LANES * 15 + lane, 30)])


def early_word_plane(rng, lane=7):
    """skewed_plane with a once-seen value in slot 1 of a stream's first group: the last symbol the encoder codes, the word the decoder
    takes at step 0."""
    return skewed_plane(rng, first=[(lane, 1)])


def noise_block_plane(rng, q=4, blocks=3, noisy=1):
    """Zeros with exactly one block of uniform noise: the table is dominated by 0, a noise symbol costs more than q bits."""
    codes = np.zeros(32 * BLOCK * blocks, dtype=np.int64)
    codes[32 * BLOCK * noisy:32 * BLOCK * (noisy + 1)] = rng.integers(0, 1 << q, 32 * BLOCK)
    return q, codes


def noise_plane(rng, q=6, groups=BLOCK + 40):
    """Uniform noise: every block is raw."""
    return q, rng.integers(0, 1 << q, 32 * groups - 3).astype(np.int64)


def built_planes(seed=21700):
    """name -> (q, codes): every plane above, from one seed."""
    rng = np.random.default_rng(seed)
    return {
        "constant": constant_plane(),
        "two_symbols": two_symbol_plane(rng),
        "one_bit": two_symbol_plane(rng, q=1, groups=200),
        "skewed": skewed_plane(rng),
        "late_word": late_word_plane(rng),
        "early_word": early_word_plane(rng),
        "noise_block": noise_block_plane(rng),
        "noise": noise_plane(rng),
    }
