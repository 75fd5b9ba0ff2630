// csic_rice_decode.h -- what the decoder of the Rice coding (include/csic.h: CSIC_CODING_RICE) does with the bits of one chunk: the
// terminator select that finds a group's unary run, and the per-slot read of a folded residual.  Plain C++ over a segment of `nwords`
// dwords, __host__ __device__: k_rice_unpack (csic_rice.hip) runs it on a chunk in LDS, csic_rice_unpack_host on the bytes of a coded
// frame, tests/cpp/rice_fuzz.cpp on exactly-sized heap blocks of random bytes under the sanitizers.  Nothing here trusts the bits: every
// word index is compared with nwords first (a word behind the segment reads as 0), a unary run ends at `uend` at the latest, and every
// loop is bounded by the segment's length.  rice_unfold, the inverse of the fold of a residual, is the one definition for both codings:
// the group coding's codecs (csic_pack.hip, csic_pack_host.cpp) call it as well; rice_fold is the host codecs' one statement of the fold
// (csic_group_host.h's load_group, csic_temporal_host.h's group_cost).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define CSIC_RICE_HD __host__ __device__ inline
#else
#define CSIC_RICE_HD inline
#endif

namespace csic {

CSIC_RICE_HD uint32_t rice_word(const uint32_t *seg, uint32_t nwords, uint32_t i) { return i < nwords ? seg[i] : 0u; }

// the n <= 8 bits at [bit, bit + n) of the segment
CSIC_RICE_HD uint32_t rice_bits(const uint32_t *seg, uint32_t nwords, uint32_t bit, uint32_t n)
{
    const uint32_t wi = bit >> 5, sh = bit & 31u;
    uint32_t v = rice_word(seg, nwords, wi) >> sh;
    if (sh + n > 32u) v |= rice_word(seg, nwords, wi + 1u) << (32u - sh);
    return v & ((1u << n) - 1u);
}

// the position of set bit number r (0 = the lowest) of w; 32 when w has no more than r set bits
CSIC_RICE_HD uint32_t rice_select32(uint32_t w, uint32_t r)
{
    uint32_t pos = 0;
    for (uint32_t s = 16; s >= 1u; s >>= 1) {
        const uint32_t lo = w & ((1u << s) - 1u), c = (uint32_t)__builtin_popcount(lo);
        if (r >= c) { r -= c; w >>= s; pos += s; } else w = lo;
    }
    return (w & 1u) && r == 0 ? pos : 32u;
}

// cum[i] = the number of set bits in words 0 .. i of a bit string of n words (non-decreasing).  Returns the bit position right behind
// set bit number t (1 = the first; t = 0: position 0), 32 n when the string has fewer than t set bits.
CSIC_RICE_HD uint32_t rice_after_terminator(const uint32_t *words, const uint32_t *cum, uint32_t n, uint32_t t)
{
    if (t == 0) return 0;
    uint32_t lo = 0, hi = n;                           // the smallest i with cum[i] >= t, n when there is none
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (cum[mid] >= t) hi = mid; else lo = mid + 1u;
    }
    if (lo >= n) return 32u * n;
    const uint32_t before = lo ? cum[lo - 1u] : 0u;
    if (before >= t) return 32u * n;                   // (cum not monotonic: cannot happen with real counts)
    const uint32_t pos = rice_select32(words[lo], t - 1u - before);
    return pos >= 32u ? 32u * n : 32u * lo + pos + 1u;
}

// One unary number at bit *ubit of the segment: the zero bits up to the next one bit, which is consumed.  The run ends at bit `uend`
// (<= 32 nwords is enforced here) at the latest: then *terminated is false and *ubit = the end.
CSIC_RICE_HD uint32_t rice_unary(const uint32_t *seg, uint32_t nwords, uint32_t *ubit, uint32_t uend, bool *terminated)
{
    if (uend > 32u * nwords) uend = 32u * nwords;
    uint32_t at = *ubit, zeros = 0;
    *terminated = false;
    while (at < uend) {
        const uint32_t sh = at & 31u, room = 32u - sh, avail = uend - at < room ? uend - at : room;
        uint32_t w = seg[at >> 5] >> sh;               // (at < uend <= 32 nwords)
        if (avail < 32u) w &= (1u << avail) - 1u;
        if (w) {
            const uint32_t tz = (uint32_t)__builtin_ctz(w);
            *ubit = at + tz + 1u;
            *terminated = true;
            return zeros + tz;
        }
        zeros += avail;
        at += avail;
    }
    *ubit = at;
    return zeros;
}

// Slot j >= 1 of a group that is not in zero mode: u_j = (zeros << k) | remainder, masked to q bits.  k = min(mode, q); a group with
// k = q (raw) has no unary part.  *rbit and *ubit step on to the next slot.
CSIC_RICE_HD uint32_t rice_next_u(const uint32_t *seg, uint32_t nwords, uint32_t *rbit, uint32_t *ubit, uint32_t uend, uint32_t k, uint32_t q)
{
    uint32_t u = k ? rice_bits(seg, nwords, *rbit, k) : 0u;
    *rbit += k;
    if (k < q) {
        bool terminated;
        const uint32_t zeros = rice_unary(seg, nwords, ubit, uend, &terminated);
        u |= (zeros < 256u ? zeros : 255u) << k;
    }
    return u & ((1u << q) - 1u);
}

// a difference e to the code before, modulo mask + 1 -> its folded, centred residual u (the host codecs' one statement of the fold)
CSIC_RICE_HD uint32_t rice_fold(uint32_t e, uint32_t mask) { return e <= (mask >> 1) ? 2u * e : 2u * (mask + 1u - e) - 1u; }
// a folded residual u -> e, the inverse
CSIC_RICE_HD uint32_t rice_unfold(uint32_t u, uint32_t mask) { return ((u & 1u) ? ~(u >> 1) : (u >> 1)) & mask; }

} // namespace csic
