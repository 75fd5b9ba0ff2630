// csic_rans_decode.h -- what the decoder of the rANS coding (include/csic.h: CSIC_CODING_RANS) does with the bits of one chunk: the
// constants of the coder, the clamp of a chunk's extent, the 16-bit word read, the packed (f, cum) entry of a symbol and the decode
// step of one stream.  Plain C++ over a segment of `ndwords` dwords, __host__ __device__: k_rans_unpack (csic_rans.hip) runs it on a
// chunk in LDS, csic_rans_unpack_host on the bytes of a coded frame, tests/cpp/rans_fuzz.cpp on exactly-sized heap blocks of random
// bytes under the sanitizers.  Nothing here trusts the bits: a word behind the segment reads as 0, a table entry is clamped so that no
// slot index leaves the 4096 slots, and a chunk's extent is clamped to the frame and to the block's raw size before anything is read.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define CSIC_RANS_HD __host__ __device__ inline
#else
#define CSIC_RANS_HD inline
#endif

namespace csic {

constexpr uint32_t RANS_SCALE_BITS = 12, RANS_M = 1u << RANS_SCALE_BITS;      // frequencies sum to M
constexpr uint32_t RANS_L = 1u << 16;                                         // the lower bound of a state; words are 16 bits
constexpr uint32_t RANS_LANES = 64, RANS_ROUNDS = 16;                         // streams per block, groups per stream
constexpr uint32_t RANS_BLOCK = RANS_LANES * RANS_ROUNDS;                     // groups per block: 1024
constexpr uint32_t RANS_RAW_FLAG = 0x80000000u;                               // bit 31 of a directory entry

// the dwords of the raw chunk of a block of `ng` groups at q bits per code
CSIC_RANS_HD uint32_t rans_raw_dwords(uint32_t ng, uint32_t q) { return (ng * 31u * q + 31u) / 32u; }

// The extent of a block's chunk as the device decoder takes it, from the two directory entries as stored: the offsets clamped to
// max_dwords (no payload dword of a frame lies behind) and to each other, the length to the block's raw size.
CSIC_RANS_HD void rans_chunk_extent(uint32_t e0, uint32_t e1, uint32_t max_dwords, uint32_t raw_dwords, uint32_t *d0, uint32_t *ndwords, bool *raw)
{
    const uint32_t a = (e0 & ~RANS_RAW_FLAG) < max_dwords ? (e0 & ~RANS_RAW_FLAG) : max_dwords;
    uint32_t b = (e1 & ~RANS_RAW_FLAG) < max_dwords ? (e1 & ~RANS_RAW_FLAG) : max_dwords;
    if (b < a) b = a;
    *d0 = a;
    *ndwords = b - a < raw_dwords ? b - a : raw_dwords;
    *raw = (e0 & RANS_RAW_FLAG) != 0;
}

CSIC_RANS_HD uint32_t rans_dword(const uint32_t *seg, uint32_t ndwords, uint32_t i) { return i < ndwords ? seg[i] : 0u; }

// 16-bit word number i of the segment (word 2 k is the low half of dword k); 0 behind the segment
CSIC_RANS_HD uint32_t rans_word(const uint32_t *seg, uint32_t ndwords, uint32_t i) { return (rans_dword(seg, ndwords, i >> 1) >> (16u * (i & 1u))) & 0xFFFFu; }

// the q bits at [bit, bit + q) of the segment, q <= 8 (a raw chunk's u_j)
CSIC_RANS_HD uint32_t rans_raw_bits(const uint32_t *seg, uint32_t ndwords, uint32_t bit, uint32_t q)
{
    const uint32_t wi = bit >> 5, sh = bit & 31u;
    uint32_t v = rans_dword(seg, ndwords, wi) >> sh;
    if (sh + q > 32u) v |= rans_dword(seg, ndwords, wi + 1u) << (32u - sh);
    return v & ((1u << q) - 1u);
}

// A symbol's table entry: f in bits 0 .. 15, cum in bits 16 .. 31 -- as the decoder takes them, cum <= M and cum + f <= M, whatever the
// stored table says.
CSIC_RANS_HD uint32_t rans_entry(uint32_t f, uint32_t cum)
{
    if (cum > RANS_M) cum = RANS_M;
    if (f > RANS_M - cum) f = RANS_M - cum;
    return f | (cum << 16);
}

// One decode step of a stream in state *x: returns the symbol of the state's slot, advances the state and says whether the stream takes
// a word now.  slot2sym has M entries, entry[] one per symbol.
CSIC_RANS_HD uint32_t rans_decode_step(uint32_t *x, const uint8_t *slot2sym, const uint32_t *entry, bool *refill)
{
    const uint32_t slot = *x & (RANS_M - 1u), s = slot2sym[slot], e = entry[s];
    *x = (e & 0xFFFFu) * (*x >> RANS_SCALE_BITS) + slot - (e >> 16);
    *refill = *x < RANS_L;
    return s;
}
CSIC_RANS_HD void rans_refill(uint32_t *x, uint32_t word) { *x = (*x << 16) | word; }

} // namespace csic
