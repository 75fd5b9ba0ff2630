// rans_fuzz.cpp -- the host codec of the rANS coding (csic_rans_pack_host / csic_rans_unpack_host, csrc/csic_rans_host.cpp) and the
// decode step, word reads and clamps the device decoder shares with it (csrc/csic_rans_decode.h) under ASan + UBSan:
//   1. random frames packed and unpacked, then about 10 000 mutated coded frames -- bit flips, truncations, extensions, table entries,
//      directory entries, random bytes -- fed to csic_rans_unpack_host from heap blocks of exactly their length: CSIC_OK with a frame
//      that packs again and decodes to itself, or CSIC_EFORMAT with the destination untouched;
//   2. every one of those byte strings, valid or not, through device_unpack below: the flow of k_rans_unpack (csrc/csic_rans.hip) line
//      by line -- the clamp of the chunk's extent, the clamped table entries, the slot table, the 496 steps with the words taken in
//      lane order, the raw reads -- on a chunk, an entry table and a slot table that live in heap blocks of exactly their sizes (what
//      the kernel holds in LDS), the coded frame in a block of exactly bound_bytes.  On a valid frame it must give the source back; on
//      any bytes it must stay inside its blocks and give codes below 2^q.
// Built and run by tests/test_cpp_rans.py; no GPU, nothing of the HIP library.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csic.h"
#include "csic_rans_decode.h"
#include "csic_rice_decode.h"

using namespace csic;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, csic_last_error()); return 1; } } while (0)

struct Planes { int64_t off[3], bytes[3], n[3]; int q[3]; };

// a frame buffer whose payload ranges hold valid codes (the unused high bits of a plane's last byte 0), 0xEE elsewhere
static void fill_frame(std::vector<unsigned char> &f, const Planes &P, int kind)
{
    std::memset(f.data(), 0xEE, f.size());
    for (int p = 0; p < 3; ++p) {
        unsigned char *d = f.data() + P.off[p];
        std::memset(d, 0, (size_t)P.bytes[p]);
        uint32_t c = rnd();
        for (int64_t i = 0; i < P.n[p]; ++i) {
            if (kind == 0) c = rnd();                                  // noise: raw chunks
            else if (kind == 1) c += (rnd() % 8 == 0);                 // slow ramp
            else if (kind == 2) c += (rnd() % 3) - 1;                  // small steps both ways
            else if (kind == 4) c = (i / 4096) % 3 == 1 ? rnd() : c + (rnd() % 16 == 0);     // a stretch of noise in between: both kinds of chunk
            const uint32_t v = c & ((1u << P.q[p]) - 1u);              // kind 3: constant
            const int64_t bit = i * P.q[p];
            const uint32_t s = v << (bit & 7);
            d[bit >> 3] |= (unsigned char)s;
            if (s >> 8) d[(bit >> 3) + 1] |= (unsigned char)(s >> 8);
        }
    }
}

static uint32_t ld4(const unsigned char *coded, int64_t bound, int64_t off)      // pk_coded_ld4 with its CSIC_DEBUG check always on
{
    if (off < 0 || off + 4 > bound) { std::printf("FAILED: a coded dword at %lld of %lld bytes\n", (long long)off, (long long)bound); std::abort(); }
    return (uint32_t)coded[off] | ((uint32_t)coded[off + 1] << 8) | ((uint32_t)coded[off + 2] << 16) | ((uint32_t)coded[off + 3] << 24);
}

// k_rans_unpack on the host: `coded` is a block of exactly L.bound_bytes, `frame` a frame buffer; only the payload ranges are written
static void device_unpack(const Planes &P, const csic_rans_layout &L, const unsigned char *coded, unsigned char *frame)
{
    const int64_t bound = L.bound_bytes;
    const uint32_t max_dwords = (uint32_t)((L.bound_bytes - L.payload_offset) / 4);
    int64_t blk = 0;
    for (int p = 0; p < 3; ++p) {
        const uint32_t Q = (uint32_t)P.q[p], MASK = (1u << Q) - 1u, NSYM = 1u << Q, G = (uint32_t)L.groups[p], n = (uint32_t)P.n[p];
        unsigned char *dst = frame + P.off[p];
        std::memset(dst, 0, (size_t)P.bytes[p]);
        for (uint32_t g0 = 0; g0 < G; g0 += RANS_BLOCK, ++blk) {
            const uint32_t ng = std::min(G - g0, RANS_BLOCK), ns = std::min(ng, RANS_LANES);
            uint32_t d0, nw;
            bool raw;
            rans_chunk_extent(ld4(coded, bound, L.directory_offset + 4 * blk), ld4(coded, bound, L.directory_offset + 4 * blk + 4), max_dwords,
                              rans_raw_dwords(ng, Q), &d0, &nw, &raw);
            uint32_t *chunk = (uint32_t *)std::malloc(nw ? 4 * (size_t)nw : 1);            // s_chunk: exactly the dwords the kernel fills
            for (uint32_t i = 0; i < nw; ++i) chunk[i] = ld4(coded, bound, L.payload_offset + 4 * ((int64_t)d0 + i));
            uint32_t *entry = (uint32_t *)std::malloc(4 * (size_t)NSYM);                   // s_e
            uint8_t *slots = (uint8_t *)std::calloc(RANS_M, 1);                            // s_slots
            for (uint32_t s = 0, cum = 0; s < NSYM; ++s) {                                 // rn_load_entries: the table's dwords, a running sum
                const uint32_t f = (ld4(coded, bound, L.tables_offset[p] + 4 * (int64_t)(s >> 1)) >> (16u * (s & 1u))) & 0xFFFFu;
                entry[s] = rans_entry(f, cum);
                cum += f;
            }
            if (!raw)
                for (uint32_t s = 0; s < NSYM; ++s)
                    for (uint32_t k = 0; k < (entry[s] & 0xFFFFu); ++k) {
                        if ((entry[s] >> 16) + k >= RANS_M) { std::printf("FAILED: a slot outside the table\n"); std::abort(); }
                        slots[(entry[s] >> 16) + k] = (uint8_t)s;
                    }
            uint32_t x[RANS_LANES], next = 0;
            for (uint32_t l = 0; l < RANS_LANES; ++l) x[l] = rans_dword(chunk, nw, l);
            const uint32_t segdw = nw > ns ? nw - ns : 0u;
            const uint32_t *seg = chunk + (nw > ns ? ns : nw);                              // (never read when segdw is 0)
            std::vector<uint8_t> u((size_t)ng * 32, 0);
            for (uint32_t t = 0; t < 31u * RANS_ROUNDS; ++t) {
                const uint32_t i = t / 31u, j = 1u + t % 31u;
                if (RANS_LANES * i >= ng) break;
                uint32_t taken = 0;
                for (uint32_t l = 0; l < RANS_LANES && RANS_LANES * i + l < ng; ++l) {
                    const uint32_t gl = RANS_LANES * i + l;
                    uint32_t s;
                    if (raw) s = rans_raw_bits(chunk, nw, (gl * 31u + j - 1u) * Q, Q);
                    else {
                        bool refill;
                        s = rans_decode_step(&x[l], slots, entry, &refill) & MASK;
                        if (s >= NSYM) { std::printf("FAILED: a symbol outside the table\n"); std::abort(); }
                        if (refill) rans_refill(&x[l], rans_word(seg, segdw, next + taken++));      // ascending lane order
                    }
                    u[(size_t)gl * 32 + j] = (uint8_t)s;
                }
                next += taken;
            }
            for (uint32_t gl = 0; gl < ng; ++gl) {
                const uint32_t g = g0 + gl;
                const int64_t abit = (int64_t)g * Q, aat = L.anchors_offset[p] + 4 * (abit >> 5);
                const uint32_t as = (uint32_t)(abit & 31);
                uint32_t c = ld4(coded, bound, aat) >> as;
                if (as + Q > 32u) c |= ld4(coded, bound, aat + 4) << (32u - as);
                c &= MASK;
                for (uint32_t j = 0; j < 32; ++j) {
                    if (j > 0) c = (c + rice_unfold(u[(size_t)gl * 32 + j], MASK)) & MASK;
                    if (32u * g + j < n) {
                        const int64_t bit = ((int64_t)32 * g + j) * Q;
                        const uint32_t s = c << (bit & 7);
                        dst[bit >> 3] |= (unsigned char)s;
                        if (s >> 8) dst[(bit >> 3) + 1] |= (unsigned char)(s >> 8);
                    }
                }
            }
            std::free(slots);
            std::free(entry);
            std::free(chunk);
        }
    }
}

int main()
{
    static const int perms[6][3] = {{1, 2, 3}, {1, 3, 2}, {2, 1, 3}, {2, 3, 1}, {3, 1, 2}, {3, 2, 1}};
    static const int ab[6][2] = {{4, 4}, {2, 2}, {2, 0}, {1, 1}, {4, 0}, {1, 0}};
    long mutated = 0, accepted = 0, refused = 0, raw_blocks = 0, rans_blocks = 0;
    for (int it = 0; it < 60; ++it) {
        csic_params p;
        const bool wide = it % 6 == 5;                                 // every sixth frame has more than one block per plane
        REQUIRE(csic_params_default(&p, wide ? 32768 + (int)(rnd() % 3000) : 1 + (int)(rnd() % 80), wide ? 1 + (int)(rnd() % 3) : 1 + (int)(rnd() % 24)) == CSIC_OK);
        const int k = wide ? 0 : (int)(rnd() % 6);
        p.chroma_a = ab[k][0]; p.chroma_b = ab[k][1];
        p.y_bits = 1 + (int)(rnd() % 8); p.cb_bits = 1 + (int)(rnd() % 8); p.cr_bits = 1 + (int)(rnd() % 8);
        p.factor = wide ? 1 : 1 << (rnd() % 4);
        std::memcpy(p.op, perms[rnd() % 6], sizeof p.op);
        p.out_format = (int)(rnd() % 4);                               // ignored
        csic_planar_bits_layout B;
        csic_rans_layout L;
        REQUIRE(csic_planar_bits_layout_of(&p, &B) == CSIC_OK && csic_rans_layout_of(&p, &L) == CSIC_OK);
        Planes P = {{B.y_offset, B.cb_offset, B.cr_offset}, {B.y_bytes, B.cb_bytes, B.cr_bytes},
                    {(int64_t)B.geometry.y_width * B.geometry.y_height, B.geometry.chroma_samples, B.geometry.chroma_samples},
                    {p.y_bits, p.cb_bits, p.cr_bits}};
        int64_t top = L.fixed_bytes, nb = 0;
        for (int pl = 0; pl < 3; ++pl) {
            REQUIRE(L.groups[pl] == (P.n[pl] + 31) / 32 && L.blocks[pl] == (L.groups[pl] + 1023) / 1024);
            for (int64_t b = 0; b < L.blocks[pl]; ++b) top += 4 * (int64_t)rans_raw_dwords((uint32_t)std::min<int64_t>(1024, L.groups[pl] - 1024 * b), (uint32_t)P.q[pl]);
            nb += L.blocks[pl];
        }
        REQUIRE(L.bound_bytes >= top && L.bound_bytes < top + 256 && L.bound_bytes % 256 == 0 && L.payload_offset == L.fixed_bytes);
        REQUIRE(L.payload_offset == L.directory_offset + 4 * (nb + 1));

        std::vector<unsigned char> frame((size_t)B.frame_bytes), back((size_t)B.frame_bytes), again((size_t)B.frame_bytes);
        std::vector<unsigned char> coded((size_t)L.bound_bytes), recoded((size_t)L.bound_bytes);
        fill_frame(frame, P, it % 5);
        uint64_t size = 0;
        REQUIRE(csic_rans_pack_host(&p, frame.data(), coded.data(), coded.size(), &size) == CSIC_OK);
        REQUIRE((int64_t)size >= L.fixed_bytes && (int64_t)size <= top && size % 4 == 0);
        for (int64_t b = 0; b < nb; ++b) (ld4(coded.data(), L.bound_bytes, L.directory_offset + 4 * b) & RANS_RAW_FLAG ? raw_blocks : rans_blocks) += 1;
        unsigned char *dev = (unsigned char *)std::malloc((size_t)L.bound_bytes);          // what the device reads: exactly bound_bytes
        {
            // exact-size blocks on both sides: the sanitizer sees any access past either
            unsigned char *src = (unsigned char *)std::malloc(size ? size : 1), *dst = (unsigned char *)std::malloc(frame.size());
            std::memcpy(src, coded.data(), size);
            std::memset(dst, 0xEE, frame.size());
            REQUIRE(csic_rans_unpack_host(&p, src, size, dst) == CSIC_OK);
            REQUIRE(std::memcmp(dst, frame.data(), frame.size()) == 0);   // the payload ranges restored, the canary around them kept
            // the device's flow on the same bytes, garbage behind coded_bytes
            for (int64_t i = 0; i < L.bound_bytes; ++i) dev[i] = i < (int64_t)size ? coded[i] : (unsigned char)rnd();
            std::memset(dst, 0xEE, frame.size());
            device_unpack(P, L, dev, dst);
            REQUIRE(std::memcmp(dst, frame.data(), frame.size()) == 0);
            std::free(src); std::free(dst);
        }
        REQUIRE(csic_rans_pack_host(&p, frame.data(), recoded.data(), (size_t)size, &size) == CSIC_OK);     // capacity = exactly the size
        if (size > (uint64_t)L.fixed_bytes) {
            uint64_t need = 0;
            REQUIRE(csic_rans_pack_host(&p, frame.data(), recoded.data(), (size_t)size - 4, &need) == CSIC_EINVAL_SIZE && need == size);
        }

        for (int m = 0; m < (wide ? 30 : 200); ++m) {
            size_t len = (size_t)size;
            const int how = (int)(rnd() % 8);
            if (how == 1) len = rnd() % (size + 1);                                       // truncated anywhere
            else if (how == 2) len = (size_t)size + 4 * (1 + rnd() % 3);                  // extended
            else if (how == 5) len = 4 * (rnd() % (size_t)(top / 4 + 2));                 // any length in dwords
            len = std::min(len, (size_t)L.bound_bytes);
            unsigned char *src = (unsigned char *)std::malloc(len ? len : 1);
            for (size_t i = 0; i < len; ++i) src[i] = i < size ? coded[i] : (unsigned char)rnd();
            if (how == 0 && len)                                                           // 1 .. 3 bit flips
                for (int b = 1 + (int)(rnd() % 3); b > 0; --b) src[rnd() % len] ^= (unsigned char)(1u << (rnd() % 8));
            if (how == 3 && len) {                                                         // a table: one frequency moved to a neighbour (the sum stays), or anything
                const int pl = (int)(rnd() % 3);
                const size_t at = (size_t)L.tables_offset[pl] + 2 * (rnd() % (size_t)(1 << P.q[pl]));
                if ((at | 2) + 2 <= len) { if (rnd() & 1) { src[at] += 1; src[at ^ 2] -= 1; } else { src[at] = (unsigned char)rnd(); src[at + 1] = (unsigned char)rnd(); } }
            }
            if (how == 4) for (size_t i = 0; i < len; ++i) if (rnd() % 16 == 0) src[i] = (unsigned char)rnd();     // bytes at random
            if (how == 6) {                                                                // a directory entry: a little off, its flag, or anything
                const size_t at = (size_t)L.directory_offset + 4 * (rnd() % (size_t)(nb + 1));
                const int what = (int)(rnd() % 3);
                if (at + 4 <= len) { if (what == 0) src[at] += (unsigned char)(1 + rnd() % 3); else if (what == 1) src[at + 3] ^= 0x80; else for (int b = 0; b < 4; ++b) src[at + b] = (unsigned char)rnd(); }
            }
            if (how == 7 && len > (size_t)L.payload_offset)                                // bit flips in the payload
                for (int b = 1 + (int)(rnd() % 3); b > 0; --b) src[(size_t)L.payload_offset + rnd() % (len - (size_t)L.payload_offset)] ^= (unsigned char)(1u << (rnd() % 8));
            std::memset(back.data(), 0xEE, back.size());
            const int st = csic_rans_unpack_host(&p, src, len, back.data());
            ++mutated;
            if (st == CSIC_EFORMAT) {
                ++refused;
                for (size_t i = 0; i < back.size(); ++i) REQUIRE(back[i] == 0xEE);        // a refused frame writes nothing
            } else {
                REQUIRE(st == CSIC_OK);
                ++accepted;
                // re-packable: a valid frame that packs within the bound and decodes to itself; outside the payload ranges untouched
                uint64_t rsize = 0;
                REQUIRE(csic_rans_pack_host(&p, back.data(), recoded.data(), recoded.size(), &rsize) == CSIC_OK && (int64_t)rsize <= top);
                std::memset(again.data(), 0xEE, again.size());
                REQUIRE(csic_rans_unpack_host(&p, recoded.data(), (size_t)rsize, again.data()) == CSIC_OK);
                REQUIRE(std::memcmp(again.data(), back.data(), back.size()) == 0);
                for (int pl = 0; pl < 3; ++pl) {
                    const int used = (int)((P.n[pl] * P.q[pl]) % 8);
                    if (used) REQUIRE((back[(size_t)(P.off[pl] + P.bytes[pl] - 1)] >> used) == 0);
                }
            }
            // the device's flow on the same bytes, whatever the host said: inside its blocks, and equal to the host on what the host accepts
            for (int64_t i = 0; i < L.bound_bytes; ++i) dev[i] = i < (int64_t)len ? src[i] : (unsigned char)rnd();
            std::memset(again.data(), 0xEE, again.size());
            device_unpack(P, L, dev, again.data());
            if (st == CSIC_OK) REQUIRE(std::memcmp(again.data(), back.data(), back.size()) == 0);
            std::free(src);
        }
        // nothing but random bytes
        for (int64_t i = 0; i < L.bound_bytes; ++i) dev[i] = (unsigned char)rnd();
        device_unpack(P, L, dev, again.data());
        std::free(dev);
    }
    REQUIRE(csic_rans_unpack_host(nullptr, "", 0, &mutated) == CSIC_EINVAL_NULL);
    REQUIRE(mutated >= 9000 && accepted > 100 && refused > 1000 && raw_blocks > 10 && rans_blocks > 10);
    std::printf("rans fuzz ok: %ld mutated frames, %ld accepted, %ld refused; %ld rANS and %ld raw blocks\n", mutated, accepted, refused, rans_blocks, raw_blocks);
    return 0;
}
