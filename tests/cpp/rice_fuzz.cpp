// rice_fuzz.cpp -- the host codec of the Rice coding (csic_rice_pack_host / csic_rice_unpack_host, csrc/csic_rice_host.cpp) and the bit
// reads the device decoder shares with it (csrc/csic_rice_decode.h) under ASan + UBSan:
//   1. random frames packed and unpacked, then about 20 000 mutated coded frames -- bit flips, truncations, extensions, bad nibbles,
//      directory entries, random bytes -- fed to csic_rice_unpack_host from heap blocks of exactly their length: CSIC_OK with a frame
//      that packs again and decodes to itself, or CSIC_EFORMAT with the destination untouched;
//   2. every one of those byte strings, valid or not, through device_unpack below: the flow of k_rice_unpack (csrc/csic_rice.hip) line
//      by line -- the clamps of the directory and the chunk, the two scans, the terminator select, 31 slots per group -- on a chunk and
//      a count array that live in heap blocks of exactly nw and uw dwords (what the kernel holds in LDS), the coded frame in a block of
//      exactly bound_bytes.  On a valid frame it must give the source back; on any bytes it must stay inside its blocks and give codes
//      below 2^q;
//   3. rice_select32, rice_after_terminator and rice_unary on random words against bit-by-bit loops.
// Built and run by tests/test_cpp_rice.py; no GPU, nothing of the HIP library.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csic.h"
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
            if (kind == 0) c = rnd();                                  // noise
            else if (kind == 1) c += (rnd() % 8 == 0);                 // slow ramp
            else if (kind == 2) c += (rnd() % 3) - 1;                  // small steps both ways
            else if (kind == 4) c = (i / 32) % 3 == 0 ? c : (i / 32) % 3 == 1 ? rnd() : c + (rnd() % 5) - 2;     // zero, raw and Rice groups in turn
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

// k_rice_unpack on the host: `coded` is a block of exactly L.bound_bytes, `frame` a frame buffer; only the payload ranges are written
static void device_unpack(const Planes &P, const csic_rice_layout &L, const unsigned char *coded, unsigned char *frame)
{
    const int64_t bound = L.bound_bytes;
    const uint32_t max_dwords = (uint32_t)((L.bound_bytes - L.payload_offset) / 4);
    int64_t blk = 0;
    for (int p = 0; p < 3; ++p) {
        const uint32_t Q = (uint32_t)P.q[p], MASK = (1u << Q) - 1u, CAP = 248u * Q + 1u, G = (uint32_t)L.groups[p], n = (uint32_t)P.n[p];
        unsigned char *dst = frame + P.off[p];
        std::memset(dst, 0, (size_t)P.bytes[p]);
        for (uint32_t g0 = 0; g0 < G; g0 += 256, ++blk) {
            const uint32_t d0 = std::min(ld4(coded, bound, L.directory_offset + 4 * blk), max_dwords);
            const uint32_t d1 = std::min(std::max(ld4(coded, bound, L.directory_offset + 4 * blk + 4), d0), max_dwords);
            const uint32_t nw = std::min(d1 - d0, CAP);
            uint32_t *chunk = (uint32_t *)std::malloc(nw ? 4 * (size_t)nw : 1);            // s_chunk: exactly the dwords the kernel fills
            for (uint32_t i = 0; i < nw; ++i) chunk[i] = ld4(coded, bound, L.payload_offset + 4 * ((int64_t)d0 + i));
            uint32_t k[256], before_r[256], before_z[256], rtot = 0, ztot = 0;
            bool zero[256], unary[256];
            for (uint32_t t = 0; t < 256; ++t) {                                            // the first block scan
                const uint32_t g = g0 + t;
                uint32_t m = 15u;
                if (g < G) m = (ld4(coded, bound, L.modes_offset[p] + 4 * (int64_t)(g >> 3)) >> (4u * (g & 7u))) & 15u;
                zero[t] = m == 15u;
                k[t] = std::min(m, Q);
                unary[t] = !zero[t] && k[t] < Q;
                before_r[t] = rtot; before_z[t] = ztot;
                if (!zero[t]) { rtot += 31u * k[t]; ztot += unary[t]; }
            }
            const uint32_t rdw = std::min((rtot + 31u) / 32u, nw), uw = nw - rdw;
            uint32_t *cum = (uint32_t *)std::malloc(uw ? 4 * (size_t)uw : 1);              // s_cum
            for (uint32_t i = 0, run = 0; i < uw; ++i) cum[i] = run += (uint32_t)__builtin_popcount(chunk[rdw + i]);
            for (uint32_t t = 0; t < 256 && g0 + t < G; ++t) {
                const uint32_t g = g0 + t;
                const int64_t abit = (int64_t)g * Q, aat = L.anchors_offset[p] + 4 * (abit >> 5);
                const uint32_t as = (uint32_t)(abit & 31);
                uint32_t c = ld4(coded, bound, aat) >> as;
                if (as + Q > 32u) c |= ld4(coded, bound, aat + 4) << (32u - as);
                c &= MASK;
                uint32_t rbit = before_r[t], ubit = 32u * rdw;
                if (unary[t]) ubit += rice_after_terminator(chunk + rdw, cum, uw, 31u * before_z[t]);
                const uint32_t uend = 32u * nw;
                for (uint32_t j = 0; j < 32; ++j) {
                    if (j > 0 && !zero[t]) c = (c + rice_unfold(rice_next_u(chunk, nw, &rbit, &ubit, uend, k[t], Q), MASK)) & MASK;
                    if (c > MASK) { std::printf("FAILED: a code of more than q bits\n"); std::abort(); }
                    if (32u * g + j < n) {
                        const int64_t bit = ((int64_t)32 * g + j) * Q;
                        const uint32_t s = c << (bit & 7);
                        dst[bit >> 3] |= (unsigned char)s;
                        if (s >> 8) dst[(bit >> 3) + 1] |= (unsigned char)(s >> 8);
                    }
                }
            }
            std::free(cum);
            std::free(chunk);
        }
    }
}

static int bit_loops()
{
    for (int it = 0; it < 200000; ++it) {
        uint32_t w = rnd();
        if (it % 3 == 0) w &= rnd();
        if (it % 7 == 0) w = it % 14 ? 0u : 0xFFFFFFFFu;
        const uint32_t r = rnd() % 34;
        uint32_t want = 32, seen = 0;
        for (uint32_t b = 0; b < 32; ++b)
            if ((w >> b) & 1u) { if (seen == r) { want = b; break; } ++seen; }
        REQUIRE(rice_select32(w, r) == want);
    }
    for (int it = 0; it < 20000; ++it) {
        const uint32_t n = rnd() % 40;
        uint32_t *words = (uint32_t *)std::malloc(n ? 4 * (size_t)n : 1), *cum = (uint32_t *)std::malloc(n ? 4 * (size_t)n : 1);
        uint32_t ones = 0;
        for (uint32_t i = 0; i < n; ++i) { words[i] = it % 4 == 0 ? rnd() & rnd() & rnd() : rnd(); cum[i] = ones += (uint32_t)__builtin_popcount(words[i]); }
        for (int rep = 0; rep < 8; ++rep) {
            const uint32_t t = rep == 0 ? 0 : rep == 1 ? ones : rep == 2 ? ones + 1 : rnd() % (ones + 3);
            uint32_t want = 32 * n, seen = 0;
            if (t == 0) want = 0;
            else
                for (uint32_t b = 0; b < 32 * n; ++b)
                    if ((words[b >> 5] >> (b & 31)) & 1u) { if (++seen == t) { want = b + 1; break; } }
            REQUIRE(rice_after_terminator(words, cum, n, t) == want);
            // a unary number from any position, to any end
            uint32_t ubit = rnd() % (32 * n + 40), uend = rnd() % (32 * n + 40);
            const uint32_t from = ubit, end = std::min(uend, 32 * n);
            uint32_t zeros = 0, at = from;
            bool term = false;
            while (at < end) { if ((words[at >> 5] >> (at & 31)) & 1u) { term = true; ++at; break; } ++zeros; ++at; }
            bool got_term;
            const uint32_t got = rice_unary(words, n, &ubit, uend, &got_term);
            REQUIRE(got == zeros && got_term == term && ubit == (from < end ? at : from));
        }
        std::free(words); std::free(cum);
    }
    return 0;
}

int main()
{
    if (bit_loops()) return 1;
    static const int perms[6][3] = {{1, 2, 3}, {1, 3, 2}, {2, 1, 3}, {2, 3, 1}, {3, 1, 2}, {3, 2, 1}};
    static const int ab[6][2] = {{4, 4}, {2, 2}, {2, 0}, {1, 1}, {4, 0}, {1, 0}};
    long mutated = 0, accepted = 0, refused = 0;
    for (int it = 0; it < 80; ++it) {
        csic_params p;
        const bool wide = it % 8 == 7;                                 // every eighth frame has more than one block per plane
        REQUIRE(csic_params_default(&p, wide ? 8192 + (int)(rnd() % 700) : 1 + (int)(rnd() % 80), wide ? 1 + (int)(rnd() % 3) : 1 + (int)(rnd() % 24)) == CSIC_OK);
        const int k = (int)(rnd() % 6);
        p.chroma_a = ab[k][0]; p.chroma_b = ab[k][1];
        p.y_bits = 1 + (int)(rnd() % 8); p.cb_bits = 1 + (int)(rnd() % 8); p.cr_bits = 1 + (int)(rnd() % 8);
        p.factor = wide ? 1 : 1 << (rnd() % 4);
        std::memcpy(p.op, perms[rnd() % 6], sizeof p.op);
        p.out_format = (int)(rnd() % 4);                               // ignored
        csic_planar_bits_layout B;
        csic_rice_layout L;
        REQUIRE(csic_planar_bits_layout_of(&p, &B) == CSIC_OK && csic_rice_layout_of(&p, &L) == CSIC_OK);
        Planes P = {{B.y_offset, B.cb_offset, B.cr_offset}, {B.y_bytes, B.cb_bytes, B.cr_bytes},
                    {(int64_t)B.geometry.y_width * B.geometry.y_height, B.geometry.chroma_samples, B.geometry.chroma_samples},
                    {p.y_bits, p.cb_bits, p.cr_bits}};
        int64_t top = L.fixed_bytes, nb = 0;
        for (int pl = 0; pl < 3; ++pl) {
            REQUIRE(L.groups[pl] == (P.n[pl] + 31) / 32 && L.blocks[pl] == (L.groups[pl] + 255) / 256);
            top += 4 * L.blocks[pl] * (248 * P.q[pl] + 1);
            nb += L.blocks[pl];
        }
        REQUIRE(L.bound_bytes >= top && L.bound_bytes < top + 256 && L.bound_bytes % 256 == 0 && L.payload_offset == L.fixed_bytes);
        REQUIRE(L.payload_offset == L.directory_offset + 4 * (nb + 1));

        std::vector<unsigned char> frame((size_t)B.frame_bytes), back((size_t)B.frame_bytes), again((size_t)B.frame_bytes);
        std::vector<unsigned char> coded((size_t)L.bound_bytes), recoded((size_t)L.bound_bytes);
        fill_frame(frame, P, it % 5);
        uint64_t size = 0;
        REQUIRE(csic_rice_pack_host(&p, frame.data(), coded.data(), coded.size(), &size) == CSIC_OK);
        REQUIRE((int64_t)size >= L.fixed_bytes && (int64_t)size <= top && size % 4 == 0);
        REQUIRE(it % 5 != 3 || (int64_t)size == L.fixed_bytes);         // a constant frame has no payload
        unsigned char *dev = (unsigned char *)std::malloc((size_t)L.bound_bytes);          // what the device reads: exactly bound_bytes
        {
            // exact-size blocks on both sides: the sanitizer sees any access past either
            unsigned char *src = (unsigned char *)std::malloc(size ? size : 1), *dst = (unsigned char *)std::malloc(frame.size());
            std::memcpy(src, coded.data(), size);
            std::memset(dst, 0xEE, frame.size());
            REQUIRE(csic_rice_unpack_host(&p, src, size, dst) == CSIC_OK);
            REQUIRE(std::memcmp(dst, frame.data(), frame.size()) == 0);   // the payload ranges restored, the canary around them kept
            // the device's flow on the same bytes, garbage behind coded_bytes
            for (int64_t i = 0; i < L.bound_bytes; ++i) dev[i] = i < (int64_t)size ? coded[i] : (unsigned char)rnd();
            std::memset(dst, 0xEE, frame.size());
            device_unpack(P, L, dev, dst);
            REQUIRE(std::memcmp(dst, frame.data(), frame.size()) == 0);
            std::free(src); std::free(dst);
        }
        REQUIRE(csic_rice_pack_host(&p, frame.data(), recoded.data(), (size_t)size, &size) == CSIC_OK);     // capacity = exactly the size
        if (size > (uint64_t)L.fixed_bytes) {
            uint64_t need = 0;
            REQUIRE(csic_rice_pack_host(&p, frame.data(), recoded.data(), (size_t)size - 4, &need) == CSIC_EINVAL_SIZE && need == size);
        }

        for (int m = 0; m < (wide ? 40 : 300); ++m) {
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
            if (how == 3 && len) {                                                         // a nibble outside the modes, or any nibble
                const int pl = (int)(rnd() % 3);
                const size_t at = (size_t)L.modes_offset[pl] + rnd() % (size_t)(4 * ((L.groups[pl] + 7) / 8));
                if (at < len) src[at] = (unsigned char)((rnd() & 1) && P.q[pl] < 14 ? (src[at] & 0xF0) | (P.q[pl] + 1 + rnd() % (14 - P.q[pl])) : rnd());
            }
            if (how == 4) for (size_t i = 0; i < len; ++i) if (rnd() % 16 == 0) src[i] = (unsigned char)rnd();     // bytes at random
            if (how == 6) {                                                                // a directory entry: a little off, or anything
                const size_t at = (size_t)L.directory_offset + 4 * (rnd() % (size_t)(nb + 1));
                if (at + 4 <= len) { if (rnd() & 1) src[at] += (unsigned char)(1 + rnd() % 3); else for (int b = 0; b < 4; ++b) src[at + b] = (unsigned char)rnd(); }
            }
            if (how == 7 && len > (size_t)L.payload_offset)                                // bit flips in the payload
                for (int b = 1 + (int)(rnd() % 3); b > 0; --b) src[(size_t)L.payload_offset + rnd() % (len - (size_t)L.payload_offset)] ^= (unsigned char)(1u << (rnd() % 8));
            std::memset(back.data(), 0xEE, back.size());
            const int st = csic_rice_unpack_host(&p, src, len, back.data());
            ++mutated;
            if (st == CSIC_EFORMAT) {
                ++refused;
                for (size_t i = 0; i < back.size(); ++i) REQUIRE(back[i] == 0xEE);        // a refused frame writes nothing
            } else {
                REQUIRE(st == CSIC_OK);
                ++accepted;
                // re-packable: a valid frame that packs within the bound and decodes to itself; outside the payload ranges untouched
                uint64_t rsize = 0;
                REQUIRE(csic_rice_pack_host(&p, back.data(), recoded.data(), recoded.size(), &rsize) == CSIC_OK && (int64_t)rsize <= top);
                std::memset(again.data(), 0xEE, again.size());
                REQUIRE(csic_rice_unpack_host(&p, recoded.data(), (size_t)rsize, again.data()) == CSIC_OK);
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
    REQUIRE(csic_rice_unpack_host(nullptr, "", 0, &mutated) == CSIC_EINVAL_NULL);
    REQUIRE(mutated >= 18000 && accepted > 100 && refused > 1000);
    std::printf("rice fuzz ok: %ld mutated frames, %ld accepted, %ld refused\n", mutated, accepted, refused);
    return 0;
}
