// pack_fuzz.cpp -- the host codec of the group coding (csic_pack_host / csic_unpack_host, csrc/csic_pack_host.cpp) under ASan + UBSan:
// random frames packed and unpacked, then about 20 000 mutated coded frames -- bit flips, truncations, extensions, nibbles above q,
// random bytes -- fed to csic_unpack_host from heap blocks of exactly their length.  Every call must return CSIC_OK with a frame that
// packs again and decodes to itself, or CSIC_EFORMAT with the destination untouched; the sanitizers must stay silent.
// Built and run by tests/test_cpp_pack.py; no GPU, nothing of the HIP library.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csic.h"

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
            const uint32_t v = c & ((1u << P.q[p]) - 1u);              // kind 3: constant
            const int64_t bit = i * P.q[p];
            const uint32_t s = v << (bit & 7);
            d[bit >> 3] |= (unsigned char)s;
            if (s >> 8) d[(bit >> 3) + 1] |= (unsigned char)(s >> 8);
        }
    }
}

int main()
{
    static const int perms[6][3] = {{1, 2, 3}, {1, 3, 2}, {2, 1, 3}, {2, 3, 1}, {3, 1, 2}, {3, 2, 1}};
    static const int ab[6][2] = {{4, 4}, {2, 2}, {2, 0}, {1, 1}, {4, 0}, {1, 0}};
    long mutated = 0, accepted = 0, refused = 0;
    for (int it = 0; it < 64; ++it) {
        csic_params p;
        REQUIRE(csic_params_default(&p, 1 + (int)(rnd() % 80), 1 + (int)(rnd() % 24)) == CSIC_OK);
        const int k = (int)(rnd() % 6);
        p.chroma_a = ab[k][0]; p.chroma_b = ab[k][1];
        p.y_bits = 1 + (int)(rnd() % 8); p.cb_bits = 1 + (int)(rnd() % 8); p.cr_bits = 1 + (int)(rnd() % 8);
        p.factor = 1 << (rnd() % 4);
        std::memcpy(p.op, perms[rnd() % 6], sizeof p.op);
        p.out_format = (int)(rnd() % 4);                               // ignored
        csic_planar_bits_layout B;
        csic_pack_layout L;
        REQUIRE(csic_planar_bits_layout_of(&p, &B) == CSIC_OK && csic_pack_layout_of(&p, &L) == CSIC_OK);
        Planes P = {{B.y_offset, B.cb_offset, B.cr_offset}, {B.y_bytes, B.cb_bytes, B.cr_bytes},
                    {(int64_t)B.geometry.y_width * B.geometry.y_height, B.geometry.chroma_samples, B.geometry.chroma_samples},
                    {p.y_bits, p.cb_bits, p.cr_bits}};
        int64_t top = L.fixed_bytes;
        for (int pl = 0; pl < 3; ++pl) {
            REQUIRE(L.groups[pl] == (P.n[pl] + 31) / 32);
            top += 4 * L.groups[pl] * P.q[pl];
        }
        REQUIRE(L.bound_bytes >= top && L.bound_bytes % 256 == 0 && L.payload_offset == L.fixed_bytes);

        std::vector<unsigned char> frame((size_t)B.frame_bytes), back((size_t)B.frame_bytes), again((size_t)B.frame_bytes);
        std::vector<unsigned char> coded((size_t)L.bound_bytes), recoded((size_t)L.bound_bytes);
        fill_frame(frame, P, it % 4);
        uint64_t size = 0;
        REQUIRE(csic_pack_host(&p, frame.data(), coded.data(), coded.size(), &size) == CSIC_OK);
        REQUIRE((int64_t)size >= L.fixed_bytes && (int64_t)size <= top && size % 4 == 0);
        REQUIRE(it % 4 != 3 || (int64_t)size == L.fixed_bytes);         // a constant frame has no payload
        {
            // exact-size blocks on both sides: the sanitizer sees any access past either
            unsigned char *src = (unsigned char *)std::malloc(size ? size : 1), *dst = (unsigned char *)std::malloc(frame.size());
            std::memcpy(src, coded.data(), size);
            std::memset(dst, 0xEE, frame.size());
            REQUIRE(csic_unpack_host(&p, src, size, dst) == CSIC_OK);
            REQUIRE(std::memcmp(dst, frame.data(), frame.size()) == 0);   // the payload ranges restored, the canary around them kept
            std::free(src); std::free(dst);
        }
        REQUIRE(csic_pack_host(&p, frame.data(), recoded.data(), (size_t)size, &size) == CSIC_OK);     // capacity = exactly the size
        if (size > (uint64_t)L.fixed_bytes) {
            uint64_t need = 0;
            REQUIRE(csic_pack_host(&p, frame.data(), recoded.data(), (size_t)size - 4, &need) == CSIC_EINVAL_SIZE && need == size);
        }

        for (int m = 0; m < 320; ++m) {
            size_t len = (size_t)size;
            const int how = (int)(rnd() % 6);
            if (how == 1) len = rnd() % (size + 1);                                       // truncated anywhere
            else if (how == 2) len = (size_t)size + 4 * (1 + rnd() % 3);                  // extended
            else if (how == 5) len = 4 * (rnd() % (size_t)(top / 4 + 2));                 // any length in dwords
            unsigned char *src = (unsigned char *)std::malloc(len ? len : 1);
            for (size_t i = 0; i < len; ++i) src[i] = i < size ? coded[i] : (unsigned char)rnd();
            if (how == 0 && len)                                                           // 1 .. 3 bit flips
                for (int b = 1 + (int)(rnd() % 3); b > 0; --b) src[rnd() % len] ^= (unsigned char)(1u << (rnd() % 8));
            if (how == 3 && len) {                                                         // a nibble above q, or any nibble
                const int pl = (int)(rnd() % 3);
                const size_t at = (size_t)L.widths_offset[pl] + rnd() % (size_t)(4 * ((L.groups[pl] + 7) / 8));
                if (at < len) src[at] = (unsigned char)((rnd() & 1) ? (src[at] & 0xF0) | (P.q[pl] + 1 + rnd() % (15 - P.q[pl])) : rnd());
            }
            if (how == 4) for (size_t i = 0; i < len; ++i) if (rnd() % 16 == 0) src[i] = (unsigned char)rnd();     // bytes at random
            std::memset(back.data(), 0xEE, back.size());
            const int st = csic_unpack_host(&p, src, len, back.data());
            ++mutated;
            if (st == CSIC_EFORMAT) {
                ++refused;
                for (size_t i = 0; i < back.size(); ++i) REQUIRE(back[i] == 0xEE);        // a refused frame writes nothing
            } else {
                REQUIRE(st == CSIC_OK);
                ++accepted;
                // re-packable: a valid frame that packs within the bound and decodes to itself; outside the payload ranges untouched
                uint64_t rsize = 0;
                REQUIRE(csic_pack_host(&p, back.data(), recoded.data(), recoded.size(), &rsize) == CSIC_OK && (int64_t)rsize <= top);
                std::memset(again.data(), 0xEE, again.size());
                REQUIRE(csic_unpack_host(&p, recoded.data(), (size_t)rsize, again.data()) == CSIC_OK);
                REQUIRE(std::memcmp(again.data(), back.data(), back.size()) == 0);
                for (int pl = 0; pl < 3; ++pl) {
                    const int used = (int)((P.n[pl] * P.q[pl]) % 8);
                    if (used) REQUIRE((back[(size_t)(P.off[pl] + P.bytes[pl] - 1)] >> used) == 0);
                }
            }
            std::free(src);
        }
    }
    REQUIRE(csic_unpack_host(nullptr, "", 0, &mutated) == CSIC_EINVAL_NULL);
    REQUIRE(mutated >= 20000 && accepted > 100 && refused > 1000);
    std::printf("pack fuzz ok: %ld mutated frames, %ld accepted, %ld refused\n", mutated, accepted, refused);
    return 0;
}
