// mc_fuzz.cpp -- the host codec of the motion-compensated temporal layer (csic_mc_delta_host / csic_mc_undelta_host,
// csrc/csic_mc_host.cpp) under ASan + UBSan: random sequences of frames whose contents move go through delta and undelta with the
// frames, the difference frames and the maps in heap blocks of exactly their sizes (nframes * frame_bytes; (nframes - 1) * map_stride +
// map_bytes); then mutated maps -- table sizes, table words up to INT32_MIN and INT32_MAX, nibbles, padding nibbles, bytes of a key
// frame's map, random bytes, a sequence cut to its first frames -- are fed to csic_mc_undelta_host.  Every call must return CSIC_OK with
// frames that delta again and come back, or CSIC_EFORMAT with the destination untouched; the sanitizers must stay silent.  Built and run
// by tests/test_cpp_mc.py; no GPU, nothing of the HIP library.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csic.h"

static uint64_t rng_state = 0xA0761D6478BD642Full;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, csic_last_error()); return 1; } } while (0)

struct Planes { int64_t off[3], bytes[3], n[3], w[3]; int q[3]; };

static void put_code(unsigned char *d, int64_t i, int q, uint32_t v)
{
    const int64_t bit = i * q;
    const uint32_t s = v << (bit & 7);
    d[bit >> 3] |= (unsigned char)s;
    if (s >> 8) d[(bit >> 3) + 1] |= (unsigned char)(s >> 8);
}
static uint32_t get_code(const unsigned char *d, int64_t bytes, int64_t i, int q)
{
    const int64_t bit = i * q, b = bit >> 3;
    uint32_t v = d[b];
    if (b + 1 < bytes) v |= (uint32_t)d[b + 1] << 8;
    return (v >> (bit & 7)) & ((1u << q) - 1u);
}
static void put_word(unsigned char *p, uint32_t v) { p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); p[2] = (unsigned char)(v >> 16); p[3] = (unsigned char)(v >> 24); }
static uint32_t get_word(const unsigned char *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// frame k of a sequence: frame k - 1 moved by one vector per stretch of a few groups, some groups redrawn (frame 0: noise or small steps)
static void fill_frame(unsigned char *f, const unsigned char *prev, size_t frame_bytes, const Planes &P, int kind, int range)
{
    std::memset(f, 0xEE, frame_bytes);
    for (int p = 0; p < 3; ++p) {
        unsigned char *d = f + P.off[p];
        std::memset(d, 0, (size_t)P.bytes[p]);
        const uint32_t mask = (1u << P.q[p]) - 1u;
        uint32_t c = rnd(), how = 0;
        int64_t s = 0;
        for (int64_t i = 0; i < P.n[p]; ++i) {
            if (i % 96 == 0) s = ((int64_t)(rnd() % (2 * range + 3)) - range - 1) * P.w[p] + (int64_t)(rnd() % (2 * range + 3)) - range - 1;
            if (i % 32 == 0) how = prev ? rnd() % 4 : 3;
            if (kind == 0) c = rnd(); else c += (rnd() % 3) - 1;
            uint32_t v = c;
            if (how < 3) {
                int64_t at = i + s;
                at = at < 0 ? 0 : at > P.n[p] - 1 ? P.n[p] - 1 : at;
                v = get_code(prev + P.off[p], P.bytes[p], at, P.q[p]);
            }
            put_code(d, i, P.q[p], v & mask);
        }
    }
}

int main()
{
    static const int perms[6][3] = {{1, 2, 3}, {1, 3, 2}, {2, 1, 3}, {2, 3, 1}, {3, 1, 2}, {3, 2, 1}};
    static const int ab[6][2] = {{4, 4}, {2, 2}, {2, 0}, {1, 1}, {4, 0}, {1, 0}};
    static const uint32_t words[6] = {0x80000000u, 0x7FFFFFFFu, 0xFFFFFFFFu, 1u, 0x7FFFFFE0u, 0x80000020u};
    long mutated = 0, accepted = 0, refused = 0, inter = 0, moved = 0;
    for (int it = 0; it < 64; ++it) {
        csic_params p;
        REQUIRE(csic_params_default(&p, 1 + (int)(rnd() % 96), 1 + (int)(rnd() % 32)) == CSIC_OK);
        const int k = (int)(rnd() % 6);
        p.chroma_a = ab[k][0]; p.chroma_b = ab[k][1];
        p.y_bits = 1 + (int)(rnd() % 8); p.cb_bits = 1 + (int)(rnd() % 8); p.cr_bits = 1 + (int)(rnd() % 8);
        p.factor = 1 << (rnd() % 3);
        std::memcpy(p.op, perms[rnd() % 6], sizeof p.op);
        p.out_format = (int)(rnd() % 4);                               // ignored
        csic_planar_bits_layout B;
        csic_mc_layout L;
        REQUIRE(csic_planar_bits_layout_of(&p, &B) == CSIC_OK && csic_mc_layout_of(&p, &L) == CSIC_OK);
        Planes P = {{B.y_offset, B.cb_offset, B.cr_offset}, {B.y_bytes, B.cb_bytes, B.cr_bytes},
                    {(int64_t)B.geometry.y_width * B.geometry.y_height, B.geometry.chroma_samples, B.geometry.chroma_samples},
                    {B.geometry.y_width, B.geometry.chroma_width, B.geometry.chroma_width}, {p.y_bits, p.cb_bits, p.cr_bits}};
        int64_t at = 192;
        for (int pl = 0; pl < 3; ++pl) {
            REQUIRE(L.groups[pl] == (P.n[pl] + 31) / 32 && L.map_offset[pl] == at && L.table_offset[pl] == 64 * pl && L.width[pl] == P.w[pl]);
            at += 4 * ((L.groups[pl] + 7) / 8);
        }
        REQUIRE(L.map_bytes == at && L.map_stride == (at + 255) / 256 * 256);

        const int nframes = 1 + (int)(rnd() % 4), gop = 1 + (int)(rnd() % (nframes + 1)), range = (int)(rnd() % 4) + (it % 16 == 0 ? 4 : 0);
        const size_t fb = (size_t)B.frame_bytes, ms = (size_t)L.map_stride, mb = (size_t)L.map_bytes;
        const size_t fbytes = (size_t)nframes * fb, mbytes = (size_t)(nframes - 1) * ms + mb;
        // exact-size blocks: the sanitizer sees any access past any of them
        unsigned char *frames = (unsigned char *)std::malloc(fbytes), *diff = (unsigned char *)std::malloc(fbytes);
        unsigned char *back = (unsigned char *)std::malloc(fbytes), *maps = (unsigned char *)std::malloc(mbytes), *bad = (unsigned char *)std::malloc(mbytes);
        unsigned char *diff2 = (unsigned char *)std::malloc(fbytes), *maps2 = (unsigned char *)std::malloc(mbytes), *again = (unsigned char *)std::malloc(fbytes);
        for (int f = 0; f < nframes; ++f) fill_frame(frames + f * fb, f ? frames + (f - 1) * fb : nullptr, fb, P, it % 2, range);
        std::memset(diff, 0xEE, fbytes);
        std::memset(maps, 0xEE, mbytes);
        REQUIRE(csic_mc_delta_host(&p, frames, nframes, gop, range, diff, maps) == CSIC_OK);
        for (int f = 0; f < nframes; ++f) {
            for (size_t i = mb; i < ms && (size_t)f * ms + i < mbytes; ++i) REQUIRE(maps[f * ms + i] == 0xEE);      // behind map_bytes: untouched
            for (size_t i = 0; i < mb; ++i)
                if (f % gop == 0) REQUIRE(maps[f * ms + i] == 0);
            if (f % gop)
                for (int pl = 0; pl < 3; ++pl) {
                    const uint32_t T = get_word(maps + f * ms + 64 * pl);
                    REQUIRE(T >= 1 && T <= 15 && get_word(maps + f * ms + 64 * pl + 4) == 0);
                    for (int64_t g = 0; g < L.groups[pl]; ++g) {
                        const uint32_t nib = (maps[f * ms + L.map_offset[pl] + (g >> 1)] >> (4 * (g & 1))) & 15u;
                        REQUIRE(nib <= T);
                        inter += nib != 0;
                        moved += nib > 1;
                    }
                }
            for (size_t i = 0; i < fb; ++i) {                                                                       // outside the payload ranges: untouched
                bool payload = false;
                for (int pl = 0; pl < 3; ++pl) payload |= (int64_t)i >= P.off[pl] && (int64_t)i < P.off[pl] + P.bytes[pl];
                if (!payload) REQUIRE(diff[f * fb + i] == 0xEE);
            }
        }
        std::memset(back, 0xEE, fbytes);
        REQUIRE(csic_mc_undelta_host(&p, diff, maps, nframes, gop, back) == CSIC_OK);
        REQUIRE(std::memcmp(back, frames, fbytes) == 0);
        // in place is refused, as is a partial overlap and a range outside 0..7
        std::memcpy(back, frames, fbytes);
        REQUIRE(csic_mc_delta_host(&p, back, nframes, gop, range, back, maps2) == CSIC_EINVAL_SIZE && std::memcmp(back, frames, fbytes) == 0);
        REQUIRE(csic_mc_undelta_host(&p, back, maps, nframes, gop, back) == CSIC_EINVAL_SIZE && std::memcmp(back, frames, fbytes) == 0);
        if (nframes > 2) REQUIRE(csic_mc_delta_host(&p, frames, nframes - 1, gop, range, frames + fb, maps2) == CSIC_EINVAL_SIZE);
        REQUIRE(csic_mc_delta_host(&p, frames, nframes, gop, 8, diff2, maps2) == CSIC_EINVAL_SIZE && csic_mc_delta_host(&p, frames, nframes, gop, -1, diff2, maps2) == CSIC_EINVAL_SIZE);

        for (int m = 0; m < 96; ++m) {
            std::memcpy(bad, maps, mbytes);
            int nf = nframes;
            const int how = (int)(rnd() % 8);
            const int f = (int)(rnd() % nframes), pl = (int)(rnd() % 3);
            unsigned char *map = bad + f * ms, *tab = map + 64 * pl, *sec = map + L.map_offset[pl];
            const int64_t room = (L.groups[pl] + 7) / 8 * 8;
            if (how == 0) put_word(tab, rnd() % 4 ? rnd() % 18 : rnd());                                                        // the table's size
            else if (how == 1) put_word(tab + 4 * (1 + rnd() % 15), rnd() % 2 ? words[rnd() % 6] : rnd());                      // a word, any displacement
            else if (how == 2) { const int64_t g = rnd() % L.groups[pl]; sec[g >> 1] ^= (unsigned char)((1 + rnd() % 15) << (4 * (g & 1))); }   // a group's nibble
            else if (how == 3 && room > L.groups[pl]) { const int64_t g = L.groups[pl] + rnd() % (room - L.groups[pl]); sec[g >> 1] |= (unsigned char)((1 + rnd() % 15) << (4 * (g & 1))); }
            else if (how == 4) { const int kf = f / gop * gop; bad[kf * ms + rnd() % mb] |= (unsigned char)(1u << (rnd() % 8)); }   // a key frame's map
            else if (how == 5) { for (size_t i = 0; i < mb; ++i) if (rnd() % 8 == 0) map[i] = (unsigned char)rnd(); }
            else if (how == 6) { for (int t = 2; t < 16; ++t) if (t <= (int)get_word(tab)) put_word(tab + 4 * t, words[rnd() % 6]); }  // every entry far out
            else nf = 1 + (int)(rnd() % nframes);                                                                               // cut to the first frames
            const size_t nfb = (size_t)nf * fb, nmb = (size_t)(nf - 1) * ms + mb;
            unsigned char *src = (unsigned char *)std::malloc(nmb), *dst = (unsigned char *)std::malloc(nfb);
            std::memcpy(src, bad, nmb);
            std::memset(dst, 0xEE, nfb);
            const int st = csic_mc_undelta_host(&p, diff, src, nf, gop, dst);
            ++mutated;
            if (st == CSIC_EFORMAT) {
                ++refused;
                REQUIRE(how != 7 && how != 6);
                for (size_t i = 0; i < nfb; ++i) REQUIRE(dst[i] == 0xEE);                       // a refused call writes nothing
            } else {
                REQUIRE(st == CSIC_OK && how != 4);
                ++accepted;
                if (how == 7) REQUIRE(std::memcmp(dst, frames, nfb) == 0);                      // the first frames of a sequence are a sequence
                // valid frames: they delta again and come back, and nothing outside the payload ranges was written
                REQUIRE(csic_mc_delta_host(&p, dst, nf, gop, range, diff2, maps2) == CSIC_OK);
                std::memset(again, 0xEE, nfb);
                REQUIRE(csic_mc_undelta_host(&p, diff2, maps2, nf, gop, again) == CSIC_OK && std::memcmp(again, dst, nfb) == 0);
            }
            std::free(src); std::free(dst);
        }
        std::free(frames); std::free(diff); std::free(back); std::free(maps); std::free(bad); std::free(diff2); std::free(maps2); std::free(again);
    }
    csic_mc_layout L;
    REQUIRE(csic_mc_undelta_host(nullptr, "", "", 1, 1, &mutated) == CSIC_EINVAL_NULL && csic_mc_layout_of(nullptr, &L) == CSIC_EINVAL_NULL);
    REQUIRE(mutated >= 6000 && accepted > 500 && refused > 500 && inter > 1000 && moved > 200);
    std::printf("mc fuzz ok: %ld mutated sequences, %ld accepted, %ld refused, %ld inter groups, %ld of them displaced\n", mutated, accepted, refused, inter, moved);
    return 0;
}
