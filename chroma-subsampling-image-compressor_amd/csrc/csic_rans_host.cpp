// csic_rans_host.cpp -- the host codec of the rANS coding (csic_rans_layout_of, csic_rans_pack_host, csic_rans_unpack_host; host only, no
// device).  The format -- the model and its scaling rule, the state, blocks of 1024 groups with 64 interleaved streams, the directory,
// rANS and raw chunks -- is stated in include/csic.h next to the group coding, whose groups, anchors and folded residuals it takes from
// pack_geometry (csic_pack_host.cpp) and whose byte accessors and group load it shares through csic_group_host.h.  The blocks, the
// tables section and the directory are this coding's own.  csic_rans_unpack_host and the container reader take bytes nobody vouches
// for: rans_decode_frame proves every length before it reads and runs once without an output (rans_check_coded) before anything is
// written; the decode step and the word reads are those of csic_rans_decode.h, which the device codec (csic_rans.hip) runs as well.
#include <algorithm>
#include <cstring>
#include <vector>

#include "csic_group_host.h"
#include "csic_rans_decode.h"

namespace csic {

int rans_geometry(const csic_params *p, RansGeometry *G)
{
    if (!p || !G) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    const int st = pack_geometry(p, &G->pk);
    if (st != CSIC_OK) return st;
    const PackGeometry &P = G->pk;
    csic_rans_layout &L = G->layout;
    int64_t at = 0;
    G->max_payload_dwords = G->nblocks = 0;
    for (int pl = 0; pl < 3; ++pl) {
        L.groups[pl] = P.layout.groups[pl];
        L.blocks[pl] = (L.groups[pl] + RANS_BLOCK - 1) / RANS_BLOCK;
        G->block0[pl] = G->nblocks;
        G->nblocks += L.blocks[pl];
        L.tables_offset[pl] = at;
        at += 2 * ((int64_t)1 << P.q[pl]);
        const int64_t last = L.groups[pl] - (L.blocks[pl] - 1) * RANS_BLOCK;       // groups of the plane's last block, 1 .. 1024
        G->max_payload_dwords += (L.blocks[pl] - 1) * rans_raw_dwords(RANS_BLOCK, (uint32_t)P.q[pl]) + rans_raw_dwords((uint32_t)last, (uint32_t)P.q[pl]);
    }
    if (G->max_payload_dwords >= ((int64_t)1 << 31)) return set_error(CSIC_EINVAL_SIZE, "frame too large for the rANS coding's directory");
    for (int pl = 0; pl < 3; ++pl) {
        L.anchors_offset[pl] = at;
        at += 4 * ((L.groups[pl] * P.q[pl] + 31) / 32);
    }
    L.directory_offset = at;
    L.payload_offset = L.fixed_bytes = at + 4 * (G->nblocks + 1);
    L.bound_bytes = (L.fixed_bytes + 4 * G->max_payload_dwords + 255) / 256 * 256;
    return CSIC_OK;
}

void rans_scale_counts(const uint32_t *c, int nsym, uint64_t N, uint16_t *f)
{
    uint32_t v[256];
    int64_t sum = 0;
    int top = 0;                                       // the largest count, the smallest s on a tie
    for (int s = 0; s < nsym; ++s) {
        const uint64_t fl = (uint64_t)c[s] * RANS_M / N;
        v[s] = c[s] == 0 ? 0u : fl < 1 ? 1u : (uint32_t)fl;
        sum += v[s];
        if (c[s] > c[top]) top = s;
    }
    if (sum < (int64_t)RANS_M) v[top] += (uint32_t)(RANS_M - sum);
    for (; sum > (int64_t)RANS_M; --sum) {
        int t = 0;
        for (int s = 1; s < nsym; ++s)
            if (v[s] > v[t]) t = s;
        --v[t];
    }
    for (int s = 0; s < nsym; ++s) f[s] = (uint16_t)v[s];
}

// the folded residuals of the groups [g0, g1) of a plane, 32 per group (slot 0 unused), and their anchors into the coded frame
static void load_block(const RansGeometry &G, const unsigned char *frame, int pl, int64_t g0, int64_t g1, std::vector<uint8_t> &u, unsigned char *coded)
{
    u.resize((size_t)(g1 - g0) * 32);
    for (int64_t g = g0; g < g1; ++g) {
        uint32_t c[32], uu[32];
        (void)load_group(G.pk, frame, pl, g, c, uu);
        for (int j = 0; j < 32; ++j) u[(size_t)(g - g0) * 32 + j] = (uint8_t)uu[j];
        if (coded) or_bits(coded + G.layout.anchors_offset[pl], g * G.pk.q[pl], c[0]);
    }
}

int rans_pack_frame(const RansGeometry &G, const unsigned char *frame, unsigned char *coded, size_t capacity, uint64_t *coded_bytes)
{
    const csic_rans_layout &L = G.layout;
    if (capacity < (size_t)L.fixed_bytes)
        return set_error(CSIC_EINVAL_SIZE, "a coded frame of these parameters needs at least %lld bytes, got room for %zu", (long long)L.fixed_bytes, capacity);
    std::memset(coded, 0, (size_t)L.fixed_bytes);
    unsigned char *dir = coded + L.directory_offset;
    size_t pos = (size_t)L.payload_offset;            // where the next chunk goes; keeps counting past `capacity`
    std::vector<uint8_t> u;
    std::vector<uint16_t> words;
    std::vector<uint32_t> chunk;
    for (int pl = 0; pl < 3; ++pl) {
        const int q = G.pk.q[pl], nsym = 1 << q;
        // the model: counts over every coded slot of the plane, scaled
        uint32_t cnt[256] = {0}, cum[256];
        uint16_t f[256];
        for (int64_t b = 0; b < L.blocks[pl]; ++b) {
            const int64_t g0 = b * RANS_BLOCK, g1 = std::min<int64_t>(g0 + RANS_BLOCK, L.groups[pl]);
            load_block(G, frame, pl, g0, g1, u, coded);
            for (size_t k = 0; k < u.size(); ++k)
                if (k & 31) ++cnt[u[k]];
        }
        rans_scale_counts(cnt, nsym, (uint64_t)31 * (uint64_t)L.groups[pl], f);
        for (int s = 0, run = 0; s < nsym; ++s) {
            cum[s] = (uint32_t)run;
            run += f[s];
            coded[L.tables_offset[pl] + 2 * s] = (unsigned char)f[s];
            coded[L.tables_offset[pl] + 2 * s + 1] = (unsigned char)(f[s] >> 8);
        }
        for (int64_t b = 0; b < L.blocks[pl]; ++b) {
            const int64_t g0 = b * RANS_BLOCK, g1 = std::min<int64_t>(g0 + RANS_BLOCK, L.groups[pl]);
            const uint32_t ng = (uint32_t)(g1 - g0), ns = std::min(ng, RANS_LANES), rawdw = rans_raw_dwords(ng, (uint32_t)q);
            load_block(G, frame, pl, g0, g1, u, nullptr);
            // the encoder: the decode order backwards, words collected backwards
            uint32_t x[RANS_LANES];
            for (uint32_t l = 0; l < RANS_LANES; ++l) x[l] = RANS_L;
            words.clear();
            for (int t = 31 * (int)RANS_ROUNDS - 1; t >= 0; --t) {
                const uint32_t i = (uint32_t)t / 31u, j = 1u + (uint32_t)t % 31u;
                for (int l = (int)RANS_LANES - 1; l >= 0; --l) {
                    const uint32_t g = RANS_LANES * i + (uint32_t)l;
                    if (g >= ng) continue;
                    const uint32_t s = u[(size_t)g * 32 + j], fs = f[s];
                    if ((x[l] >> 20) >= fs) { words.push_back((uint16_t)x[l]); x[l] >>= 16; }
                    x[l] = ((x[l] / fs) << RANS_SCALE_BITS) + x[l] % fs + cum[s];
                }
            }
            const uint32_t ransdw = ns + (uint32_t)((words.size() + 1) / 2);
            const bool raw = rawdw < ransdw;
            chunk.assign(raw ? rawdw : ransdw, 0u);
            if (raw) {
                for (uint32_t g = 0; g < ng; ++g)
                    for (uint32_t j = 1; j < 32; ++j) {
                        const uint64_t bit = ((uint64_t)g * 31 + (j - 1)) * (uint64_t)q;
                        const uint64_t v = (uint64_t)u[(size_t)g * 32 + j] << (bit & 31);
                        chunk[bit >> 5] |= (uint32_t)v;
                        if (v >> 32) chunk[(bit >> 5) + 1] |= (uint32_t)(v >> 32);
                    }
            } else {
                for (uint32_t l = 0; l < ns; ++l) chunk[l] = x[l];
                for (size_t k = 0; k < words.size(); ++k) chunk[ns + k / 2] |= (uint32_t)words[words.size() - 1 - k] << (16 * (k & 1));
            }
            put_u32(dir + 4 * (G.block0[pl] + b), (uint32_t)((pos - (size_t)L.payload_offset) / 4) | (raw ? RANS_RAW_FLAG : 0u));
            if (pos + 4 * chunk.size() <= capacity)
                for (size_t k = 0; k < chunk.size(); ++k) put_u32(coded + pos + 4 * k, chunk[k]);
            pos += 4 * chunk.size();
        }
    }
    put_u32(dir + 4 * G.nblocks, (uint32_t)((pos - (size_t)L.payload_offset) / 4));
    *coded_bytes = pos;
    if (pos > capacity) return set_error(CSIC_EINVAL_SIZE, "this frame codes to %zu bytes, got room for %zu", pos, capacity);
    return CSIC_OK;
}

// Checks everything csic_rans_unpack_host checks and, with a `frame`, writes the three payload ranges (the caller has run it without
// one first).  Reads coded[0, coded_bytes) only.
static int rans_decode_frame(const RansGeometry &G, const unsigned char *coded, size_t coded_bytes, unsigned char *frame)
{
    const csic_rans_layout &L = G.layout;
    if (coded_bytes < (size_t)L.fixed_bytes || coded_bytes % 4 != 0 || coded_bytes > (size_t)(L.fixed_bytes + 4 * G.max_payload_dwords))
        return set_error(CSIC_EFORMAT, "a rANS-coded frame of these parameters has %lld to %lld bytes in dwords, not %zu", (long long)L.fixed_bytes,
                         (long long)(L.fixed_bytes + 4 * G.max_payload_dwords), coded_bytes);
    const unsigned char *dir = coded + L.directory_offset;
    const uint64_t total = (coded_bytes - (size_t)L.fixed_bytes) / 4;
    if (get_u32(dir) & ~RANS_RAW_FLAG || get_u32(dir + 4 * G.nblocks) != total)
        return set_error(CSIC_EFORMAT, "rANS-coded frame: the directory runs from %u to %u dwords, the frame's size says 0 to %llu", get_u32(dir) & ~RANS_RAW_FLAG,
                         get_u32(dir + 4 * G.nblocks), (unsigned long long)total);
    std::vector<uint8_t> slot2sym(RANS_M), u;
    std::vector<uint32_t> w;
    for (int pl = 0; pl < 3; ++pl) {
        const int q = G.pk.q[pl], nsym = 1 << q;
        const uint32_t mask = (1u << q) - 1u;
        const int64_t n = G.pk.n[pl], groups = L.groups[pl];
        const unsigned char *an = coded + L.anchors_offset[pl];
        uint32_t entry[256], sum = 0;
        for (int s = 0; s < nsym; ++s) {
            const uint32_t fs = coded[L.tables_offset[pl] + 2 * s] | ((uint32_t)coded[L.tables_offset[pl] + 2 * s + 1] << 8);
            entry[s] = rans_entry(fs, sum);
            for (uint32_t k = 0; k < (entry[s] & 0xFFFFu); ++k) slot2sym[sum + k] = (uint8_t)s;
            sum += fs;                                 // (65535 * 256 < 2^32)
        }
        if (sum != RANS_M) return set_error(CSIC_EFORMAT, "rANS-coded frame: the table of plane %d sums to %u, not %u", pl, sum, RANS_M);
        for (int64_t bit = groups * q; bit < (groups * q + 31) / 32 * 32; ++bit)
            if ((an[bit >> 3] >> (bit & 7)) & 1) return set_error(CSIC_EFORMAT, "rANS-coded frame: the anchors of plane %d are not zero-padded", pl);
        unsigned char *dst = frame ? frame + G.pk.src_offset[pl] : nullptr;
        if (dst) std::memset(dst, 0, (size_t)G.pk.src_bytes[pl]);
        for (int64_t b = 0; b < L.blocks[pl]; ++b) {
            const int64_t blk = G.block0[pl] + b;
            const uint32_t e0 = get_u32(dir + 4 * blk), e1 = get_u32(dir + 4 * (blk + 1));
            const uint64_t d0 = e0 & ~RANS_RAW_FLAG, d1 = e1 & ~RANS_RAW_FLAG;
            const bool raw = (e0 & RANS_RAW_FLAG) != 0;
            const int64_t g0 = b * RANS_BLOCK, g1 = std::min<int64_t>(g0 + RANS_BLOCK, groups);
            const uint32_t ng = (uint32_t)(g1 - g0), ns = std::min(ng, RANS_LANES), rawdw = rans_raw_dwords(ng, (uint32_t)q);
            if (d1 < d0 || d1 > total || (raw ? d1 - d0 != rawdw : d1 - d0 < ns || d1 - d0 > rawdw))
                return set_error(CSIC_EFORMAT, "rANS-coded frame: the %s chunk of block %lld of plane %d lies at dwords %llu to %llu; raw it has %u, its states %u",
                                 raw ? "raw" : "rANS", (long long)b, pl, (unsigned long long)d0, (unsigned long long)d1, rawdw, ns);
            const uint32_t nw = (uint32_t)(d1 - d0);
            w.resize(nw);
            for (uint32_t i = 0; i < nw; ++i) w[i] = get_u32(coded + L.payload_offset + 4 * (d0 + i));     // (d1 <= total: inside coded_bytes)
            u.assign((size_t)ng * 32, 0);
            if (raw) {
                const uint32_t bits = ng * 31u * (uint32_t)q;
                if ((bits & 31u) && (w[nw - 1] >> (bits & 31u)))
                    return set_error(CSIC_EFORMAT, "rANS-coded frame: the raw chunk of block %lld of plane %d is not zero-padded", (long long)b, pl);
                for (uint32_t g = 0; g < ng; ++g)
                    for (uint32_t j = 1; j < 32; ++j) u[(size_t)g * 32 + j] = (uint8_t)rans_raw_bits(w.data(), nw, (g * 31u + j - 1u) * (uint32_t)q, (uint32_t)q);
            } else {
                uint32_t x[RANS_LANES], next = 0;
                const uint32_t *seg = w.data() + ns, segdw = nw - ns;
                for (uint32_t l = 0; l < ns; ++l)
                    if ((x[l] = w[l]) < RANS_L)
                        return set_error(CSIC_EFORMAT, "rANS-coded frame: stream %u of block %lld of plane %d starts below 2^16", l, (long long)b, pl);
                for (uint32_t t = 0; t < 31u * RANS_ROUNDS; ++t) {
                    const uint32_t i = t / 31u, j = 1u + t % 31u;
                    for (uint32_t l = 0; l < ns && RANS_LANES * i + l < ng; ++l) {
                        bool refill;
                        u[(size_t)(RANS_LANES * i + l) * 32 + j] = (uint8_t)rans_decode_step(&x[l], slot2sym.data(), entry, &refill);
                        if (refill) rans_refill(&x[l], rans_word(seg, segdw, next++));
                    }
                }
                const bool padded = next + 1u == 2u * segdw && rans_word(seg, segdw, next) == 0;
                if (next != 2u * segdw && !padded)
                    return set_error(CSIC_EFORMAT, "rANS-coded frame: block %lld of plane %d stores %u words and uses %u", (long long)b, pl, 2u * segdw, next);
                for (uint32_t l = 0; l < ns; ++l)
                    if (x[l] != RANS_L)
                        return set_error(CSIC_EFORMAT, "rANS-coded frame: stream %u of block %lld of plane %d does not end at 2^16", l, (long long)b, pl);
            }
            if (!dst) continue;
            for (int64_t g = g0; g < g1; ++g) {
                uint32_t c = code_at(an, (groups * q + 7) / 8, g, q);
                for (int j = 0; j < 32 && 32 * g + j < n; ++j) {
                    if (j > 0) c = (c + rice_unfold(u[(size_t)(g - g0) * 32 + j], mask)) & mask;
                    or_bits(dst, (32 * g + j) * q, c);
                }
            }
        }
    }
    return CSIC_OK;
}

int rans_check_coded(const RansGeometry &G, const unsigned char *coded, size_t coded_bytes) { return rans_decode_frame(G, coded, coded_bytes, nullptr); }

int rans_unpack_frame(const RansGeometry &G, const unsigned char *coded, size_t coded_bytes, unsigned char *frame)
{
    const int st = rans_check_coded(G, coded, coded_bytes);
    return st != CSIC_OK ? st : rans_decode_frame(G, coded, coded_bytes, frame);
}

} // namespace csic

using namespace csic;

extern "C" {

int csic_rans_layout_of(const csic_params *p, csic_rans_layout *layout)
{
    return host_codec_call(!p || !layout, p, rans_geometry, "", [&](const RansGeometry &G) { *layout = G.layout; return (int)CSIC_OK; });
}

int csic_rans_pack_host(const csic_params *p, const void *bits_frame, void *coded, size_t capacity, uint64_t *coded_bytes)
{
    return host_codec_call(!p || !bits_frame || !coded || !coded_bytes, p, rans_geometry, "out of host memory coding a frame", [&](const RansGeometry &G) {
        return rans_pack_frame(G, static_cast<const unsigned char *>(bits_frame), static_cast<unsigned char *>(coded), capacity, coded_bytes);
    });
}

int csic_rans_unpack_host(const csic_params *p, const void *coded, size_t coded_bytes, void *bits_frame)
{
    return host_codec_call(!p || !coded || !bits_frame, p, rans_geometry, "out of host memory decoding a frame", [&](const RansGeometry &G) {
        return rans_unpack_frame(G, static_cast<const unsigned char *>(coded), coded_bytes, static_cast<unsigned char *>(bits_frame));
    });
}

} // extern "C"
