// csic_rice_host.cpp -- the host codec of the Rice coding (csic_rice_layout_of, csic_rice_pack_host, csic_rice_unpack_host; host only, no
// device).  The format -- modes, blocks, the directory, a chunk's R and U -- is stated in include/csic.h next to the group coding, whose
// groups, anchors, folded residuals, nibble and anchors sections and block numbering it takes from pack_geometry (csic_pack_host.cpp),
// and whose byte accessors, group load and section check it shares through csic_group_host.h.  csic_rice_unpack_host and the
// container reader take bytes nobody vouches for: rice_check_coded proves every length before anything is decoded, and the bit reads
// themselves are those of csic_rice_decode.h, which the device codec (csic_rice.hip) runs as well.
#include <cstring>
#include <vector>

#include "csic_group_host.h"

namespace csic {

int rice_geometry(const csic_params *p, RiceGeometry *G)
{
    if (!p || !G) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    const int st = pack_geometry(p, &G->pk);
    if (st != CSIC_OK) return st;
    const PackGeometry &P = G->pk;
    csic_rice_layout &L = G->layout;
    G->max_payload_dwords = 0;
    for (int pl = 0; pl < 3; ++pl) {
        L.groups[pl] = P.layout.groups[pl];
        L.blocks[pl] = P.blocks[pl];
        L.modes_offset[pl] = P.layout.widths_offset[pl];
        L.anchors_offset[pl] = P.layout.anchors_offset[pl];
        G->max_payload_dwords += P.blocks[pl] * rice_chunk_cap(P.q[pl]);
    }
    L.directory_offset = P.layout.fixed_bytes;       // behind the anchors
    L.payload_offset = L.fixed_bytes = L.directory_offset + 4 * (P.nblocks + 1);
    L.bound_bytes = (L.fixed_bytes + 4 * G->max_payload_dwords + 255) / 256 * 256;
    if (G->max_payload_dwords >= ((int64_t)1 << 32)) return set_error(CSIC_EINVAL_SIZE, "frame too large for the Rice coding's directory");
    return CSIC_OK;
}

// a growing string of bits, LSB first in dwords
struct BitString {
    std::vector<uint32_t> w;
    int64_t bits = 0;
    void clear() { w.clear(); bits = 0; }
    void put(uint32_t v, int n)                        // the n <= 8 low bits of v
    {
        for (int i = 0; i < n; ++i, ++bits) {
            if ((bits & 31) == 0) w.push_back(0);
            w.back() |= ((v >> i) & 1u) << (bits & 31);
        }
    }
    void unary(uint32_t zeros)
    {
        for (uint32_t i = 0; i < zeros; ++i, ++bits)
            if ((bits & 31) == 0) w.push_back(0);
        put(1, 1);
    }
};

// the mode of a group with these folded residuals of w significant bits: 15, or the cheapest k = 0 .. q (q: raw), the smallest on a tie
static int choose_mode(const uint32_t u[32], int w, int q)
{
    if (w == 0) return 15;
    int best = q;
    uint32_t cost = 31u * (uint32_t)q;
    for (int k = q - 1; k >= 0; --k) {
        uint32_t c = 31u * (uint32_t)k + 31u;
        for (int j = 1; j < 32; ++j) c += u[j] >> k;
        if (c <= cost) { cost = c; best = k; }
    }
    return best;
}

int rice_pack_frame(const RiceGeometry &G, const unsigned char *frame, unsigned char *coded, size_t capacity, uint64_t *coded_bytes)
{
    const csic_rice_layout &L = G.layout;
    if (capacity < (size_t)L.fixed_bytes)
        return set_error(CSIC_EINVAL_SIZE, "a coded frame of these parameters needs at least %lld bytes, got room for %zu", (long long)L.fixed_bytes, capacity);
    std::memset(coded, 0, (size_t)L.fixed_bytes);
    unsigned char *dir = coded + L.directory_offset;
    size_t pos = (size_t)L.payload_offset;            // where the next chunk goes; keeps counting past `capacity`
    BitString R, U;
    for (int pl = 0; pl < 3; ++pl) {
        const int q = G.pk.q[pl];
        for (int64_t b = 0; b < L.blocks[pl]; ++b) {
            R.clear(); U.clear();
            const int64_t g1 = (b + 1) * RICE_BLOCK < L.groups[pl] ? (b + 1) * RICE_BLOCK : L.groups[pl];
            for (int64_t g = b * RICE_BLOCK; g < g1; ++g) {
                uint32_t c[32], u[32];
                const int w = load_group(G.pk, frame, pl, g, c, u);
                const int m = choose_mode(u, w, q);
                coded[L.modes_offset[pl] + (g >> 1)] |= (unsigned char)(m << (4 * (g & 1)));
                or_bits(coded + L.anchors_offset[pl], g * q, c[0]);
                if (m == 15) continue;
                for (int j = 1; j < 32; ++j) {
                    R.put(u[j], m);                    // (m = q: the whole u_j)
                    if (m < q) U.unary(u[j] >> m);
                }
            }
            put_u32(dir + 4 * (G.pk.block0[pl] + b), (uint32_t)((pos - (size_t)L.payload_offset) / 4));
            const size_t bytes = 4 * (R.w.size() + U.w.size());
            if (pos + bytes <= capacity) {
                unsigned char *d = coded + pos;
                for (uint32_t v : R.w) { put_u32(d, v); d += 4; }
                for (uint32_t v : U.w) { put_u32(d, v); d += 4; }
            }
            pos += bytes;
        }
    }
    put_u32(dir + 4 * G.pk.nblocks, (uint32_t)((pos - (size_t)L.payload_offset) / 4));
    *coded_bytes = pos;
    if (pos > capacity) return set_error(CSIC_EINVAL_SIZE, "this frame codes to %zu bytes, got room for %zu", pos, capacity);
    return CSIC_OK;
}

// What csic_rice_unpack_host checks before it decodes -- everything: sizes, nibbles, padding, the directory against the modes and the
// terminators, every decoded u_j.  Reads coded[0, coded_bytes) only.
int rice_check_coded(const RiceGeometry &G, const unsigned char *coded, size_t coded_bytes)
{
    const csic_rice_layout &L = G.layout;
    if (coded_bytes < (size_t)L.fixed_bytes || coded_bytes % 4 != 0 || coded_bytes > (size_t)(L.fixed_bytes + 4 * G.max_payload_dwords))
        return set_error(CSIC_EFORMAT, "a Rice-coded frame of these parameters has %lld to %lld bytes in dwords, not %zu", (long long)L.fixed_bytes,
                         (long long)(L.fixed_bytes + 4 * G.max_payload_dwords), coded_bytes);
    const unsigned char *dir = coded + L.directory_offset;
    const uint64_t total = (coded_bytes - (size_t)L.fixed_bytes) / 4;
    if (get_u32(dir) != 0 || get_u32(dir + 4 * G.pk.nblocks) != total)
        return set_error(CSIC_EFORMAT, "Rice-coded frame: the directory runs from %u to %u dwords, the frame's size says 0 to %llu", get_u32(dir),
                         get_u32(dir + 4 * G.pk.nblocks), (unsigned long long)total);
    std::vector<uint32_t> w;
    for (int pl = 0; pl < 3; ++pl) {
        const unsigned char *md = coded + L.modes_offset[pl];
        const int q = G.pk.q[pl];
        const int64_t groups = L.groups[pl];
        const int st = check_plane_sections(G.pk, coded, pl, "Rice-coded frame", "mode", [](int m, int qq) { return m <= qq || m == 15; });
        if (st != CSIC_OK) return st;
        for (int64_t b = 0; b < L.blocks[pl]; ++b) {
            const int64_t blk = G.pk.block0[pl] + b;
            const uint64_t d0 = get_u32(dir + 4 * blk), d1 = get_u32(dir + 4 * (blk + 1));
            const int64_t g0 = b * RICE_BLOCK, g1 = g0 + RICE_BLOCK < groups ? g0 + RICE_BLOCK : groups;
            int64_t rbits = 0, z = 0;
            for (int64_t g = g0; g < g1; ++g) {
                const int m = nibble_at(md, g);
                if (m != 15) { rbits += 31 * m; z += m < q; }
            }
            const uint64_t rdw = (uint64_t)((rbits + 31) / 32);
            if (d1 < d0 || d1 > total || d1 - d0 > (uint64_t)rice_chunk_cap(q) || d1 - d0 < rdw || (z == 0 && d1 - d0 != rdw))
                return set_error(CSIC_EFORMAT, "Rice-coded frame: block %lld of plane %d lies at dwords %llu to %llu; its modes need %llu for R%s",
                                 (long long)b, pl, (unsigned long long)d0, (unsigned long long)d1, (unsigned long long)rdw, z ? " and some for U" : " and none for U");
            const uint32_t nw = (uint32_t)(d1 - d0), udw = nw - (uint32_t)rdw;
            w.resize(nw);
            for (uint32_t i = 0; i < nw; ++i) w[i] = get_u32(coded + L.payload_offset + 4 * (d0 + i));     // (d1 <= total: inside coded_bytes)
            if ((rbits & 31) && (w[rdw - 1] >> (rbits & 31)))
                return set_error(CSIC_EFORMAT, "Rice-coded frame: R of block %lld of plane %d is not zero-padded", (long long)b, pl);
            if (z == 0) continue;
            int64_t ones = 0;
            for (uint32_t i = 0; i < udw; ++i) ones += __builtin_popcount(w[rdw + i]);
            if (ones != 31 * z || udw == 0 || w[nw - 1] == 0)        // (the last terminator lies in U's last dword: U is ceil(U bits / 32) dwords)
                return set_error(CSIC_EFORMAT, "Rice-coded frame: U of block %lld of plane %d holds %lld terminators in %u dwords; %lld unary groups need %lld",
                                 (long long)b, pl, (long long)ones, udw, (long long)z, (long long)(31 * z));
            uint32_t ubit = 32u * (uint32_t)rdw;
            for (int64_t g = g0; g < g1; ++g) {
                const int m = nibble_at(md, g);
                if (m >= q) continue;                  // zero and raw groups have no unary part
                for (int j = 1; j < 32; ++j) {
                    bool terminated;
                    const uint32_t zeros = rice_unary(w.data(), nw, &ubit, 32u * nw, &terminated);    // (terminated: 31 z ones were counted)
                    if (!terminated || (zeros >> (q - m)) != 0)
                        return set_error(CSIC_EFORMAT, "Rice-coded frame: slot %d of group %lld of plane %d decodes to a residual of more than %d bits", j,
                                         (long long)g, pl, q);
                }
            }
        }
    }
    return CSIC_OK;
}

int rice_unpack_frame(const RiceGeometry &G, const unsigned char *coded, size_t coded_bytes, unsigned char *frame)
{
    const int st = rice_check_coded(G, coded, coded_bytes);
    if (st != CSIC_OK) return st;
    const csic_rice_layout &L = G.layout;
    const unsigned char *dir = coded + L.directory_offset;
    std::vector<uint32_t> w;
    for (int pl = 0; pl < 3; ++pl) {
        unsigned char *dst = frame + G.pk.src_offset[pl];
        const unsigned char *md = coded + L.modes_offset[pl];
        const int q = G.pk.q[pl];
        const uint32_t mask = (1u << q) - 1u;
        const int64_t n = G.pk.n[pl], groups = L.groups[pl];
        std::memset(dst, 0, (size_t)G.pk.src_bytes[pl]);
        for (int64_t b = 0; b < L.blocks[pl]; ++b) {
            const uint64_t d0 = get_u32(dir + 4 * (G.pk.block0[pl] + b)), d1 = get_u32(dir + 4 * (G.pk.block0[pl] + b + 1));
            const int64_t g0 = b * RICE_BLOCK, g1 = g0 + RICE_BLOCK < groups ? g0 + RICE_BLOCK : groups;
            const uint32_t nw = (uint32_t)(d1 - d0);
            w.resize(nw);
            for (uint32_t i = 0; i < nw; ++i) w[i] = get_u32(coded + L.payload_offset + 4 * (d0 + i));
            int64_t rtot = 0;
            for (int64_t g = g0; g < g1; ++g) rtot += nibble_at(md, g) == 15 ? 0 : 31 * nibble_at(md, g);
            uint32_t rbit = 0, ubit = 32u * (uint32_t)((rtot + 31) / 32);        // both step through the chunk group by group
            for (int64_t g = g0; g < g1; ++g) {
                const int m = nibble_at(md, g);
                uint32_t c = code_at(coded + L.anchors_offset[pl], (groups * q + 7) / 8, g, q);
                for (int j = 0; j < 32 && 32 * g + j < n; ++j) {
                    if (j > 0 && m != 15) c = (c + rice_unfold(rice_next_u(w.data(), nw, &rbit, &ubit, 32u * nw, (uint32_t)m, (uint32_t)q), mask)) & mask;
                    or_bits(dst, (32 * g + j) * q, c);
                }
                // a ragged last group stops early: it is the chunk's last, nothing is read behind it
            }
        }
    }
    return CSIC_OK;
}

} // namespace csic

using namespace csic;

extern "C" {

int csic_rice_layout_of(const csic_params *p, csic_rice_layout *layout)
{
    return host_codec_call(!p || !layout, p, rice_geometry, "", [&](const RiceGeometry &G) { *layout = G.layout; return (int)CSIC_OK; });
}

int csic_rice_pack_host(const csic_params *p, const void *bits_frame, void *coded, size_t capacity, uint64_t *coded_bytes)
{
    return host_codec_call(!p || !bits_frame || !coded || !coded_bytes, p, rice_geometry, "out of host memory coding a frame", [&](const RiceGeometry &G) {
        return rice_pack_frame(G, static_cast<const unsigned char *>(bits_frame), static_cast<unsigned char *>(coded), capacity, coded_bytes);
    });
}

int csic_rice_unpack_host(const csic_params *p, const void *coded, size_t coded_bytes, void *bits_frame)
{
    return host_codec_call(!p || !coded || !bits_frame, p, rice_geometry, "out of host memory decoding a frame", [&](const RiceGeometry &G) {
        return rice_unpack_frame(G, static_cast<const unsigned char *>(coded), coded_bytes, static_cast<unsigned char *>(bits_frame));
    });
}

} // extern "C"
