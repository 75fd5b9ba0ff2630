// csic_pack_host.cpp -- the host codec of the group coding (csic_pack_layout_of, csic_pack_host, csic_unpack_host; host only, no device).
// The format -- groups of 32 samples, anchors, folded residuals, widths, the sections of a coded frame -- is stated in include/csic.h;
// this file is that statement written out sample by sample, with every access to the coded bytes behind a length that was checked
// first: csic_unpack_host and the container reader take bytes nobody vouches for.  pack_geometry is the one place that derives the
// groups, the nibble and anchors sections and the numbering of the 256-group blocks: the Rice coding (rice_geometry) and both device
// codecs read them from it.  The byte and bit accessors, the load of a group and the check of the sections are csic_group_host.h's,
// shared with csic_rice_host.cpp.
#include <cstring>

#include "csic_group_host.h"

namespace csic {

int pack_geometry(const csic_params *p, PackGeometry *G)
{
    if (!p || !G) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    csic_params c = *p;
    c.out_format = CSIC_FMT_PLANAR_BITS;
    int st = csic_validate(&c);                       // refuses in_format != ARGB for PLANAR_BITS
    if (st != CSIC_OK) return st;
    st = csic_planar_bits_layout_of(&c, &G->bits);
    if (st != CSIC_OK) return st;
    const csic_planar_bits_layout &B = G->bits;
    G->n[0] = (int64_t)B.geometry.y_width * B.geometry.y_height;
    G->n[1] = G->n[2] = B.geometry.chroma_samples;
    G->q[0] = B.y_bits; G->q[1] = B.cb_bits; G->q[2] = B.cr_bits;
    G->src_offset[0] = B.y_offset; G->src_offset[1] = B.cb_offset; G->src_offset[2] = B.cr_offset;
    G->src_bytes[0] = B.y_bytes; G->src_bytes[1] = B.cb_bytes; G->src_bytes[2] = B.cr_bytes;
    csic_pack_layout &L = G->layout;
    int64_t at = 0;
    G->max_payload_dwords = G->nblocks = 0;
    for (int pl = 0; pl < 3; ++pl) {
        L.groups[pl] = (G->n[pl] + 31) / 32;
        G->blocks[pl] = (L.groups[pl] + RICE_BLOCK - 1) / RICE_BLOCK;
        G->block0[pl] = G->nblocks;
        G->nblocks += G->blocks[pl];
        L.widths_offset[pl] = at;
        at += 4 * ((L.groups[pl] + 7) / 8);
        G->max_payload_dwords += L.groups[pl] * G->q[pl];
    }
    for (int pl = 0; pl < 3; ++pl) {
        L.anchors_offset[pl] = at;
        at += 4 * ((L.groups[pl] * G->q[pl] + 31) / 32);
    }
    L.payload_offset = L.fixed_bytes = at;
    L.bound_bytes = (at + 4 * G->max_payload_dwords + 255) / 256 * 256;
    return CSIC_OK;
}

// What csic_unpack_host checks before it decodes: the sizes, every nibble, every padding bit.  Reads coded[0, coded_bytes) only.
int pack_check_coded(const PackGeometry &G, const unsigned char *coded, size_t coded_bytes)
{
    const csic_pack_layout &L = G.layout;
    if (coded_bytes < (size_t)L.fixed_bytes || coded_bytes % 4 != 0 || coded_bytes > (size_t)(L.fixed_bytes + 4 * G.max_payload_dwords))
        return set_error(CSIC_EFORMAT, "a coded frame of these parameters has %lld to %lld bytes in dwords, not %zu", (long long)L.fixed_bytes,
                         (long long)(L.fixed_bytes + 4 * G.max_payload_dwords), coded_bytes);
    int64_t dwords = 0;
    for (int pl = 0; pl < 3; ++pl) {
        const int st = check_plane_sections(G, coded, pl, "coded frame", "width", [](int w, int q) { return w <= q; });
        if (st != CSIC_OK) return st;
        for (int64_t g = 0; g < L.groups[pl]; ++g) dwords += nibble_at(coded + L.widths_offset[pl], g);
    }
    if ((int64_t)coded_bytes != L.fixed_bytes + 4 * dwords)
        return set_error(CSIC_EFORMAT, "coded frame: the widths imply %lld bytes, not %zu", (long long)(L.fixed_bytes + 4 * dwords), coded_bytes);
    return CSIC_OK;
}

int pack_frame(const PackGeometry &G, const unsigned char *frame, unsigned char *coded, size_t capacity, uint64_t *coded_bytes)
{
    const csic_pack_layout &L = G.layout;
    if (capacity < (size_t)L.fixed_bytes)
        return set_error(CSIC_EINVAL_SIZE, "a coded frame of these parameters needs at least %lld bytes, got room for %zu", (long long)L.fixed_bytes, capacity);
    std::memset(coded, 0, (size_t)L.fixed_bytes);
    size_t pos = (size_t)L.payload_offset;            // where the next group's dwords go; keeps counting past `capacity`
    for (int pl = 0; pl < 3; ++pl) {
        for (int64_t g = 0; g < L.groups[pl]; ++g) {
            uint32_t c[32], u[32];
            const int w = load_group(G, frame, pl, g, c, u);
            coded[L.widths_offset[pl] + (g >> 1)] |= (unsigned char)(w << (4 * (g & 1)));
            or_bits(coded + L.anchors_offset[pl], g * G.q[pl], c[0]);
            if (pos + 4 * (size_t)w <= capacity) {
                uint64_t acc = 0;
                int fill = 0, out = 0;
                for (int j = 0; j < 32; ++j) {
                    acc |= (uint64_t)u[j] << fill;
                    fill += w;
                    if (fill >= 32) { put_u32(coded + pos + 4 * out++, (uint32_t)acc); acc >>= 32; fill -= 32; }
                }
            }
            pos += 4 * (size_t)w;
        }
    }
    *coded_bytes = pos;
    if (pos > capacity) return set_error(CSIC_EINVAL_SIZE, "this frame codes to %zu bytes, got room for %zu", pos, capacity);
    return CSIC_OK;
}

int unpack_frame(const PackGeometry &G, const unsigned char *coded, size_t coded_bytes, unsigned char *frame)
{
    const int st = pack_check_coded(G, coded, coded_bytes);
    if (st != CSIC_OK) return st;
    const csic_pack_layout &L = G.layout;
    size_t pos = (size_t)L.payload_offset;            // pos + 4 w <= coded_bytes for every group: the check above summed the widths
    for (int pl = 0; pl < 3; ++pl) {
        unsigned char *dst = frame + G.src_offset[pl];
        const int q = G.q[pl];
        const uint32_t mask = (1u << q) - 1u;
        const int64_t n = G.n[pl];
        std::memset(dst, 0, (size_t)G.src_bytes[pl]);
        for (int64_t g = 0; g < L.groups[pl]; ++g) {
            const int w = nibble_at(coded + L.widths_offset[pl], g);
            uint32_t c = code_at(coded + L.anchors_offset[pl], (L.groups[pl] * q + 7) / 8, g, q);
            const unsigned char *pay = coded + pos;
            for (int j = 0; j < 32 && 32 * g + j < n; ++j) {
                if (j > 0 && w > 0) {
                    const int bit = j * w, sh = bit & 31;
                    uint32_t u = get_u32(pay + 4 * (bit >> 5)) >> sh;
                    if (sh + w > 32) u |= get_u32(pay + 4 * (bit >> 5) + 4) << (32 - sh);      // (the next dword is one of the group's w)
                    c = (c + rice_unfold(u & ((1u << w) - 1u), mask)) & mask;
                }
                or_bits(dst, (32 * g + j) * q, c);
            }
            pos += 4 * (size_t)w;
        }
    }
    return CSIC_OK;
}

} // namespace csic

using namespace csic;

extern "C" {

int csic_pack_layout_of(const csic_params *p, csic_pack_layout *layout)
{
    return host_codec_call(!p || !layout, p, pack_geometry, "", [&](const PackGeometry &G) { *layout = G.layout; return (int)CSIC_OK; });
}

int csic_pack_host(const csic_params *p, const void *bits_frame, void *coded, size_t capacity, uint64_t *coded_bytes)
{
    return host_codec_call(!p || !bits_frame || !coded || !coded_bytes, p, pack_geometry, "out of host memory coding a frame", [&](const PackGeometry &G) {
        return pack_frame(G, static_cast<const unsigned char *>(bits_frame), static_cast<unsigned char *>(coded), capacity, coded_bytes);
    });
}

int csic_unpack_host(const csic_params *p, const void *coded, size_t coded_bytes, void *bits_frame)
{
    return host_codec_call(!p || !coded || !bits_frame, p, pack_geometry, "out of host memory decoding a frame", [&](const PackGeometry &G) {
        return unpack_frame(G, static_cast<const unsigned char *>(coded), coded_bytes, static_cast<unsigned char *>(bits_frame));
    });
}

} // extern "C"
