// csic_group_host.h -- what the host codecs of the group coding (csic_pack_host.cpp) and of the Rice coding (csic_rice_host.cpp) share,
// header-only: the little-endian dword and bit-string accessors (csic_container.cpp uses the dwords too), the nibble read, the load of a
// group with the ragged-tail rule and its folded residuals, the validation of a plane's nibble and anchors sections, and the body of the
// extern "C" entry points.  The fold e -> u and the unfold u -> e are rice_fold and rice_unfold of csic_rice_decode.h.
#pragma once
#include <new>

#include "csic_internal.h"
#include "csic_rice_decode.h"

namespace csic {

inline uint32_t get_u32(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline void put_u32(unsigned char *p, uint32_t v) { p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); p[2] = (unsigned char)(v >> 16); p[3] = (unsigned char)(v >> 24); }

// the q bits at [i q, i q + q) of a plane of `bytes` bytes; a code that straddles two bytes has both inside the plane
inline uint32_t code_at(const unsigned char *plane, int64_t bytes, int64_t i, int q)
{
    const int64_t bit = i * q, b = bit >> 3;
    uint32_t v = plane[b];
    if (b + 1 < bytes) v |= (uint32_t)plane[b + 1] << 8;
    return (v >> (bit & 7)) & ((1u << q) - 1u);
}

// ORs a value of at most 8 bits into a zeroed bit string at bit position `bit` (both bytes lie inside the string when touched)
inline void or_bits(unsigned char *dst, int64_t bit, uint32_t v)
{
    const uint32_t s = v << (bit & 7);
    dst[bit >> 3] |= (unsigned char)s;
    if (s >> 8) dst[(bit >> 3) + 1] |= (unsigned char)(s >> 8);
}

// nibble g of a widths / modes section
inline int nibble_at(const unsigned char *nibbles, int64_t g) { return (nibbles[g >> 1] >> (4 * (g & 1))) & 15; }

// Group g of plane pl of a frame: its 32 codes c -- the slots behind the plane's last sample repeat the last real code -- and their
// folded residuals u (u[0] = 0).  c[0] is the anchor; returns w, the significant bits of the OR of u.
inline int load_group(const PackGeometry &G, const unsigned char *frame, int pl, int64_t g, uint32_t c[32], uint32_t u[32])
{
    const int q = G.q[pl];
    const uint32_t mask = (1u << q) - 1u;
    for (int j = 0; j < 32; ++j) {
        const int64_t i = 32 * g + j;
        c[j] = i < G.n[pl] ? code_at(frame + G.src_offset[pl], G.src_bytes[pl], i, q) : c[j - 1];   // (i >= n only behind a real sample of this group)
    }
    uint32_t any = 0;
    u[0] = 0;
    for (int j = 1; j < 32; ++j) {
        u[j] = rice_fold((c[j] - c[j - 1]) & mask, mask);
        any |= u[j];
    }
    int w = 0;
    while (any) { ++w; any >>= 1; }
    return w;
}

// What both *_check_coded ask of plane pl's sections: every nibble of a group is legal(nibble, q) -- the coding's rule --, the nibbles
// behind the last group and the bits behind the last anchor are 0.  `frame` and `nibble` name the coding in the messages.
inline int check_plane_sections(const PackGeometry &G, const unsigned char *coded, int pl, const char *frame, const char *nibble, bool (*legal)(int, int))
{
    const unsigned char *nb = coded + G.layout.widths_offset[pl], *an = coded + G.layout.anchors_offset[pl];
    const int q = G.q[pl];
    const int64_t groups = G.layout.groups[pl], slots = (groups + 7) / 8 * 8;
    for (int64_t g = 0; g < slots; ++g) {
        const int v = nibble_at(nb, g);
        if (g >= groups ? v != 0 : !legal(v, q))
            return set_error(CSIC_EFORMAT, "%s: %s %d of group %lld of plane %d (%d bits per code)", frame, nibble, v, (long long)g, pl, q);
    }
    const int64_t used = groups * q, room = (used + 31) / 32 * 32;
    for (int64_t bit = used; bit < room; ++bit)
        if ((an[bit >> 3] >> (bit & 7)) & 1) return set_error(CSIC_EFORMAT, "%s: the anchors of plane %d are not zero-padded", frame, pl);
    return CSIC_OK;
}

// The body of the host codecs' extern "C" entry points: the geometry of *p, then body(G) with an allocation failure caught; the error
// state is cleared on success.  `no_memory` is what CSIC_ENOMEM says.
template <class Geo, class Body>
inline int host_codec_call(bool null_argument, const csic_params *p, int (*geometry)(const csic_params *, Geo *), const char *no_memory, Body body)
{
    if (null_argument) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    Geo G;
    int st = geometry(p, &G);
    if (st != CSIC_OK) return st;
    try {
        st = body(G);
    } catch (const std::bad_alloc &) {
        return set_error(CSIC_ENOMEM, "%s", no_memory);
    }
    if (st != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

} // namespace csic
