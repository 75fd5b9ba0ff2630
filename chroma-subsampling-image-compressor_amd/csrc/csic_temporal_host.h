// csic_temporal_host.h -- what the host codecs of the two temporal layers (csic_delta_host.cpp, csic_mc_host.cpp) share, header-only:
// a plane's codes one to a byte and the plane written back from them, the cost of a group -- of its codes, or of their differences
// against a reference at a clamped displacement (0 is the delta layer's) --, the differences themselves and their inverse, the layout
// of a map's sections, what the entry points refuse of a call (the device entry points ask the same), and the body of the four
// extern "C" sequence entry points.  What defines a layer -- its choice per group, its map, its check of a map -- stays in its unit.
#pragma once
#include <cstring>
#include <vector>

#include "csic_group_host.h"

namespace csic {

typedef std::vector<unsigned char> Codes;

// a plane's codes, one to a byte
inline void plane_codes(const PackGeometry &P, const unsigned char *frame, int pl, Codes &v)
{
    v.resize((size_t)P.n[pl]);
    for (int64_t i = 0; i < P.n[pl]; ++i) v[(size_t)i] = (unsigned char)code_at(frame + P.src_offset[pl], P.src_bytes[pl], i, P.q[pl]);
}

// The plane of `frame` from its codes, through a zeroed copy of the plane: the bits behind the last sample are stored as 0, and
// `frame` may be the frame the codes were cut from.
inline void store_codes(const PackGeometry &P, int pl, const Codes &v, Codes &plane, unsigned char *frame)
{
    plane.assign((size_t)P.src_bytes[pl], 0);
    for (int64_t i = 0; i < P.n[pl]; ++i) or_bits(plane.data(), i * P.q[pl], v[(size_t)i]);
    std::memcpy(frame + P.src_offset[pl], plane.data(), (size_t)P.src_bytes[pl]);
}

// the real slots of group g of a plane of n samples
inline int group_slots(int64_t n, int64_t g) { return (int)(n - 32 * g < 32 ? n - 32 * g : 32); }

inline int64_t clamp_sample(int64_t i, int64_t n) { return i < 0 ? 0 : i > n - 1 ? n - 1 : i; }

// The m real slots of the group at sample i0, sign = -1: out = c - r displaced by s (the differences); sign = +1: out = c + r (their
// inverse); modulo mask + 1.  `out` may be `c`, not `r`.
inline void group_against(const unsigned char *c, const unsigned char *r, int64_t n, int64_t i0, int m, int64_t s, int sign, uint32_t mask, unsigned char *out)
{
    for (int j = 0; j < m; ++j) out[i0 + j] = (unsigned char)((c[i0 + j] + (uint32_t)sign * r[clamp_sample(i0 + j + s, n)]) & mask);
}

// cost() of the m real slots of the group at sample i0: the sum of the folded residuals of the codes themselves (r == NULL), or of
// their differences against the reference displaced by s
inline uint32_t group_cost(const unsigned char *c, const unsigned char *r, int64_t n, int64_t i0, int m, int64_t s, uint32_t mask)
{
    uint32_t sum = 0, before = 0;
    for (int j = 0; j < m; ++j) {
        uint32_t v = c[i0 + j];
        if (r) v = (v - r[clamp_sample(i0 + j + s, n)]) & mask;
        if (j) sum += rice_fold((v - before) & mask, mask);
        before = v;
    }
    return sum;
}

// The sections of a map, one per plane of `bits` bits per group in whole dwords, behind `leading` bytes: fills groups[], map_offset[],
// map_bytes and map_stride of a csic_delta_layout or a csic_mc_layout.
template <class Layout> inline void map_sections(const PackGeometry &P, int bits, int64_t leading, Layout *L)
{
    int64_t at = leading;
    for (int pl = 0; pl < 3; ++pl) {
        L->groups[pl] = P.layout.groups[pl];
        L->map_offset[pl] = at;
        at += 4 * ((L->groups[pl] * bits + 31) / 32);
    }
    L->map_bytes = at;
    L->map_stride = (at + 255) / 256 * 256;
}

inline bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// What the host and the device entry points of both layers refuse of a call (NULLs are the callers'): nframes, gop, and any overlap of
// the three buffers -- other than diff == frames exactly where the layer works in place.
inline int temporal_check_call(int64_t frame_bytes, int64_t map_stride, int64_t map_bytes, const void *frames, const void *diff, const void *maps, int32_t nframes,
                               int32_t gop, bool in_place_ok)
{
    if (nframes < 1 || nframes > 65535) return set_error(CSIC_EINVAL_SIZE, "nframes must be 1..65535. Got %d", nframes);
    if (gop < 1) return set_error(CSIC_EINVAL_SIZE, "gop must be at least 1. Got %d", gop);
    const size_t fb = (size_t)nframes * (size_t)frame_bytes, mb = (size_t)(nframes - 1) * (size_t)map_stride + (size_t)map_bytes;
    if (!(in_place_ok && frames == diff) && overlap(frames, fb, diff, fb))
        return set_error(CSIC_EINVAL_SIZE, in_place_ok ? "the frames and the difference frames overlap: they must be the same buffer or apart"
                                                       : "the frames and the difference frames overlap: a group reads other groups of its reference, so not even in place");
    if (overlap(maps, mb, frames, fb) || overlap(maps, mb, diff, fb)) return set_error(CSIC_EINVAL_SIZE, "the maps overlap the frames");
    return CSIC_OK;
}
template <class Geo> inline int temporal_check_call(const Geo &G, const void *frames, const void *diff, const void *maps, int32_t nframes, int32_t gop, bool in_place_ok)
{
    return temporal_check_call(G.pk.bits.frame_bytes, G.layout.map_stride, G.layout.map_bytes, frames, diff, maps, nframes, gop, in_place_ok);
}

// The body of csic_delta_host, csic_undelta_host, csic_mc_delta_host and csic_mc_undelta_host: the NULLs, the geometry, the call,
// then ready(G) -- what else is refused before anything is written: a range, or check_maps below -- and
// step(G, frame k, frame k - 1 or NULL for a key frame, difference frame k, map k) for every frame; `last_first` walks them from the
// last to the first (the forward delta in place: frame k - 1 is still the source when frame k is taken).
template <class Geo, class Ready, class Step>
inline int temporal_sequence(const csic_params *p, const void *frames, const void *diff, const void *maps, int32_t nframes, int32_t gop,
                             int (*geometry)(const csic_params *, Geo *), const char *no_memory, bool in_place_ok, bool last_first, Ready ready, Step step)
{
    return host_codec_call(!p || !frames || !diff || !maps, p, geometry, no_memory, [&](const Geo &G) {
        int st = temporal_check_call(G, frames, diff, maps, nframes, gop, in_place_ok);
        if (st == CSIC_OK) st = ready(G);
        if (st != CSIC_OK) return st;
        unsigned char *x = static_cast<unsigned char *>(const_cast<void *>(frames)), *d = static_cast<unsigned char *>(const_cast<void *>(diff)),
                      *m = static_cast<unsigned char *>(const_cast<void *>(maps));
        const int64_t fb = G.pk.bits.frame_bytes;
        for (int32_t i = 0; i < nframes; ++i) {
            const int32_t k = last_first ? nframes - 1 - i : i;
            step(G, x + k * fb, k % gop ? x + (k - 1) * fb : nullptr, d + k * fb, m + k * G.layout.map_stride);
        }
        return (int)CSIC_OK;
    });
}

// every map of a sequence through the layer's check of one map
template <class Geo>
inline int check_maps(const Geo &G, const void *maps, int32_t nframes, int32_t gop, int (*check)(const Geo &, const unsigned char *, bool, int))
{
    int st = CSIC_OK;
    for (int32_t k = 0; k < nframes && st == CSIC_OK; ++k) st = check(G, static_cast<const unsigned char *>(maps) + k * G.layout.map_stride, k % gop == 0, k);
    return st;
}

} // namespace csic
