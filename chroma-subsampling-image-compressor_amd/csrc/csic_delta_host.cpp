// csic_delta_host.cpp -- the host codec of the temporal layer (csic_delta_layout_of, csic_delta_host, csic_undelta_host; host only, no
// device).  The definition -- key and delta frames, the per-group choice between the codes and their differences against the previous
// frame, the map -- is stated in include/csic.h; this file is that statement written out sample by sample.  The groups, the payload
// ranges and the bit accessors are the group coding's (pack_geometry, csic_group_host.h).  csic_undelta_host and the container reader
// take maps nobody vouches for: delta_check_map is what they ask of one before anything is written.
#include <cstring>
#include <vector>

#include "csic_group_host.h"

namespace csic {

int delta_geometry(const csic_params *p, DeltaGeometry *G)
{
    if (!p || !G) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    const int st = pack_geometry(p, &G->pk);
    if (st != CSIC_OK) return st;
    csic_delta_layout &L = G->layout;
    int64_t at = 0;
    for (int pl = 0; pl < 3; ++pl) {
        L.groups[pl] = G->pk.layout.groups[pl];
        L.map_offset[pl] = at;
        at += 4 * ((L.groups[pl] + 31) / 32);
    }
    L.map_bytes = at;
    L.map_stride = (at + 255) / 256 * 256;
    return CSIC_OK;
}

// the sum of the folded residuals of the first `m` values of a group
static uint32_t cost_of(const uint32_t *v, int m, int q)
{
    const uint32_t mask = (1u << q) - 1u, half = 1u << (q - 1);
    uint32_t sum = 0;
    for (int j = 1; j < m; ++j) {
        const uint32_t e = (v[j] - v[j - 1]) & mask;
        sum += e < half ? 2u * e : 2u * (mask + 1u - e) - 1u;
    }
    return sum;
}

// One frame, plane by plane through a zeroed copy of the plane: `out` may be `cur` (forward) or `diff` (inverse) itself.
template <bool FORWARD>
static void frame_pass(const DeltaGeometry &G, const unsigned char *in, const unsigned char *map_in, const unsigned char *prev, unsigned char *out,
                       unsigned char *map_out)
{
    const PackGeometry &P = G.pk;
    if (FORWARD) std::memset(map_out, 0, (size_t)G.layout.map_bytes);
    std::vector<unsigned char> plane;
    for (int pl = 0; pl < 3; ++pl) {
        const int q = P.q[pl];
        const uint32_t mask = (1u << q) - 1u;
        const int64_t n = P.n[pl], bytes = P.src_bytes[pl];
        const unsigned char *src = in + P.src_offset[pl], *ref = prev ? prev + P.src_offset[pl] : nullptr;
        plane.assign((size_t)bytes, 0);
        for (int64_t g = 0; g < G.layout.groups[pl]; ++g) {
            const int m = (int)(n - 32 * g < 32 ? n - 32 * g : 32);       // the group's real slots
            uint32_t c[32], r[32], d[32];
            for (int j = 0; j < m; ++j) {
                c[j] = code_at(src, bytes, 32 * g + j, q);
                r[j] = ref ? code_at(ref, bytes, 32 * g + j, q) : 0;
            }
            bool inter;
            if (FORWARD) {
                for (int j = 0; j < m; ++j) d[j] = (c[j] - r[j]) & mask;
                inter = ref && cost_of(d, m, q) < cost_of(c, m, q);       // a tie is intra
                if (inter) map_out[G.layout.map_offset[pl] + (g >> 3)] |= (unsigned char)(1u << (g & 7));
            } else {
                inter = ref && ((map_in[G.layout.map_offset[pl] + (g >> 3)] >> (g & 7)) & 1);
                for (int j = 0; j < m; ++j) d[j] = (c[j] + r[j]) & mask;
            }
            for (int j = 0; j < m; ++j) or_bits(plane.data(), (32 * g + j) * q, inter ? d[j] : c[j]);
        }
        std::memcpy(out + P.src_offset[pl], plane.data(), (size_t)bytes);
    }
}

void delta_frame(const DeltaGeometry &G, const unsigned char *cur, const unsigned char *prev, unsigned char *diff, unsigned char *map)
{
    frame_pass<true>(G, cur, nullptr, prev, diff, map);
}

void undelta_frame(const DeltaGeometry &G, const unsigned char *diff, const unsigned char *map, const unsigned char *prev, unsigned char *cur)
{
    frame_pass<false>(G, diff, map, prev, cur, nullptr);
}

int delta_check_map(const DeltaGeometry &G, const unsigned char *map, bool key, int frame)
{
    for (int pl = 0; pl < 3; ++pl) {
        const unsigned char *sec = map + G.layout.map_offset[pl];
        const int64_t groups = G.layout.groups[pl], room = (groups + 31) / 32 * 32;
        for (int64_t g = key ? 0 : groups; g < room; ++g)
            if ((sec[g >> 3] >> (g & 7)) & 1)
                return set_error(CSIC_EFORMAT, g < groups ? "frame %d is a key frame, but bit %lld of plane %d of its map is set"
                                                          : "frame %d: padding bit %lld of plane %d of its map is set", frame, (long long)g, pl);
    }
    return CSIC_OK;
}

static bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

int delta_check_call(const DeltaGeometry &G, const void *frames, const void *diff, const void *maps, int32_t nframes, int32_t gop)
{
    if (nframes < 1 || nframes > 65535) return set_error(CSIC_EINVAL_SIZE, "nframes must be 1..65535. Got %d", nframes);
    if (gop < 1) return set_error(CSIC_EINVAL_SIZE, "gop must be at least 1. Got %d", gop);
    const size_t fb = (size_t)nframes * (size_t)G.pk.bits.frame_bytes, mb = (size_t)(nframes - 1) * (size_t)G.layout.map_stride + (size_t)G.layout.map_bytes;
    if (frames != diff && overlap(frames, fb, diff, fb))
        return set_error(CSIC_EINVAL_SIZE, "the frames and the difference frames overlap: they must be the same buffer or apart");
    if (overlap(maps, mb, frames, fb) || overlap(maps, mb, diff, fb)) return set_error(CSIC_EINVAL_SIZE, "the maps overlap the frames");
    return CSIC_OK;
}

} // namespace csic

using namespace csic;

extern "C" {

int csic_delta_layout_of(const csic_params *p, csic_delta_layout *layout)
{
    return host_codec_call(!p || !layout, p, delta_geometry, "", [&](const DeltaGeometry &G) { *layout = G.layout; return (int)CSIC_OK; });
}

int csic_delta_host(const csic_params *p, const void *frames, int32_t nframes, int32_t gop, void *diff, void *maps)
{
    return host_codec_call(!p || !frames || !diff || !maps, p, delta_geometry, "out of host memory in csic_delta_host", [&](const DeltaGeometry &G) {
        const int st = delta_check_call(G, frames, diff, maps, nframes, gop);
        if (st != CSIC_OK) return st;
        const unsigned char *x = static_cast<const unsigned char *>(frames);
        unsigned char *d = static_cast<unsigned char *>(diff), *m = static_cast<unsigned char *>(maps);
        const int64_t fb = G.pk.bits.frame_bytes;
        // last frame first: in place, frame k - 1 is still the source when frame k is taken
        for (int32_t k = nframes - 1; k >= 0; --k) delta_frame(G, x + k * fb, k % gop ? x + (k - 1) * fb : nullptr, d + k * fb, m + k * G.layout.map_stride);
        return (int)CSIC_OK;
    });
}

int csic_undelta_host(const csic_params *p, const void *diff, const void *maps, int32_t nframes, int32_t gop, void *frames)
{
    return host_codec_call(!p || !frames || !diff || !maps, p, delta_geometry, "out of host memory in csic_undelta_host", [&](const DeltaGeometry &G) {
        int st = delta_check_call(G, frames, diff, maps, nframes, gop);
        const unsigned char *d = static_cast<const unsigned char *>(diff), *m = static_cast<const unsigned char *>(maps);
        for (int32_t k = 0; k < nframes && st == CSIC_OK; ++k) st = delta_check_map(G, m + k * G.layout.map_stride, k % gop == 0, k);
        if (st != CSIC_OK) return st;
        unsigned char *x = static_cast<unsigned char *>(frames);
        const int64_t fb = G.pk.bits.frame_bytes;
        for (int32_t k = 0; k < nframes; ++k) undelta_frame(G, d + k * fb, m + k * G.layout.map_stride, k % gop ? x + (k - 1) * fb : nullptr, x + k * fb);
        return (int)CSIC_OK;
    });
}

} // extern "C"
