// csic_delta_host.cpp -- the host codec of the temporal layer (csic_delta_layout_of, csic_delta_host, csic_undelta_host; host only, no
// device).  The definition -- key and delta frames, the per-group choice between the codes and their differences against the previous
// frame, the map -- is stated in include/csic.h; this file is that statement written out sample by sample.  The groups, the payload
// ranges and the bit accessors are the group coding's (pack_geometry, csic_group_host.h).  csic_undelta_host and the container reader
// take maps nobody vouches for: delta_check_map is what they ask of one before anything is written.
// Shared with csic_mc_host.cpp, in csic_temporal_host.h: a plane's codes and the plane written back, the cost of a group and its
// differences (here at displacement 0), the layout of the map's sections, the refusals of a call and the body of the two sequence
// entry points.  What is left here defines the layer: the choice per group, the bit map and its check.
#include "csic_temporal_host.h"

namespace csic {

int delta_geometry(const csic_params *p, DeltaGeometry *G)
{
    if (!p || !G) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    const int st = pack_geometry(p, &G->pk);
    if (st != CSIC_OK) return st;
    map_sections(G->pk, 1, 0, &G->layout);
    return CSIC_OK;
}

// One frame, plane by plane: a group is its codes, or -- its map bit set -- their differences against the same group of the previous
// frame (forward: where those cost less; a tie is intra).  `out` may be `in` itself (store_codes).
template <bool FORWARD>
static void frame_pass(const DeltaGeometry &G, const unsigned char *in, const unsigned char *map_in, const unsigned char *prev, unsigned char *out,
                       unsigned char *map_out)
{
    const PackGeometry &P = G.pk;
    if (FORWARD) std::memset(map_out, 0, (size_t)G.layout.map_bytes);
    Codes c, r, plane;
    for (int pl = 0; pl < 3; ++pl) {
        const uint32_t mask = (1u << P.q[pl]) - 1u;
        const int64_t n = P.n[pl], sec = G.layout.map_offset[pl];
        plane_codes(P, in, pl, c);
        if (prev) plane_codes(P, prev, pl, r);                                 // (a key frame: its codes, and its map is not read)
        for (int64_t g = 0; prev && g < G.layout.groups[pl]; ++g) {
            const int m = group_slots(n, g);
            bool inter;
            if (FORWARD) {
                inter = group_cost(c.data(), r.data(), n, 32 * g, m, 0, mask) < group_cost(c.data(), nullptr, n, 32 * g, m, 0, mask);
                if (inter) map_out[sec + (g >> 3)] |= (unsigned char)(1u << (g & 7));
            } else
                inter = (map_in[sec + (g >> 3)] >> (g & 7)) & 1;
            if (inter) group_against(c.data(), r.data(), n, 32 * g, m, 0, FORWARD ? -1 : 1, mask, c.data());
        }
        store_codes(P, pl, c, plane, out);
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

} // namespace csic

using namespace csic;

extern "C" {

int csic_delta_layout_of(const csic_params *p, csic_delta_layout *layout)
{
    return host_codec_call(!p || !layout, p, delta_geometry, "", [&](const DeltaGeometry &G) { *layout = G.layout; return (int)CSIC_OK; });
}

int csic_delta_host(const csic_params *p, const void *frames, int32_t nframes, int32_t gop, void *diff, void *maps)
{
    // last frame first: in place, frame k - 1 is still the source when frame k is taken
    return temporal_sequence(p, frames, diff, maps, nframes, gop, delta_geometry, "out of host memory in csic_delta_host", true, true,
                             [](const DeltaGeometry &) { return (int)CSIC_OK; },
                             [](const DeltaGeometry &G, unsigned char *cur, unsigned char *prev, unsigned char *d, unsigned char *map) { delta_frame(G, cur, prev, d, map); });
}

int csic_undelta_host(const csic_params *p, const void *diff, const void *maps, int32_t nframes, int32_t gop, void *frames)
{
    return temporal_sequence(p, frames, diff, maps, nframes, gop, delta_geometry, "out of host memory in csic_undelta_host", true, false,
                             [&](const DeltaGeometry &G) { return check_maps(G, maps, nframes, gop, delta_check_map); },
                             [](const DeltaGeometry &G, unsigned char *cur, unsigned char *prev, unsigned char *d, unsigned char *map) { undelta_frame(G, d, map, prev, cur); });
}

} // extern "C"
