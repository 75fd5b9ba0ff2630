// csic_mc_host.cpp -- the host codec of the motion-compensated temporal layer (csic_mc_layout_of, csic_mc_delta_host,
// csic_mc_undelta_host; host only, no device).  The definition -- displacements that clamp, the candidates and their rank, the vote, the
// table, the per-group choice, the map -- is stated in include/csic.h; this file is that statement written out sample by sample.  The
// groups, the payload ranges and the bit accessors are the group coding's (pack_geometry, csic_group_host.h).  csic_mc_undelta_host and
// the container reader take maps nobody vouches for: mc_check_map is what they ask of one before anything is written.
// Shared with csic_delta_host.cpp, in csic_temporal_host.h: a plane's codes and the plane written back, the cost of a group and its
// differences at a clamped displacement, the layout of the map's sections, the refusals of a call and the body of the two sequence
// entry points.  What is left here defines the layer: the candidates, the vote, the table, the nibble choice and mc_check_map.
#include <algorithm>

#include "csic_temporal_host.h"

namespace csic {

int mc_geometry(const csic_params *p, McGeometry *G)
{
    if (!p || !G) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    const int st = pack_geometry(p, &G->pk);
    if (st != CSIC_OK) return st;
    csic_mc_layout &L = G->layout;
    map_sections(G->pk, 4, MC_TABLE_BYTES * 3, &L);
    for (int pl = 0; pl < 3; ++pl) {
        L.width[pl] = pl == 0 ? G->pk.bits.geometry.y_width : G->pk.bits.geometry.chroma_width;
        L.table_offset[pl] = MC_TABLE_BYTES * pl;
        if (MC_MAX_RANGE * (L.width[pl] + 1) > INT32_MAX)
            return set_error(CSIC_EINVAL_SIZE, "rows of %lld samples: a displacement of %d rows does not fit 32 bits", (long long)L.width[pl], MC_MAX_RANGE);
    }
    L.workspace_frame_bytes = 3 * MC_COUNTERS * (int64_t)sizeof(uint32_t);
    return CSIC_OK;
}

int mc_candidates(int range, McCandidate *out)
{
    int n = 0;
    for (int dy = -range; dy <= range; ++dy)
        for (int dx = -range; dx <= range; ++dx) out[n++] = McCandidate{dy, dx};
    const auto l1 = [](const McCandidate &c) { return (c.dx < 0 ? -c.dx : c.dx) + (c.dy < 0 ? -c.dy : c.dy); };
    std::sort(out, out + n, [&](const McCandidate &a, const McCandidate &b) {
        if (l1(a) != l1(b)) return l1(a) < l1(b);
        return a.dy != b.dy ? a.dy < b.dy : a.dx < b.dx;
    });
    return n;
}

void mc_delta_frame(const McGeometry &G, const unsigned char *cur, const unsigned char *prev, int range, unsigned char *diff, unsigned char *map)
{
    const PackGeometry &P = G.pk;
    std::memset(map, 0, (size_t)G.layout.map_bytes);
    McCandidate cand[MC_MAX_CANDIDATES];
    const int K = mc_candidates(range, cand);
    Codes c, r, plane;
    for (int pl = 0; pl < 3; ++pl) {
        const uint32_t mask = (1u << P.q[pl]) - 1u;
        const int64_t n = P.n[pl], groups = G.layout.groups[pl];
        plane_codes(P, cur, pl, c);
        if (!prev) {                                                        // a key frame: its codes, a map of zeros
            store_codes(P, pl, c, plane, diff);
            continue;
        }
        plane_codes(P, prev, pl, r);
        int64_t s[MC_MAX_CANDIDATES], votes[MC_MAX_CANDIDATES];
        for (int k = 0; k < K; ++k) {
            s[k] = cand[k].dy * G.layout.width[pl] + cand[k].dx;
            votes[k] = 0;
        }
        // the lowest index among the cheapest of `count` displacements of group g
        const auto cheapest = [&](int64_t g, const int64_t *disp, int count, uint32_t *cost) {
            int at = 0;
            *cost = ~0u;
            for (int k = 0; k < count; ++k) {
                const uint32_t v = group_cost(c.data(), r.data(), n, 32 * g, group_slots(n, g), disp[k], mask);
                if (v < *cost) { *cost = v; at = k; }
            }
            return at;
        };
        uint32_t best;
        for (int64_t g = 0; g < groups; ++g) ++votes[cheapest(g, s, K, &best)];      // the vote: the lowest rank among the cheapest
        int order[MC_MAX_CANDIDATES], voted = 0;
        for (int k = 1; k < K; ++k)
            if (votes[k]) order[voted++] = k;
        std::stable_sort(order, order + voted, [&](int a, int b) { return votes[a] > votes[b]; });   // (stable: rank ascending within a count)
        const int T = 1 + (voted < MC_TABLE_WORDS - 2 ? voted : MC_TABLE_WORDS - 2);
        int64_t entry[MC_TABLE_WORDS] = {T, 0};
        for (int t = 2; t <= T; ++t) entry[t] = s[order[t - 2]];
        unsigned char *tab = map + G.layout.table_offset[pl], *nib = map + G.layout.map_offset[pl];
        for (int t = 0; t < MC_TABLE_WORDS; ++t) put_u32(tab + 4 * t, (uint32_t)(int32_t)entry[t]);
        for (int64_t g = 0; g < groups; ++g) {                              // the choice: the lowest t among the cheapest, against the codes
            const int m = group_slots(n, g), at = 1 + cheapest(g, entry + 1, T, &best);
            if (best < group_cost(c.data(), nullptr, n, 32 * g, m, 0, mask)) {       // a tie is intra
                nib[g >> 1] |= (unsigned char)(at << (4 * (g & 1)));
                group_against(c.data(), r.data(), n, 32 * g, m, entry[at], -1, mask, c.data());
            }
        }
        store_codes(P, pl, c, plane, diff);
    }
}

void mc_undelta_frame(const McGeometry &G, const unsigned char *diff, const unsigned char *map, const unsigned char *prev, unsigned char *cur)
{
    const PackGeometry &P = G.pk;
    Codes d, r, plane;
    for (int pl = 0; pl < 3; ++pl) {
        const uint32_t mask = (1u << P.q[pl]) - 1u;
        const int64_t n = P.n[pl];
        plane_codes(P, diff, pl, d);
        if (prev) plane_codes(P, prev, pl, r);                              // (a key frame: its codes, and its map is not read)
        const unsigned char *tab = map + G.layout.table_offset[pl], *nib = map + G.layout.map_offset[pl];
        for (int64_t g = 0; prev && g < G.layout.groups[pl]; ++g) {
            const int t = nibble_at(nib, g);
            if (t) group_against(d.data(), r.data(), n, 32 * g, group_slots(n, g), (int32_t)get_u32(tab + 4 * t), 1, mask, d.data());
        }
        store_codes(P, pl, d, plane, cur);
    }
}

int mc_check_map(const McGeometry &G, const unsigned char *map, bool key, int frame)
{
    if (key) {
        for (int64_t b = 0; b < G.layout.map_bytes; ++b)
            if (map[b]) return set_error(CSIC_EFORMAT, "frame %d is a key frame, but byte %lld of its map is not zero", frame, (long long)b);
        return CSIC_OK;
    }
    for (int pl = 0; pl < 3; ++pl) {
        const unsigned char *tab = map + G.layout.table_offset[pl], *nib = map + G.layout.map_offset[pl];
        const uint32_t T = get_u32(tab);
        if (T > MC_TABLE_WORDS - 1) return set_error(CSIC_EFORMAT, "frame %d: the table of plane %d has %u entries", frame, pl, T);
        if (T >= 1 && get_u32(tab + 4)) return set_error(CSIC_EFORMAT, "frame %d: entry 1 of the table of plane %d is not the zero vector", frame, pl);
        for (uint32_t t = T + 1; t < (uint32_t)MC_TABLE_WORDS; ++t)
            if (get_u32(tab + 4 * t)) return set_error(CSIC_EFORMAT, "frame %d: unused word %u of the table of plane %d is not zero", frame, t, pl);
        const int64_t groups = G.layout.groups[pl], room = (groups + 7) / 8 * 8;
        for (int64_t g = 0; g < room; ++g) {
            const uint32_t v = (uint32_t)nibble_at(nib, g);
            if (g >= groups ? v != 0 : v > T)
                return set_error(CSIC_EFORMAT, g < groups ? "frame %d: nibble %u of group %lld of plane %d is above the table's %u entries"
                                                          : "frame %d: padding nibble %u at %lld of plane %d is set (%u entries)", frame, v, (long long)g, pl, T);
        }
    }
    return CSIC_OK;
}

int mc_check_range(int32_t range)
{
    if (range < 0 || range > MC_MAX_RANGE) return set_error(CSIC_EINVAL_SIZE, "range must be 0..%d. Got %d", MC_MAX_RANGE, range);
    return CSIC_OK;
}

} // namespace csic

using namespace csic;

extern "C" {

int csic_mc_layout_of(const csic_params *p, csic_mc_layout *layout)
{
    return host_codec_call(!p || !layout, p, mc_geometry, "", [&](const McGeometry &G) { *layout = G.layout; return (int)CSIC_OK; });
}

int csic_mc_delta_host(const csic_params *p, const void *frames, int32_t nframes, int32_t gop, int32_t range, void *diff, void *maps)
{
    return temporal_sequence(p, frames, diff, maps, nframes, gop, mc_geometry, "out of host memory in csic_mc_delta_host", false, false,
                             [&](const McGeometry &) { return mc_check_range(range); },
                             [&](const McGeometry &G, unsigned char *cur, unsigned char *prev, unsigned char *d, unsigned char *map) { mc_delta_frame(G, cur, prev, range, d, map); });
}

int csic_mc_undelta_host(const csic_params *p, const void *diff, const void *maps, int32_t nframes, int32_t gop, void *frames)
{
    return temporal_sequence(p, frames, diff, maps, nframes, gop, mc_geometry, "out of host memory in csic_mc_undelta_host", false, false,
                             [&](const McGeometry &G) { return check_maps(G, maps, nframes, gop, mc_check_map); },
                             [](const McGeometry &G, unsigned char *cur, unsigned char *prev, unsigned char *d, unsigned char *map) { mc_undelta_frame(G, d, map, prev, cur); });
}

} // extern "C"
