// csic_rows_host.cpp -- the host codec of the row-prediction layer (csic_rows_layout_of, csic_rows_host, csic_unrows_host; host only, no
// device).  The definition -- the bands, the reference one row above, the per-group choice between the codes and the running sums of
// their differences against that reference, the map -- is stated in include/csic.h; this file is that statement written out sample by
// sample.  The groups, the payload ranges and the bit accessors are the group coding's (pack_geometry, csic_group_host.h); a plane's
// codes, the layout of the map's sections, the refusals of a call and the body of the entry points are the temporal layers'
// (csic_temporal_host.h), with every frame a frame of its own (gop 1).  csic_unrows_host and the container reader take maps nobody
// vouches for: rows_check_map is what they ask of one before anything is written.
#include "csic_temporal_host.h"

namespace csic {

int rows_geometry(const csic_params *p, RowsGeometry *G)
{
    if (!p || !G) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    const int st = pack_geometry(p, &G->pk);
    if (st != CSIC_OK) return st;
    csic_rows_layout &L = G->layout;
    map_sections(G->pk, 1, 0, &L);
    for (int pl = 0; pl < 3; ++pl) {
        L.width[pl] = pl == 0 ? G->pk.bits.geometry.y_width : G->pk.bits.geometry.chroma_width;
        L.k[pl] = L.width[pl] / 32;
        L.band[pl] = 32 * L.k[pl] * ROWS_BAND;
    }
    return CSIC_OK;
}

// ref(i) of a plane of row width w and band length S, from the codes x: the sample one row above where that lies in i's band
static inline uint32_t reference(const unsigned char *x, int64_t i, int64_t w, int64_t S) { return i - w >= i / S * S ? x[i - w] : 0u; }

void rows_frame(const RowsGeometry &G, const unsigned char *frame, unsigned char *diff, unsigned char *map)
{
    const PackGeometry &P = G.pk;
    std::memset(map, 0, (size_t)G.layout.map_bytes);
    Codes x, d, plane;
    for (int pl = 0; pl < 3; ++pl) {
        const uint32_t mask = (1u << P.q[pl]) - 1u;
        const int64_t n = P.n[pl], sec = G.layout.map_offset[pl], w = G.layout.width[pl], S = G.layout.band[pl];
        plane_codes(P, frame, pl, x);
        d = x;
        for (int64_t g = 0; S > 0 && g < G.layout.groups[pl]; ++g) {
            const int m = group_slots(n, g);
            const int64_t i0 = 32 * g;
            uint32_t cost_up = 0;
            for (int j = 1; j < m; ++j) cost_up += rice_fold((x[i0 + j] - reference(x.data(), i0 + j, w, S)) & mask, mask);
            if (cost_up < group_cost(x.data(), nullptr, n, i0, m, 0, mask)) {              // a tie is 0
                map[sec + (g >> 3)] |= (unsigned char)(1u << (g & 7));
                uint32_t v = 0;
                for (int j = 0; j < m; ++j) d[i0 + j] = (unsigned char)(v = (v + x[i0 + j] - reference(x.data(), i0 + j, w, S)) & mask);
            }
        }
        store_codes(P, pl, d, plane, diff);
    }
}

// In increasing i: every reference lies in an earlier group, which holds its samples already.  `frame` may be `diff` (store_codes).
void unrows_frame(const RowsGeometry &G, const unsigned char *diff, const unsigned char *map, unsigned char *frame)
{
    const PackGeometry &P = G.pk;
    Codes x, plane;
    for (int pl = 0; pl < 3; ++pl) {
        const uint32_t mask = (1u << P.q[pl]) - 1u;
        const int64_t n = P.n[pl], sec = G.layout.map_offset[pl], w = G.layout.width[pl], S = G.layout.band[pl];
        plane_codes(P, diff, pl, x);
        for (int64_t g = 0; S > 0 && g < G.layout.groups[pl]; ++g) {
            if (!((map[sec + (g >> 3)] >> (g & 7)) & 1)) continue;
            const int m = group_slots(n, g);
            uint32_t before = 0;
            for (int j = 0; j < m; ++j) {
                const int64_t i = 32 * g + j;
                const uint32_t v = x[i];
                x[i] = (unsigned char)((v - before + reference(x.data(), i, w, S)) & mask);
                before = v;
            }
        }
        store_codes(P, pl, x, plane, frame);
    }
}

int rows_check_map(const RowsGeometry &G, const unsigned char *map, int frame)
{
    for (int pl = 0; pl < 3; ++pl) {
        const unsigned char *sec = map + G.layout.map_offset[pl];
        const int64_t groups = G.layout.groups[pl], room = (groups + 31) / 32 * 32;
        for (int64_t g = G.layout.k[pl] ? groups : 0; g < room; ++g)
            if ((sec[g >> 3] >> (g & 7)) & 1)
                return set_error(CSIC_EFORMAT, g < groups ? "frame %d: bit %lld of plane %d of its map is set, but rows of that plane are shorter than a group"
                                                          : "frame %d: padding bit %lld of plane %d of its map is set", frame, (long long)g, pl);
    }
    return CSIC_OK;
}

} // namespace csic

using namespace csic;

extern "C" {

int csic_rows_layout_of(const csic_params *p, csic_rows_layout *layout)
{
    return host_codec_call(!p || !layout, p, rows_geometry, "", [&](const RowsGeometry &G) { *layout = G.layout; return (int)CSIC_OK; });
}

int csic_rows_host(const csic_params *p, const void *frames, int32_t nframes, void *diff, void *maps)
{
    return temporal_sequence(p, frames, diff, maps, nframes, 1, rows_geometry, "out of host memory in csic_rows_host", false, false,
                             [](const RowsGeometry &) { return (int)CSIC_OK; },
                             [](const RowsGeometry &G, unsigned char *cur, unsigned char *, unsigned char *d, unsigned char *map) { rows_frame(G, cur, d, map); });
}

int csic_unrows_host(const csic_params *p, const void *diff, const void *maps, int32_t nframes, void *frames)
{
    return temporal_sequence(p, frames, diff, maps, nframes, 1, rows_geometry, "out of host memory in csic_unrows_host", true, false,
                             [&](const RowsGeometry &G) {
                                 int st = CSIC_OK;
                                 for (int32_t k = 0; k < nframes && st == CSIC_OK; ++k) st = rows_check_map(G, static_cast<const unsigned char *>(maps) + k * G.layout.map_stride, k);
                                 return st;
                             },
                             [](const RowsGeometry &G, unsigned char *cur, unsigned char *, unsigned char *d, unsigned char *map) { unrows_frame(G, d, map, cur); });
}

} // extern "C"
