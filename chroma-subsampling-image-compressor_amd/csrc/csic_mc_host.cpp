// csic_mc_host.cpp -- the host codec of the motion-compensated temporal layer (csic_mc_layout_of, csic_mc_delta_host,
// csic_mc_undelta_host; host only, no device).  The definition -- displacements that clamp, the candidates and their rank, the vote, the
// table, the per-group choice, the map -- is stated in include/csic.h; this file is that statement written out sample by sample.  The
// groups, the payload ranges and the bit accessors are the group coding's (pack_geometry, csic_group_host.h).  csic_mc_undelta_host and
// the container reader take maps nobody vouches for: mc_check_map is what they ask of one before anything is written.
#include <algorithm>
#include <cstring>
#include <vector>

#include "csic_group_host.h"

namespace csic {

int mc_geometry(const csic_params *p, McGeometry *G)
{
    if (!p || !G) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    const int st = pack_geometry(p, &G->pk);
    if (st != CSIC_OK) return st;
    csic_mc_layout &L = G->layout;
    int64_t at = MC_TABLE_BYTES * 3;
    for (int pl = 0; pl < 3; ++pl) {
        L.groups[pl] = G->pk.layout.groups[pl];
        L.width[pl] = pl == 0 ? G->pk.bits.geometry.y_width : G->pk.bits.geometry.chroma_width;
        L.table_offset[pl] = MC_TABLE_BYTES * pl;
        L.map_offset[pl] = at;
        at += 4 * ((L.groups[pl] + 7) / 8);
        if (MC_MAX_RANGE * (L.width[pl] + 1) > INT32_MAX)
            return set_error(CSIC_EINVAL_SIZE, "rows of %lld samples: a displacement of %d rows does not fit 32 bits", (long long)L.width[pl], MC_MAX_RANGE);
    }
    L.map_bytes = at;
    L.map_stride = (at + 255) / 256 * 256;
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

// a plane's codes, one to a byte
static void plane_codes(const PackGeometry &P, const unsigned char *frame, int pl, std::vector<unsigned char> &v)
{
    v.resize((size_t)P.n[pl]);
    for (int64_t i = 0; i < P.n[pl]; ++i) v[(size_t)i] = (unsigned char)code_at(frame + P.src_offset[pl], P.src_bytes[pl], i, P.q[pl]);
}

// a plane's codes from one frame to another: the bits behind the last sample are stored as 0
static void copy_codes(const PackGeometry &P, const unsigned char *from, int pl, unsigned char *to, std::vector<unsigned char> &v, std::vector<unsigned char> &plane)
{
    plane_codes(P, from, pl, v);
    plane.assign((size_t)P.src_bytes[pl], 0);
    for (int64_t i = 0; i < P.n[pl]; ++i) or_bits(plane.data(), i * P.q[pl], v[(size_t)i]);
    std::memcpy(to + P.src_offset[pl], plane.data(), (size_t)P.src_bytes[pl]);
}

static inline uint32_t fold(uint32_t e, uint32_t mask, uint32_t half) { return e < half ? 2u * e : 2u * (mask + 1u - e) - 1u; }

// cost() of the m real slots of the group at sample i0: of the codes themselves (r == NULL), or of their differences against the
// reference displaced by s
static uint32_t group_cost(const unsigned char *c, const unsigned char *r, int64_t n, int64_t i0, int m, int64_t s, uint32_t mask)
{
    const uint32_t half = (mask + 1u) >> 1;
    uint32_t sum = 0, before = 0;
    for (int j = 0; j < m; ++j) {
        uint32_t v = c[i0 + j];
        if (r) {
            const int64_t at = i0 + j + s;
            v = (v - r[at < 0 ? 0 : at > n - 1 ? n - 1 : at]) & mask;
        }
        if (j) sum += fold((v - before) & mask, mask, half);
        before = v;
    }
    return sum;
}

void mc_delta_frame(const McGeometry &G, const unsigned char *cur, const unsigned char *prev, int range, unsigned char *diff, unsigned char *map)
{
    const PackGeometry &P = G.pk;
    std::memset(map, 0, (size_t)G.layout.map_bytes);
    McCandidate cand[MC_MAX_CANDIDATES];
    const int K = mc_candidates(range, cand);
    std::vector<unsigned char> c, r, plane;
    for (int pl = 0; pl < 3; ++pl) {
        const int q = P.q[pl];
        const uint32_t mask = (1u << q) - 1u;
        const int64_t n = P.n[pl], bytes = P.src_bytes[pl], groups = G.layout.groups[pl];
        if (!prev) {                                                        // a key frame: its codes, a map of zeros
            copy_codes(P, cur, pl, diff, c, plane);
            continue;
        }
        plane_codes(P, cur, pl, c);
        plane_codes(P, prev, pl, r);
        int64_t s[MC_MAX_CANDIDATES], votes[MC_MAX_CANDIDATES];
        for (int k = 0; k < K; ++k) {
            s[k] = cand[k].dy * G.layout.width[pl] + cand[k].dx;
            votes[k] = 0;
        }
        for (int64_t g = 0; g < groups; ++g) {                              // the vote: the lowest rank among the cheapest
            const int m = (int)(n - 32 * g < 32 ? n - 32 * g : 32);
            uint32_t best = ~0u;
            int at = 0;
            for (int k = 0; k < K; ++k) {
                const uint32_t cost = group_cost(c.data(), r.data(), n, 32 * g, m, s[k], mask);
                if (cost < best) { best = cost; at = k; }
            }
            ++votes[at];
        }
        int order[MC_MAX_CANDIDATES], voted = 0;
        for (int k = 1; k < K; ++k)
            if (votes[k]) order[voted++] = k;
        std::stable_sort(order, order + voted, [&](int a, int b) { return votes[a] > votes[b]; });   // (stable: rank ascending within a count)
        const int T = 1 + (voted < MC_TABLE_WORDS - 2 ? voted : MC_TABLE_WORDS - 2);
        int64_t entry[MC_TABLE_WORDS] = {T, 0};
        for (int t = 2; t <= T; ++t) entry[t] = s[order[t - 2]];
        unsigned char *tab = map + G.layout.table_offset[pl], *nib = map + G.layout.map_offset[pl];
        for (int t = 0; t < MC_TABLE_WORDS; ++t) put_u32(tab + 4 * t, (uint32_t)(int32_t)entry[t]);
        plane.assign((size_t)bytes, 0);
        for (int64_t g = 0; g < groups; ++g) {                              // the choice: the lowest t among the cheapest, against the codes
            const int m = (int)(n - 32 * g < 32 ? n - 32 * g : 32);
            uint32_t best = ~0u;
            int at = 0;
            for (int t = 1; t <= T; ++t) {
                const uint32_t cost = group_cost(c.data(), r.data(), n, 32 * g, m, entry[t], mask);
                if (cost < best) { best = cost; at = t; }
            }
            const bool inter = best < group_cost(c.data(), nullptr, n, 32 * g, m, 0, mask);   // a tie is intra
            if (inter) nib[g >> 1] |= (unsigned char)(at << (4 * (g & 1)));
            for (int j = 0; j < m; ++j) {
                const int64_t i = 32 * g + j, ri = i + entry[at];
                const uint32_t v = inter ? (c[(size_t)i] - r[(size_t)(ri < 0 ? 0 : ri > n - 1 ? n - 1 : ri)]) & mask : c[(size_t)i];
                or_bits(plane.data(), i * q, v);
            }
        }
        std::memcpy(diff + P.src_offset[pl], plane.data(), (size_t)bytes);
    }
}

void mc_undelta_frame(const McGeometry &G, const unsigned char *diff, const unsigned char *map, const unsigned char *prev, unsigned char *cur)
{
    const PackGeometry &P = G.pk;
    std::vector<unsigned char> d, r, plane;
    for (int pl = 0; pl < 3; ++pl) {
        const int q = P.q[pl];
        const uint32_t mask = (1u << q) - 1u;
        const int64_t n = P.n[pl], bytes = P.src_bytes[pl];
        if (!prev) {
            copy_codes(P, diff, pl, cur, d, plane);
            continue;
        }
        plane_codes(P, diff, pl, d);
        plane_codes(P, prev, pl, r);
        const unsigned char *tab = map + G.layout.table_offset[pl], *nib = map + G.layout.map_offset[pl];
        plane.assign((size_t)bytes, 0);
        for (int64_t i = 0; i < n; ++i) {
            const int t = nibble_at(nib, i >> 5);
            uint32_t v = d[(size_t)i];
            if (t) {
                const int64_t ri = i + (int32_t)get_u32(tab + 4 * t);
                v = (v + r[(size_t)(ri < 0 ? 0 : ri > n - 1 ? n - 1 : ri)]) & mask;
            }
            or_bits(plane.data(), i * q, v);
        }
        std::memcpy(cur + P.src_offset[pl], plane.data(), (size_t)bytes);
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

static bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

int mc_check_call(const McGeometry &G, const void *frames, const void *diff, const void *maps, int32_t nframes, int32_t gop)
{
    if (nframes < 1 || nframes > 65535) return set_error(CSIC_EINVAL_SIZE, "nframes must be 1..65535. Got %d", nframes);
    if (gop < 1) return set_error(CSIC_EINVAL_SIZE, "gop must be at least 1. Got %d", gop);
    const size_t fb = (size_t)nframes * (size_t)G.pk.bits.frame_bytes, mb = (size_t)(nframes - 1) * (size_t)G.layout.map_stride + (size_t)G.layout.map_bytes;
    if (overlap(frames, fb, diff, fb))
        return set_error(CSIC_EINVAL_SIZE, "the frames and the difference frames overlap: a group reads other groups of the previous frame, so not even in place");
    if (overlap(maps, mb, frames, fb) || overlap(maps, mb, diff, fb)) return set_error(CSIC_EINVAL_SIZE, "the maps overlap the frames");
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
    return host_codec_call(!p || !frames || !diff || !maps, p, mc_geometry, "out of host memory in csic_mc_delta_host", [&](const McGeometry &G) {
        int st = mc_check_call(G, frames, diff, maps, nframes, gop);
        if (st == CSIC_OK) st = mc_check_range(range);
        if (st != CSIC_OK) return st;
        const unsigned char *x = static_cast<const unsigned char *>(frames);
        unsigned char *d = static_cast<unsigned char *>(diff), *m = static_cast<unsigned char *>(maps);
        const int64_t fb = G.pk.bits.frame_bytes;
        for (int32_t k = 0; k < nframes; ++k) mc_delta_frame(G, x + k * fb, k % gop ? x + (k - 1) * fb : nullptr, range, d + k * fb, m + k * G.layout.map_stride);
        return (int)CSIC_OK;
    });
}

int csic_mc_undelta_host(const csic_params *p, const void *diff, const void *maps, int32_t nframes, int32_t gop, void *frames)
{
    return host_codec_call(!p || !frames || !diff || !maps, p, mc_geometry, "out of host memory in csic_mc_undelta_host", [&](const McGeometry &G) {
        int st = mc_check_call(G, frames, diff, maps, nframes, gop);
        const unsigned char *d = static_cast<const unsigned char *>(diff), *m = static_cast<const unsigned char *>(maps);
        for (int32_t k = 0; k < nframes && st == CSIC_OK; ++k) st = mc_check_map(G, m + k * G.layout.map_stride, k % gop == 0, k);
        if (st != CSIC_OK) return st;
        unsigned char *x = static_cast<unsigned char *>(frames);
        const int64_t fb = G.pk.bits.frame_bytes;
        for (int32_t k = 0; k < nframes; ++k) mc_undelta_frame(G, d + k * fb, m + k * G.layout.map_stride, k % gop ? x + (k - 1) * fb : nullptr, x + k * fb);
        return (int)CSIC_OK;
    });
}

} // extern "C"
