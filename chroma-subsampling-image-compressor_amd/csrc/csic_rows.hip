// csic_rows.hip -- the device codec of the row-prediction layer (csic_rows_device, csic_unrows_device): CSIC_FMT_PLANAR_BITS frames to
// difference frames and maps, and back.  The definition is stated in include/csic.h; csic_rows_host.cpp is the host codec and owns the
// geometry (K, the bands) and the map's layout.
//
// A group's 32 references are the 32 samples that begin w = 32 K + delta samples before it: slots j >= delta lie in the group K groups
// back, slots j < delta in the group before that one, and a reference exists iff its group belongs to the same band (csic.h).  So a
// lane takes those one or two whole groups -- they lie in front of its own, never at the ragged end of the plane --, zeros for a group
// outside the band, and shifts the 64 samples right by 32 - delta samples into Q registers (rw_reference): delta is uniform over a
// plane, the shift is scalar.
//   k_rows<Q, NT>      the encoder; its references are SOURCE samples, so nothing depends on anything: one lane per group, 256-thread
//                      blocks of 256 consecutive groups, plane = plane0 + blockIdx.y, frame = blockIdx.z, as k_delta.  A lane loads its
//                      group and its references, forms u, both costs and both candidates in one slot loop, stores the cheaper one (a
//                      tie: the codes) through PkGroupOut; the wave's ballot is two dwords of the map, stored as k_delta stores them.
//                      No LDS, no atomics.
//   k_unrows<Q, NT>    the decoder; one workgroup per band (grid x), lane k walks the band-local groups k, K + k, 2 K + k, ... down
//                      the 16 steps (lanes loop over k when K > 256).  delta = 0 -- every width that is a multiple of 32 --: the only
//                      reference group is the one the lane decoded one step before, which it keeps in registers; no barrier, no LDS,
//                      k_undelta's loop with the steps of a band in place of the frames of a run.  delta != 0: the second reference
//                      group is the neighbour lane's, so the lanes take the steps together, one __syncthreads() per step, and read
//                      both reference groups back from the decoded frame -- the workgroup's own stores of the last two steps, which
//                      the barrier publishes inside the workgroup.  A ring in LDS would hold 2 K Q dwords and K has no bound below
//                      2^26 (a frame may be one long row), so the frame itself is the ring.  A plane with K = 0 is copied, 256
//                      groups per workgroup.
// In place (frames == diff) is safe for k_unrows: a group is read only by the lane that then writes it, and what other lanes read of
// it later is the decoded group.  k_rows reads other groups of the source: the entry point refuses any overlap.
// Every global access goes through the accessors of csic_pack_common.h and tp_map_* (csic_temporal_common.h), which the CSIC_DEBUG
// build checks.  CSIC_TUNE_NONTEMPORAL selects the accesses of the frames.
#include "csic_temporal_common.h"

namespace csic {

// TpArgs: gop is 1 (every frame stands alone), a frame is grid z
struct RwArgs : TpArgs {
    uint32_t w[3], K[3];           // a plane's row width and whole groups per row
    uint32_t bands[3];             // workgroups of k_unrows: bands, or blocks of 256 groups where K = 0
};

// far : near as one string of 64 Q-bit samples, right by 32 (Q - words) + bits bits, the low Q dwords.  `words` is one of 0 .. Q, tried in
// turn, and the dwords are taken by templates, so that every register index is a constant: a private array that is indexed by a value
// goes to scratch or to LDS.
template <int Q, int AT> __device__ __forceinline__ uint32_t rw_word(const uint32_t (&far)[Q], const uint32_t (&near)[Q])
{
    if constexpr (AT < Q) return far[AT];
    else if constexpr (AT < 2 * Q) return near[AT - Q];
    else return 0u;
}
template <int Q, int WS, int I>
__device__ __forceinline__ void rw_shift_word(const uint32_t (&far)[Q], const uint32_t (&near)[Q], uint32_t bits, uint32_t (&r)[Q])
{
    r[I] = __builtin_amdgcn_alignbit(rw_word<Q, Q - WS + I + 1>(far, near), rw_word<Q, Q - WS + I>(far, near), bits);      // (hi : lo) >> bits, bits 0 .. 31
    if constexpr (I + 1 < Q) rw_shift_word<Q, WS, I + 1>(far, near, bits, r);
}
template <int Q, int WS>
__device__ __forceinline__ void rw_shift(const uint32_t (&far)[Q], const uint32_t (&near)[Q], uint32_t words, uint32_t bits, uint32_t (&r)[Q])
{
    if (words == (uint32_t)WS) rw_shift_word<Q, WS, 0>(far, near, bits, r);        // plane-uniform
    else if constexpr (WS < Q) rw_shift<Q, WS + 1>(far, near, words, bits, r);
}

// The references of group g of a plane with K >= 1, as the Q dwords of a group, from the frame at `fb`.
template <int Q, bool NT>
__device__ __forceinline__ void rw_reference(const RwArgs &a, gpdst_t fb, int plane, uint32_t g, uint32_t (&r)[Q])
{
    const uint32_t K = a.K[plane], delta = a.w[plane] - 32u * K, local = g % ((uint32_t)CSIC_ROWS_BAND * K);
    // both groups are whole -- they lie in front of group g --: dwords, without pk_load_group's ragged path
    const int64_t base = a.off[plane] + 4 * (int64_t)(g - K) * Q;
    const bool has_near = local >= K, has_far = delta != 0u && local > K;          // slots j >= delta; slots j < delta
    uint32_t near[Q], far[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        near[i] = has_near ? pk_bits_ld4<NT>(a, fb, base + 4 * i) : 0u;
        far[i] = has_far ? pk_bits_ld4<NT>(a, fb, base + 4 * (i - Q)) : 0u;
    }
    // taken from sample 32 - delta of the 64 on
    const uint32_t sh = delta * Q, words = (sh + 31u) >> 5;
    rw_shift<Q, 0>(far, near, words, 32u * words - sh, r);
}

template <int Q, bool NT>
__global__ void __launch_bounds__(PK_T) k_rows(RwArgs a)
{
    constexpr uint32_t MASK = (1u << Q) - 1u;
    const PkArgs &e = a;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g0 = blockIdx.x * PK_T, t = threadIdx.x, g = g0 + t;
    if (g0 >= G) return;                                                    // block-uniform
    const uint32_t n = e.n[plane], f = blockIdx.z;
    const uint32_t my_dw = g0 / 32u + 2u * (t >> 6) + (t & 63u);              // lanes 0, 1 of a wave: the map dwords of its ballot
    bool up = false;
    if (g < G) {                                                            // lanes behind the last group stay for the ballot
        const gpdst_t src = tp_frame(a, a.bits, f);
        uint32_t cur[Q], ref[Q];
        pk_load_group<Q, NT>(e, src, plane, g, cur);
#pragma unroll
        for (int i = 0; i < Q; ++i) ref[i] = 0;
        if (a.K[plane] != 0u) rw_reference<Q, NT>(a, src, plane, g, ref);
        PkGroupOut<Q> ox, ov;
        uint32_t cost_left = 0, cost_up = 0, px = 0, v = 0;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            if (32u * g + (uint32_t)j < n) {                                // slots behind the last sample: no cost, zero bits
                const uint32_t x = pk_code<Q>(cur, j), u = (x - pk_code<Q>(ref, j)) & MASK;
                if (j > 0) {
                    cost_left += pk_fold<Q>((x - px) & MASK);
                    cost_up += pk_fold<Q>(u);
                }
                v = (v + u) & MASK;
                ox.put(j, x);
                ov.put(j, v);
                px = x;
            }
        }
        up = a.K[plane] != 0u && cost_up < cost_left;                       // a tie is 0
        if (up) ox = ov;
        ox.template store<NT>(e, tp_frame(a, a.diff, f), plane, g);
    }
    const unsigned long long votes = __ballot(up);
    if ((t & 63u) < 2u && my_dw < a.mdw[plane]) tp_map_st4(a, tp_map(a, f), plane, my_dw, (uint32_t)(votes >> (32u * (t & 63u))));
}

// One group of the difference frame back to its samples: its codes where `up` is clear, else x = (v_j - v_(j - 1)) + ref.
template <int Q, bool NT>
__device__ __forceinline__ void rw_decode_group(const RwArgs &a, gpdst_t src, gpdst_t dst, int plane, uint32_t g, bool up, const uint32_t (&ref)[Q], PkGroupOut<Q> &out)
{
    constexpr uint32_t MASK = (1u << Q) - 1u;
    const uint32_t n = a.n[plane];
    uint32_t cur[Q];
    pk_load_group<Q, NT>(a, src, plane, g, cur);
    uint32_t before = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        if (32u * g + (uint32_t)j < n) {
            const uint32_t v = pk_code<Q>(cur, j);
            out.put(j, up ? (v - before + pk_code<Q>(ref, j)) & MASK : v);
            before = v;
        }
    }
    out.template store<NT>(a, dst, plane, g);
}

template <int Q, bool NT>
__global__ void __launch_bounds__(PK_T) k_unrows(RwArgs a)
{
    const PkArgs &e = a;
    const int plane = e.plane0 + (int)blockIdx.y;
    if (blockIdx.x >= a.bands[plane]) return;                               // block-uniform
    const uint32_t G = e.groups[plane], K = a.K[plane], t = threadIdx.x, f = blockIdx.z;
    const gpdst_t src = tp_frame(a, a.diff, f), dst = tp_frame(a, a.bits, f), map = tp_map(a, f);
    uint32_t ref[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) ref[i] = 0;
    if (K == 0u) {                                                          // no part in the layer: the codes, whatever the map says
        const uint32_t g = blockIdx.x * PK_T + t;
        if (g < G) {
            PkGroupOut<Q> out;
            rw_decode_group<Q, NT>(a, src, dst, plane, g, false, ref, out);
        }
        return;
    }
    const uint32_t first = blockIdx.x * (uint32_t)CSIC_ROWS_BAND * K;       // the band's first group (below G: bands = ceil(G / 16 K))
    if (a.w[plane] == 32u * K) {
        for (uint32_t k = t; k < K; k += PK_T) {
#pragma unroll
            for (int i = 0; i < Q; ++i) ref[i] = 0;                         // step 0 has no reference
            for (uint32_t s = 0; s < (uint32_t)CSIC_ROWS_BAND; ++s) {
                const uint32_t g = first + s * K + k;
                if (g >= G) break;
                const bool up = (tp_map_ld4(a, map, plane, g >> 5) >> (g & 31u)) & 1u;
                PkGroupOut<Q> out;
                rw_decode_group<Q, NT>(a, src, dst, plane, g, up, ref, out);
#pragma unroll
                for (int i = 0; i < Q; ++i) ref[i] = out.d[i];
            }
        }
        return;
    }
    for (uint32_t s = 0; s < (uint32_t)CSIC_ROWS_BAND; ++s) {               // block-uniform: every lane meets every barrier
        for (uint32_t k = t; k < K; k += PK_T) {
            const uint32_t g = first + s * K + k;
            if (g >= G) break;
            const bool up = (tp_map_ld4(a, map, plane, g >> 5) >> (g & 31u)) & 1u;
            if (up) rw_reference<Q, NT>(a, dst, plane, g, ref);             // steps s - 1 and s - 2 of this workgroup, behind the barrier
            PkGroupOut<Q> out;
            rw_decode_group<Q, NT>(a, src, dst, plane, g, up, ref, out);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static const auto rows_fn = [](auto q, auto nt) { return k_rows<CSIC_CONST(q), CSIC_CONST(nt)>; };
static const auto unrows_fn = [](auto q, auto nt) { return k_unrows<CSIC_CONST(q), CSIC_CONST(nt)>; };

// What both entry points refuse before any device is touched (tp_prepare), then the layer's own arguments.
static int rows_prepare(csic_plan *plan, const void *d_frames, const void *d_diff, const void *d_maps, int32_t nframes, bool in_place_ok, const char *entry, RwArgs *a)
{
    RowsGeometry G;
    const int st = tp_prepare(plan, d_frames, d_diff, d_maps, nframes, 1, rows_geometry, in_place_ok, 1, entry, &G, a);
    if (st != CSIC_OK) return st;
    for (int p = 0; p < 3; ++p) {
        const int64_t K = G.layout.k[p], per = K ? ROWS_BAND * K : PK_T;
        a->w[p] = (uint32_t)G.layout.width[p];
        a->K[p] = (uint32_t)K;
        a->bands[p] = (uint32_t)((G.layout.groups[p] + per - 1) / per);
    }
    return CSIC_OK;
}

} // namespace csic

using namespace csic;

extern "C" {

const char *csic_rows_kernel_name(const csic_plan *plan) { return pk_kernel_name("k_rows", plan); }

int csic_rows_device(csic_plan *plan, const void *d_frames, int32_t nframes, void *d_diff, void *d_maps, void *hip_stream)
{
    RwArgs a;
    int st = rows_prepare(plan, d_frames, d_diff, d_maps, nframes, false, "csic_rows_device", &a);
    if (st != CSIC_OK) return st;
    CSIC_DEVICE_SCOPE(plan->device);
    st = pk_launch_planes(plan, a, nframes, static_cast<hipStream_t>(hip_stream), rows_fn);
    if (st != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

int csic_unrows_device(csic_plan *plan, const void *d_diff, const void *d_maps, int32_t nframes, void *d_frames, void *hip_stream)
{
    RwArgs a;
    int st = rows_prepare(plan, d_frames, d_diff, d_maps, nframes, true, "csic_unrows_device", &a);
    if (st != CSIC_OK) return st;
    CSIC_DEVICE_SCOPE(plan->device);
    // one launch per run of planes of equal width, as pk_launch_planes; grid x is the most workgroups a plane of the run has
    for (int p0 = 0; p0 < 3;) {
        int p1 = p0 + 1;
        while (p1 < 3 && a.q[p1] == a.q[p0]) ++p1;
        uint32_t most = 0;
        for (int p = p0; p < p1; ++p) most = a.bands[p] > most ? a.bands[p] : most;
        if (most > 0) {
            a.plane0 = p0;
            void (*const fn)(RwArgs) = with_const<true, false>(!plan->tune.no_nt, [&](auto nt) {
                return with_const<1, 2, 3, 4, 5, 6, 7, 8>(a.q[p0], [&](auto q) -> void (*)(RwArgs) { return unrows_fn(q, nt); });
            });
            st = launch(fn, dim3(most, (unsigned)(p1 - p0), (unsigned)nframes), dim3(PK_T, 1, 1), static_cast<hipStream_t>(hip_stream), a);
            if (st != CSIC_OK) return st;
        }
        p0 = p1;
    }
    clear_error();
    return CSIC_OK;
}

} // extern "C"
