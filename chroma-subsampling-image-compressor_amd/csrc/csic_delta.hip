// csic_delta.hip -- the device codec of the temporal layer (csic_delta_device, csic_undelta_device): CSIC_FMT_PLANAR_BITS frames to
// difference frames and maps, and back.  The definition is stated in include/csic.h; csic_delta_host.cpp is the host codec and owns
// the map's geometry.
//
// Mapping (the codecs'): one lane per GROUP of 32 samples = Q dwords, Q a template parameter; 256-thread blocks of 256 consecutive
// groups of one plane; plane = plane0 + blockIdx.y; planes of different widths go out as separate launches.  blockIdx.z is a RUN of
// frames -- a key frame and the delta frames behind it, frames z gop .. min(z gop + gop, nframes) - 1 -- and a lane walks its group
// through the run, the previous frame's group in Q registers: sample i of frame k depends on sample i of frame k - 1 only, so there
// is no scan, no block waits for another, and each frame is read once and written once.
//   k_delta<Q, NT>     per frame: loads the group, and slot by slot cuts the code c and the previous frame's r, forms d = c - r, adds
//                      both folded residuals to the two costs and packs both candidates; stores the cheaper one (a tie: the codes)
//                      through PkGroupOut; the wave's ballot of the choices is two dwords of the map, which lanes 0 and 1 store
//                      whole (a block's first group is a multiple of 256: its 8 map dwords are aligned; a partial last block stores
//                      only the dwords the section has).  No atomics, no LDS.  A key frame stores its codes and a map of zeros.
//   k_undelta<Q, NT>   per frame: loads the difference group and the dword of the map that holds its bit, adds the previous decoded
//                      group where the bit is set, stores.  A key frame's map is not read.
// In place (diff == frames) is safe in both directions: a lane is the only reader and the only writer of its group's bytes, and it
// has the group in registers before it stores.  Slots behind a plane's last sample take no part in the costs and are stored as zero
// bits; the ragged group is loaded and stored byte by byte (pk_load_group, PkGroupOut).  Nothing is validated on the device and there
// is nothing to clamp: any map bit decodes to valid codes.
// Every global access goes through the accessors of csic_pack_common.h -- frames against frame_bytes -- and tp_map_* -- maps against
// map_bytes --, which the CSIC_DEBUG build checks.  CSIC_TUNE_NONTEMPORAL selects the accesses of the frames.
// Shared with csic_mc.hip, in csic_temporal_common.h: the argument (TpArgs), the frame and map accessors, the refusals and the filler
// of the argument (tp_prepare); this unit keeps the run walk, the slot loops and the ballot.
#include "csic_temporal_common.h"

namespace csic {

// The slot loop fuses both costs -- of the codes, and of their differences against the previous frame's group -- in one pass (one
// cut of c per slot, both candidates packed); k_mc_delta (csic_mc.hip) runs the same two loops apart, once per table entry.
template <int Q, bool NT>
__global__ void __launch_bounds__(PK_T) k_delta(TpArgs a)
{
    constexpr uint32_t MASK = (1u << Q) - 1u;
    const PkArgs &e = a;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g0 = blockIdx.x * PK_T, t = threadIdx.x, g = g0 + t;
    if (g0 >= G) return;                                                    // block-uniform
    const bool mine = g < G;                                                // lanes behind the last group stay for the ballot
    const uint32_t n = e.n[plane], f0 = blockIdx.z * (uint32_t)a.gop, f1 = min(f0 + (uint32_t)a.gop, (uint32_t)a.nframes);
    const uint32_t my_dw = g0 / 32u + 2u * (t >> 6) + (t & 63u);              // lanes 0, 1 of a wave: the map dwords of its ballot
    uint32_t prev[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) prev[i] = 0;
    for (uint32_t f = f0; f < f1; ++f) {                                    // block-uniform
        bool inter = false;
        if (mine) {
            uint32_t cur[Q];
            pk_load_group<Q, NT>(e, tp_frame(a, a.bits, f), plane, g, cur);
            PkGroupOut<Q> oc, od;
            uint32_t cost_c = 0, cost_d = 0, pc = 0, pd = 0;
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                if (32u * g + (uint32_t)j < n) {                            // slots behind the last sample: no cost, zero bits
                    const uint32_t c = pk_code<Q>(cur, j), d = (c - pk_code<Q>(prev, j)) & MASK;
                    if (j > 0) {
                        cost_c += pk_fold<Q>((c - pc) & MASK);
                        cost_d += pk_fold<Q>((d - pd) & MASK);
                    }
                    oc.put(j, c);
                    od.put(j, d);
                    pc = c;
                    pd = d;
                }
            }
            inter = f > f0 && cost_d < cost_c;                              // a tie is intra
            if (inter) oc = od;
            oc.template store<NT>(e, tp_frame(a, a.diff, f), plane, g);
#pragma unroll
            for (int i = 0; i < Q; ++i) prev[i] = cur[i];
        }
        const unsigned long long votes = __ballot(inter);
        if ((t & 63u) < 2u && my_dw < a.mdw[plane]) tp_map_st4(a, tp_map(a, f), plane, my_dw, (uint32_t)(votes >> (32u * (t & 63u))));
    }
}

// The add-back: k_delta's slot loop run the other way (same slots, same ragged-tail rule); k_mc_undelta's (csic_mc.hip) is the same.
template <int Q, bool NT>
__global__ void __launch_bounds__(PK_T) k_undelta(TpArgs a)
{
    constexpr uint32_t MASK = (1u << Q) - 1u;
    const PkArgs &e = a;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g = blockIdx.x * PK_T + threadIdx.x;
    if (g >= G) return;
    const uint32_t n = e.n[plane], f0 = blockIdx.z * (uint32_t)a.gop, f1 = min(f0 + (uint32_t)a.gop, (uint32_t)a.nframes);
    uint32_t prev[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) prev[i] = 0;
    for (uint32_t f = f0; f < f1; ++f) {
        uint32_t cur[Q];
        pk_load_group<Q, NT>(e, tp_frame(a, a.diff, f), plane, g, cur);
        const bool inter = f > f0 && ((tp_map_ld4(a, tp_map(a, f), plane, g >> 5) >> (g & 31u)) & 1u);   // a key frame's map is not read
        PkGroupOut<Q> out;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            if (32u * g + (uint32_t)j < n) {
                const uint32_t d = pk_code<Q>(cur, j);
                out.put(j, inter ? (d + pk_code<Q>(prev, j)) & MASK : d);
            }
        }
        out.template store<NT>(e, tp_frame(a, a.bits, f), plane, g);
#pragma unroll
        for (int i = 0; i < Q; ++i) prev[i] = out.d[i];
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static const auto delta_fn = [](auto q, auto nt) { return k_delta<CSIC_CONST(q), CSIC_CONST(nt)>; };
static const auto undelta_fn = [](auto q, auto nt) { return k_undelta<CSIC_CONST(q), CSIC_CONST(nt)>; };

// What both entry points refuse before any device is touched (tp_prepare), then one launch per run of planes of equal width, grid z =
// the key-frame runs.
template <class Choose>
static int delta_call(csic_plan *plan, const void *d_frames, const void *d_diff, const void *d_maps, int32_t nframes, int32_t gop, void *hip_stream,
                      const char *entry, Choose choose)
{
    DeltaGeometry G;
    TpArgs a;
    int st = tp_prepare(plan, d_frames, d_diff, d_maps, nframes, gop, delta_geometry, true, 1, entry, &G, &a);
    if (st != CSIC_OK) return st;
    CSIC_DEVICE_SCOPE(plan->device);
    st = pk_launch_planes(plan, a, (nframes + a.gop - 1) / a.gop, static_cast<hipStream_t>(hip_stream), choose);
    if (st != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

} // namespace csic

using namespace csic;

extern "C" {

const char *csic_delta_kernel_name(const csic_plan *plan) { return pk_kernel_name("k_delta", plan); }

int csic_delta_device(csic_plan *plan, const void *d_frames, int32_t nframes, int32_t gop, void *d_diff, void *d_maps, void *hip_stream)
{
    return delta_call(plan, d_frames, d_diff, d_maps, nframes, gop, hip_stream, "csic_delta_device", delta_fn);
}

int csic_undelta_device(csic_plan *plan, const void *d_diff, const void *d_maps, int32_t nframes, int32_t gop, void *d_frames, void *hip_stream)
{
    return delta_call(plan, d_frames, d_diff, d_maps, nframes, gop, hip_stream, "csic_undelta_device", undelta_fn);
}

} // extern "C"
