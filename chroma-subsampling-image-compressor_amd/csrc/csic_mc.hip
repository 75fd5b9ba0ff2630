// csic_mc.hip -- the device codec of the motion-compensated temporal layer (csic_mc_delta_device, csic_mc_undelta_device):
// CSIC_FMT_PLANAR_BITS frames to difference frames and maps, and back.  The definition is stated in include/csic.h; csic_mc_host.cpp is
// the host codec and owns the map's geometry and the refusals.
//
// Mapping (the codecs'): one lane per GROUP of 32 samples = Q dwords, Q a template parameter; 256-thread blocks of 256 consecutive
// groups of one plane; plane = plane0 + blockIdx.y; planes of different widths go out as separate launches (pk_launch_planes: the
// launches are planned here, not in the launch table).  The encoder's reference is the previous SOURCE frame, so its frames are
// independent: blockIdx.z is the frame.  The decoder's frame k needs all of the decoded frame k - 1: one launch per step of a run,
// blockIdx.z the run.
//   k_mc_clear          zeroes the vote counters of the workspace, [frame][plane][MC_COUNTERS] uint32
//   k_mc_search<Q, NT>  delta frames only: per dy the block stages the clamped reference window of its 256 groups into LDS, one code to a
//                       byte, in rows of 32 codes that are MC_ROW_DWORDS = 9 dwords apart (an odd stride, against bank conflicts); each
//                       lane prices the 2 R + 1 candidates dx of that row and keeps the best (cost, rank); block histogram in LDS, then
//                       one vector atomic per voted candidate into the frame's counters
//   k_mc_table          one wave per frame and plane: the table's 16 words from the counters (zeros for a key frame)
//   k_mc_delta<Q, NT>   per group: prices the T <= 15 table entries, stores the cheapest difference or -- a tie is intra -- the codes
//                       through PkGroupOut, and the nibbles as whole dwords (a block's first group is a multiple of 256: aligned)
//   k_mc_undelta<Q, NT> per group of frame run * gop + step; nothing is validated: a nibble reads one of the 16 words, a word clamps
// mc_ref_group is the reference of one group under one displacement: where none of the 32 indices clamps and Q + 1 dwords lie inside the
// plane, Q + 1 dwords from the unaligned bit offset and a funnel shift per dword; edge and ragged groups go sample by sample.
// Invariants: every global access goes through the accessors of csic_pack_common.h -- frames against frame_bytes --, tp_map_* /
// mc_table_* -- maps against map_bytes, a dword against its section or table -- and mc_votes below -- counters against their number --,
// which the CSIC_DEBUG build checks; the two sides of a call
// never share memory (a group reads other groups of the previous frame).  CSIC_TUNE_NONTEMPORAL selects the accesses that stream (a
// frame's own groups, the difference frames); the reference is read through the cache.  Design, bank layout, registers, measurements
// and what is untuned: DESIGN.md section 4.12.
// Shared with csic_delta.hip, in csic_temporal_common.h: the argument's base (TpArgs), the frame and map accessors, the refusals and the
// filler of the argument (tp_prepare); this unit keeps the search, the vote, the table, the displaced reference and its slot loops.
#include "csic_temporal_common.h"

namespace csic {

constexpr int MC_ROW_DWORDS = 9, MC_WIN_DWORDS = (PK_T + 1) * MC_ROW_DWORDS;   // 256 rows and the 2 R codes behind them, in a row of their own
static_assert(2 * MC_MAX_RANGE <= 32 && MC_MAX_CANDIDATES <= MC_COUNTERS && MC_COUNTERS <= PK_T, "the window's last row, the counters");

struct McArgs : TpArgs {           // moff, mdw: a plane's nibble section
    uint32_t *votes;               // the workspace: [frame][plane][MC_COUNTERS]
    uint32_t toff[3];              // byte offset of a plane's table
    int32_t width[3];              // w_p
    int32_t range;
    int32_t step;                  // k_mc_undelta: the frame of a run this launch decodes
};

// word t of a plane's table
__device__ __forceinline__ uint32_t mc_table_word(const McArgs &a, gpdst_t mb, int plane, uint32_t t) { return tp_map_word_ld4(a, mb, a.toff[plane], MC_TABLE_WORDS, t); }
__device__ __forceinline__ void mc_table_st4(const McArgs &a, gpdst_t mb, int plane, uint32_t t, uint32_t v) { tp_map_word_st4(a, mb, a.toff[plane], MC_TABLE_WORDS, t, v); }
// counter k of a frame's plane
__device__ __forceinline__ gout_t mc_votes(const McArgs &a, uint32_t f, int plane, uint32_t k)
{
    CSIC_CHECK(f < (uint32_t)a.nframes && plane >= 0 && plane < 3 && k < (uint32_t)MC_COUNTERS);
    return (gout_t)(uintptr_t)a.votes + (((uint64_t)f * 3u + (uint32_t)plane) * MC_COUNTERS + k);
}

// what ranks the candidates, packed: smaller is the lower rank
__device__ __forceinline__ uint32_t mc_rank_key(int dy, int dx) { return (uint32_t)(abs(dx) + abs(dy)) << 16 | (uint32_t)(dy + 8) << 8 | (uint32_t)(dx + 8); }

// the code of sample i of a plane, 0 <= i < n: two byte loads
template <int Q> __device__ __forceinline__ uint32_t mc_code_at(const PkArgs &e, gpdst_t fb, int plane, int64_t i)
{
    const int64_t bit = i * Q, b = bit >> 3;
    CSIC_CHECK(i >= 0 && b < e.bytes[plane]);
    uint32_t v = pk_bits_ld1(e, fb, e.off[plane] + b);
    if (b + 1 < e.bytes[plane]) v |= pk_bits_ld1(e, fb, e.off[plane] + b + 1) << 8;
    return (v >> (bit & 7)) & ((1u << Q) - 1u);
}

__device__ __forceinline__ int64_t mc_clamp(int64_t i, int64_t n) { return i < 0 ? 0 : i > n - 1 ? n - 1 : i; }

// The 32 codes r[clamp(i0 + j, 0, n - 1)], j = 0 .. 31, of a plane as the Q dwords of a group (every slot is filled: the callers
// leave out what lies behind their own plane's end).
template <int Q> __device__ __forceinline__ void mc_ref_group(const PkArgs &e, gpdst_t fb, int plane, int64_t i0, uint32_t (&r)[Q])
{
    const int64_t n = e.n[plane], bit = i0 * Q, dw = bit >> 5;
    if (i0 >= 0 && i0 + 32 <= n && 4 * (dw + Q + 1) <= e.bytes[plane]) {
        const uint32_t sh = (uint32_t)bit & 31u;
        const int64_t base = e.off[plane] + 4 * dw;
        uint32_t w[Q + 1];
#pragma unroll
        for (int i = 0; i <= Q; ++i) w[i] = pk_bits_ld4<false>(e, fb, base + 4 * i);
#pragma unroll
        for (int i = 0; i < Q; ++i) r[i] = __builtin_amdgcn_alignbit(w[i + 1], w[i], sh);
    } else {
        PkGroupOut<Q> o;
#pragma unroll
        for (int j = 0; j < 32; ++j) o.put(j, mc_code_at<Q>(e, fb, plane, mc_clamp(i0 + j, n)));
#pragma unroll
        for (int i = 0; i < Q; ++i) r[i] = o.d[i];
    }
}

// The pricing loop is k_mc_delta's loop of the differences without the packing; its reference is a row of the LDS window, one code
// to a byte, not a group's dwords.
template <int Q, bool NT>
__global__ void __launch_bounds__(PK_T) k_mc_search(McArgs a)
{
    constexpr uint32_t MASK = (1u << Q) - 1u;
    __shared__ uint32_t s_win[MC_WIN_DWORDS], s_hist[MC_COUNTERS];
    const PkArgs &e = a;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g0 = blockIdx.x * PK_T, t = threadIdx.x, g = g0 + t, f = blockIdx.z;
    if (g0 >= G || f % (uint32_t)a.gop == 0u) return;                       // block-uniform, before any barrier: key frames do not vote
    const bool mine = g < G;                                                // lanes behind the last group stay for the stage
    const int64_t n = e.n[plane];
    const int R = a.range, w = a.width[plane];
    const gpdst_t pf = tp_frame(a, a.bits, f - 1u);
    const uint8_t *s_codes = reinterpret_cast<const uint8_t *>(s_win);
    if (t < (uint32_t)MC_COUNTERS) s_hist[t] = 0;
    uint32_t cur[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) cur[i] = 0;
    if (mine) pk_load_group<Q, NT>(e, tp_frame(a, a.bits, f), plane, g, cur);
    uint32_t best_cost = ~0u, best_key = ~0u, best_at = 0;
    for (int dy = -R; dy <= R; ++dy) {                                      // block-uniform
        __syncthreads();                                                    // the window before is read (first: s_hist is zero)
        const int64_t first = 32 * (int64_t)g0 + (int64_t)dy * w - R;       // the sample at window position 0
        {
            uint32_t r[Q];
            mc_ref_group<Q>(e, pf, plane, first + 32 * (int64_t)t, r);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                s_win[MC_ROW_DWORDS * t + (uint32_t)k] = pk_code<Q>(r, 4 * k) | pk_code<Q>(r, 4 * k + 1) << 8 | pk_code<Q>(r, 4 * k + 2) << 16 | pk_code<Q>(r, 4 * k + 3) << 24;
        }
        if (t < 2u * (uint32_t)R)                                           // the 2 R codes behind the last row
            reinterpret_cast<uint8_t *>(s_win)[4 * MC_ROW_DWORDS * PK_T + t] = (uint8_t)mc_code_at<Q>(e, pf, plane, mc_clamp(first + 32 * PK_T + t, n));
        __syncthreads();
        if (mine) {
            for (int dxo = 0; dxo <= 2 * R; ++dxo) {
                uint32_t cost = 0, pd = 0;
#pragma unroll
                for (int j = 0; j < 32; ++j) {
                    if (32 * (int64_t)g + j < n) {                          // slots behind the last sample: no cost
                        const uint32_t x = (uint32_t)(j + dxo);
                        const uint32_t d = (pk_code<Q>(cur, j) - s_codes[4 * MC_ROW_DWORDS * t + x + 4u * (x >> 5)]) & MASK;
                        if (j > 0) cost += pk_fold<Q>((d - pd) & MASK);
                        pd = d;
                    }
                }
                const uint32_t key = mc_rank_key(dy, dxo - R);
                if (cost < best_cost || (cost == best_cost && key < best_key)) {
                    best_cost = cost;
                    best_key = key;
                    best_at = (uint32_t)((dy + R) * (2 * R + 1) + dxo);
                }
            }
        }
    }
    if (mine) atomicAdd(&s_hist[best_at], 1u);
    __syncthreads();
    if (t < (uint32_t)MC_COUNTERS && s_hist[t]) atomicAdd((uint32_t *)mc_votes(a, f, plane, t), s_hist[t]);
}

// grid (plane, frame), one thread per counter: the counters are cleared by a kernel
__global__ void __launch_bounds__(MC_COUNTERS) k_mc_clear(McArgs a) { *mc_votes(a, blockIdx.y, (int)blockIdx.x, threadIdx.x) = 0u; }

// grid (plane, frame), one wave
__global__ void __launch_bounds__(64) k_mc_table(McArgs a)
{
    const int plane = (int)blockIdx.x;
    const uint32_t f = blockIdx.y, lane = threadIdx.x;
    uint32_t word = 0;
    if (f % (uint32_t)a.gop != 0u) {                                        // wave-uniform
        const int R = a.range, K1 = 2 * R + 1, K = K1 * K1, w = a.width[plane];
        uint32_t v[4], key[4];
        int32_t s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int at = (int)lane + 64 * k, dy = at / K1 - R, dx = at % K1 - R;
            const bool live = at < K && (dy != 0 || dx != 0);
            v[k] = live ? *mc_votes(a, f, plane, (uint32_t)at) : 0u;
            key[k] = live ? ~mc_rank_key(dy, dx) : 0u;                      // larger is the lower rank
            s[k] = live ? dy * w + dx : 0;
        }
        uint32_t T = 1;
        for (uint32_t slot = 2; slot < (uint32_t)MC_TABLE_WORDS; ++slot) {
            uint32_t mv = 0, mk = 0;
            int32_t ms = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (v[k] > mv || (v[k] == mv && v[k] != 0u && key[k] > mk)) { mv = v[k]; mk = key[k]; ms = s[k]; }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t ov = (uint32_t)__shfl_xor((int)mv, off, 64), ok = (uint32_t)__shfl_xor((int)mk, off, 64);
                const int32_t os = __shfl_xor(ms, off, 64);
                if (ov > mv || (ov == mv && ok > mk)) { mv = ov; mk = ok; ms = os; }
            }
            if (mv == 0u) break;                                            // wave-uniform: no candidate with votes is left
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (key[k] == mk) v[k] = 0;                                 // (the keys of live candidates differ)
            if (lane == slot) word = (uint32_t)ms;
            T = slot;
        }
        if (lane == 0u) word = T;
    }
    if (lane < (uint32_t)MC_TABLE_WORDS) mc_table_st4(a, tp_map(a, f), plane, lane, word);
}

template <int Q, bool NT>
__global__ void __launch_bounds__(PK_T) k_mc_delta(McArgs a)
{
    constexpr uint32_t MASK = (1u << Q) - 1u;
    const PkArgs &e = a;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g0 = blockIdx.x * PK_T, t = threadIdx.x, g = g0 + t, f = blockIdx.z;
    if (g0 >= G) return;                                                    // block-uniform
    const int64_t n = e.n[plane];
    const gpdst_t mb = tp_map(a, f);
    uint32_t nib = 0;
    if (g < G) {                                                            // lanes behind the last group stay for the shuffles
        uint32_t cur[Q];
        pk_load_group<Q, NT>(e, tp_frame(a, a.bits, f), plane, g, cur);
        PkGroupOut<Q> out;
        uint32_t cost_c = 0, pc = 0;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            if (32 * (int64_t)g + j < n) {                                  // slots behind the last sample: no cost, zero bits
                const uint32_t c = pk_code<Q>(cur, j);
                if (j > 0) cost_c += pk_fold<Q>((c - pc) & MASK);
                out.put(j, c);
                pc = c;
            }
        }
        if (f % (uint32_t)a.gop != 0u) {
            const gpdst_t pf = tp_frame(a, a.bits, f - 1u);
            const uint32_t T = min(mc_table_word(a, mb, plane, 0), (uint32_t)MC_TABLE_WORDS - 1u);   // (k_mc_table wrote 1 .. 15)
            uint32_t best = ~0u, best_t = 0;
            PkGroupOut<Q> keep;
            for (uint32_t tt = 1; tt <= T; ++tt) {
                const int32_t s = (int32_t)mc_table_word(a, mb, plane, tt);
                uint32_t r[Q];
                mc_ref_group<Q>(e, pf, plane, 32 * (int64_t)g + s, r);
                PkGroupOut<Q> od;
                uint32_t cost_d = 0, pd = 0;
#pragma unroll
                for (int j = 0; j < 32; ++j) {
                    if (32 * (int64_t)g + j < n) {
                        const uint32_t d = (pk_code<Q>(cur, j) - pk_code<Q>(r, j)) & MASK;
                        if (j > 0) cost_d += pk_fold<Q>((d - pd) & MASK);
                        od.put(j, d);
                        pd = d;
                    }
                }
                if (cost_d < best) {                                        // the lowest t among the cheapest
                    best = cost_d;
                    best_t = tt;
                    keep = od;
                }
            }
            if (best < cost_c) {                                            // a tie is intra
                nib = best_t;
                out = keep;
            }
        }
        out.template store<NT>(e, tp_frame(a, a.diff, f), plane, g);
    }
    uint32_t v = nib;
#pragma unroll
    for (int k = 1; k < 8; ++k) v |= (uint32_t)__shfl_down((int)nib, k, 64) << (4 * k);   // (lanes 8 i .. 8 i + 7 are in one wave)
    if ((t & 7u) == 0u && (g >> 3) < a.mdw[plane]) tp_map_st4(a, mb, plane, g >> 3, v);
}

// The add-back: the loop of the differences run the other way (same slots, same ragged-tail rule), as in k_undelta (csic_delta.hip).
template <int Q, bool NT>
__global__ void __launch_bounds__(PK_T) k_mc_undelta(McArgs a)
{
    constexpr uint32_t MASK = (1u << Q) - 1u;
    const PkArgs &e = a;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g = blockIdx.x * PK_T + threadIdx.x, f = blockIdx.z * (uint32_t)a.gop + (uint32_t)a.step;
    if (g >= G || f >= (uint32_t)a.nframes) return;
    const int64_t n = e.n[plane];
    uint32_t cur[Q], r[Q];
    pk_load_group<Q, NT>(e, tp_frame(a, a.diff, f), plane, g, cur);
    uint32_t nib = 0;
    if (a.step > 0) {                                                       // a key frame's map is not read
        const gpdst_t mb = tp_map(a, f);
        nib = (tp_map_ld4(a, mb, plane, g >> 3) >> (4u * (g & 7u))) & 15u;
        if (nib) mc_ref_group<Q>(e, tp_frame(a, a.bits, f - 1u), plane, 32 * (int64_t)g + (int32_t)mc_table_word(a, mb, plane, nib), r);
    }
    if (!nib) {
#pragma unroll
        for (int i = 0; i < Q; ++i) r[i] = 0;
    }
    PkGroupOut<Q> out;
#pragma unroll
    for (int j = 0; j < 32; ++j)
        if (32 * (int64_t)g + j < n) out.put(j, (pk_code<Q>(cur, j) + pk_code<Q>(r, j)) & MASK);
    out.template store<NT>(e, tp_frame(a, a.bits, f), plane, g);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static const auto mc_search_fn = [](auto q, auto nt) { return k_mc_search<CSIC_CONST(q), CSIC_CONST(nt)>; };
static const auto mc_delta_fn = [](auto q, auto nt) { return k_mc_delta<CSIC_CONST(q), CSIC_CONST(nt)>; };
static const auto mc_undelta_fn = [](auto q, auto nt) { return k_mc_undelta<CSIC_CONST(q), CSIC_CONST(nt)>; };

// What both entry points refuse before any device is touched and the common arguments (tp_prepare), then this layer's own.
static int mc_prepare(csic_plan *plan, const void *d_frames, const void *d_diff, const void *d_maps, int32_t nframes, int32_t gop, const char *entry,
                      McGeometry *G, McArgs *a)
{
    const int st = tp_prepare(plan, d_frames, d_diff, d_maps, nframes, gop, mc_geometry, false, 4, entry, G, a);
    if (st != CSIC_OK) return st;
    a->votes = nullptr;
    for (int p = 0; p < 3; ++p) {
        a->toff[p] = (uint32_t)G->layout.table_offset[p];
        a->width[p] = (int32_t)G->layout.width[p];
    }
    a->range = 0;
    a->step = 0;
    return CSIC_OK;
}

} // namespace csic

using namespace csic;

extern "C" {

const char *csic_mc_kernel_name(const csic_plan *plan) { return pk_kernel_name("k_mc_delta", plan); }

int csic_mc_delta_device(csic_plan *plan, const void *d_frames, int32_t nframes, int32_t gop, int32_t range, void *d_diff, void *d_maps,
                         void *d_workspace, size_t workspace_bytes, void *hip_stream)
{
    McGeometry G;
    McArgs a;
    int st = mc_prepare(plan, d_frames, d_diff, d_maps, nframes, gop, "csic_mc_delta_device", &G, &a);
    if (st == CSIC_OK) st = mc_check_range(range);
    if (st != CSIC_OK) return st;
    if (!d_workspace) return set_error(CSIC_EINVAL_NULL, "d_workspace is NULL");
    const size_t need = (size_t)nframes * (size_t)G.layout.workspace_frame_bytes;
    if (workspace_bytes < need) return set_error(CSIC_EINVAL_SIZE, "workspace of %zu bytes, %d frames need %zu", workspace_bytes, nframes, need);
    if ((uintptr_t)d_workspace & 255u) return set_error(CSIC_EINVAL_SIZE, "the workspace must be 256-byte aligned");
    a.votes = static_cast<uint32_t *>(d_workspace);
    a.range = range;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    CSIC_DEVICE_SCOPE(plan->device);
    if (range > 0 && a.gop > 1) {                                           // (at range 0 the zero vector is alone: no votes to count)
        if ((st = launch(k_mc_clear, dim3(3, (unsigned)nframes, 1), dim3(MC_COUNTERS, 1, 1), stream, a)) != CSIC_OK) return st;
        if ((st = pk_launch_planes(plan, a, nframes, stream, mc_search_fn)) != CSIC_OK) return st;
    }
    if ((st = launch(k_mc_table, dim3(3, (unsigned)nframes, 1), dim3(64, 1, 1), stream, a)) != CSIC_OK) return st;
    if ((st = pk_launch_planes(plan, a, nframes, stream, mc_delta_fn)) != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

int csic_mc_undelta_device(csic_plan *plan, const void *d_diff, const void *d_maps, int32_t nframes, int32_t gop, void *d_frames, void *hip_stream)
{
    McGeometry G;
    McArgs a;
    int st = mc_prepare(plan, d_frames, d_diff, d_maps, nframes, gop, "csic_mc_undelta_device", &G, &a);
    if (st != CSIC_OK) return st;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    CSIC_DEVICE_SCOPE(plan->device);
    for (a.step = 0; a.step < a.gop; ++a.step)
        if ((st = pk_launch_planes(plan, a, (nframes - a.step + a.gop - 1) / a.gop, stream, mc_undelta_fn)) != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

} // extern "C"
