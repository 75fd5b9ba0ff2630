// csic_rans.hip -- the device codec of the rANS coding (csic_rans_pack_device, csic_rans_unpack_device): CSIC_FMT_PLANAR_BITS frames to
// coded frames and back, lossless.  The format is stated in include/csic.h; csic_rans_host.cpp is the host codec and owns the geometry.
//
// A block of the format is 1024 groups coded by 64 interleaved streams: ONE WAVE per block, lane l is stream l and walks its groups
// 1024 b + 64 i + l, i = 0 .. 15, with Q a template parameter as in the other two codecs.  The argument, the accessors, the group load
// and fold, the anchors' store and read, the repacking of a decoded group, the refusals, the per-width launches and the scan of the
// blocks' sizes are csic_pack_common.h's; block0 / nblocks of the argument are this coding's blocks, woff its tables sections.
//   pack    k_rans_clear          zeroes the counts of the workspace.
//           k_rans_hist<Q, NT>    256 lanes = 256 groups, as k_pack_widths: folds the residuals, counts them in LDS (a lane adds its
//                                 zeros in one go), adds the block's counts to the plane's in the workspace and stores its anchors.
//           k_rans_table          one wave per plane and frame: the scaling rule of csic.h on 4 symbols per lane, the table -> frame.
//           k_rans_size<Q, NT>    one wave per block runs the encoder without storing: words -> the chunk's dwords and the raw
//                                 decision -> workspace (`ws`: the dwords, `keep`: the words and the raw flag).
//           k_pack_scan           the group coding's scan: chunk offsets in place, d_sizes[frame] from the total.
//           k_rans_emit<Q, NT>    the encoder again, now with the block's word count: the chunk is assembled in LDS, the words of a
//                                 step placed from the end in ascending lane order (ballot / mbcnt); a raw chunk is ORed together
//                                 there instead.  The wave stores the chunk as consecutive dwords, lane 0 the directory entry.
//   unpack  k_rans_unpack<Q, NT>  ONE pass, no workspace: a wave reads dir[b], dir[b + 1], builds the packed (f, cum) entries and the
//                                 4096-entry slot table in LDS, copies its chunk to LDS, takes its states and walks the 496 steps;
//                                 each finished group is unfolded, prefix-summed in registers and stored.
// The decode step and the word reads of unpack are csic_rans_decode.h's, which the host codec and tests/cpp/rans_fuzz.cpp run on the
// host.  Nothing is validated on the device; instead every extent is clamped (rans_chunk_extent, rans_entry, rans_word).
// CSIC_TUNE_NONTEMPORAL selects the accesses of the PLANAR_BITS frames; the block sizes are fixed.
// Not tuned: the encoder divides by f in every step (no reciprocal table), the two encoder passes fold every group twice, a block is a
// single wave with up to 31 KiB of LDS, and the step loop is one dependent chain of look-up, multiply, ballot and word read per lane.

#include "csic_pack_common.h"
#include "csic_rans_decode.h"

namespace csic {

struct RnArgs : PkArgs {           // woff: the tables sections; block0, nblocks: blocks of 1024 groups; ws: [frame][block] chunk dwords
    uint32_t *keep;                // [frame][block]: a block's words, bit 31 = raw
    uint32_t *counts;              // [frame][plane][256]: c_s
    uint32_t dir_off;              // byte offset of the directory
    uint32_t max_dwords;           // (bound_bytes - payload_offset) / 4: no payload dword of a frame lies behind
};

template <int Q> struct RnCap { static constexpr uint32_t DW = RANS_BLOCK * 31u * Q / 32u; };      // dwords of the longest chunk: 992 Q

__device__ __forceinline__ gout_t rn_keep(const RnArgs &a, uint32_t frame, uint32_t b)
{
    CSIC_CHECK(b < a.nblocks && frame < 65535u);
    return (gout_t)(uintptr_t)a.keep + ((uint64_t)frame * a.nblocks + b);
}
__device__ __forceinline__ gout_t rn_count(const RnArgs &a, uint32_t frame, int plane, uint32_t s)
{
    CSIC_CHECK(s < 256u && plane >= 0 && plane < 3 && frame < 65535u);
    return (gout_t)(uintptr_t)a.counts + (((uint64_t)frame * 3u + (uint32_t)plane) * 256u + s);
}

__device__ __forceinline__ uint32_t rn_lanes_below(uint64_t mask)          // the set bits of mask below this lane
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ uint64_t rn_wave_max(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t rn_wave_scan(uint32_t v, uint32_t &total)      // inclusive
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, d, 64);
        if ((threadIdx.x & 63u) >= (uint32_t)d) v += t;
    }
    total = (uint32_t)__shfl((int)v, 63, 64);
    return v;
}

// The plane's stored table -> the packed entries of its 2^Q symbols in LDS (lane l: symbols 4 l .. 4 l + 3).  One wave; ends with a barrier.
template <int Q> __device__ __forceinline__ void rn_load_entries(const RnArgs &a, gpdst_t cb, int plane, uint32_t *s_e)
{
    constexpr uint32_t NSYM = 1u << Q;
    const uint32_t lane = threadIdx.x;
    uint32_t f[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k)
        if (4u * lane + 2u * k < NSYM) {
            const uint32_t v = pk_coded_ld4(a, cb, (int64_t)a.woff[plane] + 4 * (int64_t)(2u * lane + k));
            f[2 * k] = v & 0xFFFFu;
            f[2 * k + 1] = v >> 16;
        }
    const uint32_t sum = f[0] + f[1] + f[2] + f[3];
    uint32_t total;
    uint32_t cum = rn_wave_scan(sum, total) - sum;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        if (4u * lane + k < NSYM) {
            s_e[4u * lane + k] = rans_entry(f[k], cum);
            cum += f[k];
        }
    __syncthreads();
}

// One encoder step of a lane whose stream takes part (`act`): returns the ballot of the lanes that emit `word` before they code.
__device__ __forceinline__ uint64_t rn_encode_step(uint32_t &x, uint32_t entry, bool act, uint32_t &word)
{
    const uint32_t f = entry & 0xFFFFu, cum = entry >> 16;
    const bool emit = act && (x >> 20) >= f;
    word = x & 0xFFFFu;
    if (emit) x >>= 16;
    if (act) x = ((x / f) << RANS_SCALE_BITS) + x % f + cum;
    return __ballot(emit);
}

// ------------------------------------------------------------------------------------------------
// pack
// ------------------------------------------------------------------------------------------------
// One block per frame (blockIdx.z): the frame's 3 x 256 counts = 0.  A kernel and not hipMemsetAsync on purpose: with a memset node
// in front of the histogram a captured graph of this unit stalled on replay; keep the clear a kernel.
__global__ void __launch_bounds__(PK_T) k_rans_clear(RnArgs a)
{
#pragma unroll
    for (int plane = 0; plane < 3; ++plane) *rn_count(a, blockIdx.z, plane, threadIdx.x) = 0u;
}

template <int Q, bool NT>
__global__ void __launch_bounds__(PK_T) k_rans_hist(RnArgs a)
{
    constexpr uint32_t NSYM = 1u << Q;
    __shared__ uint32_t s_h[NSYM], s_a[PK_T];
    const PkArgs &e = a;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g0 = blockIdx.x * PK_T, t = threadIdx.x;
    if (g0 >= G) return;                                                    // block-uniform, before any barrier
    for (uint32_t i = t; i < NSYM; i += PK_T) s_h[i] = 0;
    __syncthreads();
    uint32_t anchor = 0;
    if (g0 + t < G) {
        uint32_t u[32], zeros = 0;
        (void)pk_fold_group<Q, NT>(e, pk_bits_frame(e), plane, g0 + t, u, anchor);
#pragma unroll
        for (int j = 1; j < 32; ++j) {
            if (u[j] == 0) ++zeros; else atomicAdd(&s_h[u[j]], 1u);
        }
        if (zeros) atomicAdd(&s_h[0], zeros);
    }
    s_a[t] = anchor;                                                        // groups behind the plane's last: 0, the section's padding
    __syncthreads();
    for (uint32_t i = t; i < NSYM; i += PK_T)
        if (s_h[i]) (void)__hip_atomic_fetch_add(rn_count(a, blockIdx.z, plane, i), s_h[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    pk_store_anchors<Q>(e, pk_coded_frame(e), plane, s_a);
}

// One wave per plane (blockIdx.x) and frame: counts -> the table of the scaling rule, into the coded frame.
__global__ void __launch_bounds__(64) k_rans_table(RnArgs a)
{
    const PkArgs &e = a;
    const int plane = (int)blockIdx.x;
    const uint32_t nsym = 1u << e.q[plane], lane = threadIdx.x;
    if (e.groups[plane] == 0) return;
    const uint64_t N = 31ull * e.groups[plane];
    uint32_t c[4], f[4], sum = 0;
    uint64_t best = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t s = 4u * lane + k;
        c[k] = s < nsym ? *rn_count(a, blockIdx.z, plane, s) : 0u;
        const uint64_t fl = (uint64_t)c[k] * RANS_M / N;
        f[k] = c[k] == 0 ? 0u : fl < 1 ? 1u : (uint32_t)fl;
        sum += f[k];
        const uint64_t key = ((uint64_t)c[k] << 8) | (255u - s);            // the largest count, the smallest s on a tie
        best = key > best ? key : best;
    }
    best = rn_wave_max(best);
    uint32_t total;
    (void)rn_wave_scan(sum, total);
    if (total < RANS_M) {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (4u * lane + k == 255u - (uint32_t)(best & 0xFFu)) f[k] += RANS_M - total;
    }
    // wave-uniform.  Counts that sum to N overshoot by less than 2^q, one per lifted floor; the bound holds whatever the workspace holds
    for (uint32_t round = 0; round < nsym && total > RANS_M; ++round, --total) {
        uint32_t top = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t key = (f[k] << 8) | (255u - (4u * lane + k));    // the largest f, the smallest s on a tie
            top = key > top ? key : top;
        }
        const uint32_t t = 255u - (uint32_t)(rn_wave_max(top) & 0xFFu);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (4u * lane + k == t) --f[k];
    }
    const gpdst_t cb = pk_coded_frame(e);
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k)
        if (4u * lane + 2u * k < nsym) pk_coded_st4(e, cb, (int64_t)e.woff[plane] + 4 * (int64_t)(2u * lane + k), f[2 * k] | (f[2 * k + 1] << 16));
}

template <int Q, bool NT>
__global__ void __launch_bounds__(64) k_rans_size(RnArgs a)
{
    __shared__ uint32_t s_e[1u << Q];
    const PkArgs &e = a;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g0 = blockIdx.x * RANS_BLOCK, lane = threadIdx.x;
    if (g0 >= G) return;
    rn_load_entries<Q>(a, pk_coded_frame(e), plane, s_e);
    uint32_t x = RANS_L, words = 0;
    for (int i = (int)RANS_ROUNDS - 1; i >= 0; --i) {
        if (g0 + RANS_LANES * (uint32_t)i >= G) continue;                   // wave-uniform
        const uint32_t g = g0 + RANS_LANES * (uint32_t)i + lane;
        const bool act = g < G;
        uint32_t u[32], anchor;
#pragma unroll
        for (int j = 0; j < 32; ++j) u[j] = 0;
        if (act) (void)pk_fold_group<Q, NT>(e, pk_bits_frame(e), plane, g, u, anchor);
#pragma unroll
        for (int j = 31; j >= 1; --j) {
            uint32_t word;
            words += (uint32_t)__popcll(rn_encode_step(x, s_e[u[j]], act, word));
        }
    }
    const uint32_t ng = min(G - g0, RANS_BLOCK), ransdw = min(ng, RANS_LANES) + (words + 1u) / 2u, rawdw = rans_raw_dwords(ng, Q);
    if (lane == 0) {
        const uint32_t blk = e.block0[plane] + blockIdx.x;
        *pk_ws(e, blockIdx.z, blk) = rawdw < ransdw ? rawdw : ransdw;
        *rn_keep(a, blockIdx.z, blk) = words | (rawdw < ransdw ? RANS_RAW_FLAG : 0u);
    }
}

template <int Q, bool NT>
__global__ void __launch_bounds__(64) k_rans_emit(RnArgs a)
{
    constexpr uint32_t CAP = RnCap<Q>::DW;
    __shared__ uint32_t s_e[1u << Q], s_chunk[CAP];
    const PkArgs &e = a;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g0 = blockIdx.x * RANS_BLOCK, lane = threadIdx.x;
    if (g0 >= G) return;
    const gpdst_t cb = pk_coded_frame(e);
    const uint32_t blk = e.block0[plane] + blockIdx.x, base = *pk_ws(e, blockIdx.z, blk), kept = *rn_keep(a, blockIdx.z, blk);
    const bool raw = (kept & RANS_RAW_FLAG) != 0;
    const uint32_t words = kept & ~RANS_RAW_FLAG, ng = min(G - g0, RANS_BLOCK), ns = min(ng, RANS_LANES);
    const uint32_t ndw = raw ? rans_raw_dwords(ng, Q) : ns + (words + 1u) / 2u;                 // <= CAP: the sizing pass took the smaller
    CSIC_CHECK(ndw <= CAP);
    for (uint32_t i = lane; i < ndw; i += RANS_LANES) s_chunk[i] = 0;
    rn_load_entries<Q>(a, cb, plane, s_e);                                                      // (its barrier publishes the zeros)
    uint32_t x = RANS_L, pos = words;
    unsigned short *s_words = reinterpret_cast<unsigned short *>(s_chunk + ns);
    for (int i = (int)RANS_ROUNDS - 1; i >= 0; --i) {
        if (g0 + RANS_LANES * (uint32_t)i >= G) continue;                   // wave-uniform
        const uint32_t gl = RANS_LANES * (uint32_t)i + lane;                // the group inside the block
        const bool act = g0 + gl < G;
        uint32_t u[32], anchor;
#pragma unroll
        for (int j = 0; j < 32; ++j) u[j] = 0;
        if (act) (void)pk_fold_group<Q, NT>(e, pk_bits_frame(e), plane, g0 + gl, u, anchor);
        if (raw) {
            if (act) {
#pragma unroll
                for (int j = 1; j < 32; ++j) {
                    const uint32_t bit = (gl * 31u + (uint32_t)(j - 1)) * Q;
                    const uint64_t v = (uint64_t)u[j] << (bit & 31u);
                    CSIC_CHECK((bit >> 5) + ((v >> 32) ? 1u : 0u) < ndw);
                    if ((uint32_t)v) atomicOr(&s_chunk[bit >> 5], (uint32_t)v);
                    if (v >> 32) atomicOr(&s_chunk[(bit >> 5) + 1u], (uint32_t)(v >> 32));
                }
            }
        } else {
#pragma unroll
            for (int j = 31; j >= 1; --j) {
                uint32_t word;
                const uint64_t mask = rn_encode_step(x, s_e[u[j]], act, word);
                const uint32_t cnt = (uint32_t)__popcll(mask);
                if ((mask >> lane) & 1u) {                                  // the step's words: the next lower positions, ascending lane order
                    const uint32_t at = pos - cnt + rn_lanes_below(mask);
                    CSIC_CHECK(cnt <= pos && at < words);
                    s_words[at] = (unsigned short)word;
                }
                pos -= cnt;
            }
        }
    }
    if (!raw && lane < ns) s_chunk[lane] = x;
    __syncthreads();
    for (uint32_t i = lane; i < ndw; i += RANS_LANES) pk_coded_st4(e, cb, e.payload_offset + 4 * ((int64_t)base + i), s_chunk[i]);
    if (lane == 0) {
        pk_coded_st4(e, cb, (int64_t)a.dir_off + 4 * (int64_t)blk, base | (raw ? RANS_RAW_FLAG : 0u));
        if (blk + 1u == e.nblocks) pk_coded_st4(e, cb, (int64_t)a.dir_off + 4 * (int64_t)e.nblocks, base + ndw);
    }
}

// ------------------------------------------------------------------------------------------------
// unpack
// ------------------------------------------------------------------------------------------------
template <int Q, bool NT>
__global__ void __launch_bounds__(64) k_rans_unpack(RnArgs a)
{
    constexpr uint32_t MASK = (1u << Q) - 1u, NSYM = 1u << Q, CAP = RnCap<Q>::DW;
    __shared__ uint32_t s_e[NSYM], s_chunk[CAP];
    __shared__ uint32_t s_slots[RANS_M / 4u];                               // the slot table: one byte per slot
    uint8_t *const s_sym = reinterpret_cast<uint8_t *>(s_slots);
    const PkArgs &e = a;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g0 = blockIdx.x * RANS_BLOCK, lane = threadIdx.x;
    if (g0 >= G) return;
    const gpdst_t cb = pk_coded_frame(e);
    const uint32_t blk = e.block0[plane] + blockIdx.x, ng = min(G - g0, RANS_BLOCK), ns = min(ng, RANS_LANES);
    // the chunk, clamped to the frame and to the block's raw size, into LDS
    uint32_t d0, nw;
    bool raw;
    rans_chunk_extent(pk_coded_ld4(e, cb, (int64_t)a.dir_off + 4 * (int64_t)blk), pk_coded_ld4(e, cb, (int64_t)a.dir_off + 4 * (int64_t)blk + 4),
                      a.max_dwords, rans_raw_dwords(ng, Q), &d0, &nw, &raw);
    for (uint32_t i = lane; i < nw; i += RANS_LANES) s_chunk[i] = pk_coded_ld4(e, cb, e.payload_offset + 4 * ((int64_t)d0 + i));
    for (uint32_t i = lane; i < RANS_M / 4u; i += RANS_LANES) s_slots[i] = 0;                   // slots no symbol claims: symbol 0
    rn_load_entries<Q>(a, cb, plane, s_e);
    if (!raw) {
        for (uint32_t s = 0; s < NSYM; ++s) {
            const uint32_t f = s_e[s] & 0xFFFFu, cum = s_e[s] >> 16;        // cum + f <= M (rans_entry)
            for (uint32_t k = lane; k < f; k += RANS_LANES) s_sym[cum + k] = (uint8_t)s;
        }
    }
    __syncthreads();
    uint32_t x = rans_dword(s_chunk, nw, lane), next = 0;
    const uint32_t segdw = nw > ns ? nw - ns : 0u;
    const uint32_t *seg = s_chunk + ns;                                     // (ns <= 64 < CAP; read through rans_word only)
    const uint32_t n = e.n[plane];
    for (uint32_t i = 0; i < RANS_ROUNDS; ++i) {
        if (g0 + RANS_LANES * i >= G) break;                                // wave-uniform
        const uint32_t gl = RANS_LANES * i + lane, g = g0 + gl;
        const bool act = g < G;
        uint32_t c = act ? pk_anchor<Q>(e, cb, plane, g) : 0u;
        PkGroupOut<Q> out;
        out.put(0, 32u * g < n ? c : 0u);
#pragma unroll
        for (int j = 1; j < 32; ++j) {
            uint32_t s = 0;
            if (raw) {
                if (act) s = rans_raw_bits(s_chunk, nw, (gl * 31u + (uint32_t)(j - 1)) * Q, Q);
            } else {
                bool refill = false;
                if (act) s = rans_decode_step(&x, s_sym, s_e, &refill) & MASK;
                const uint64_t mask = __ballot(refill);
                if (refill) rans_refill(&x, rans_word(seg, segdw, next + rn_lanes_below(mask)));
                next += (uint32_t)__popcll(mask);
            }
            c = (c + rice_unfold(s, MASK)) & MASK;
            out.put(j, 32u * g + (uint32_t)j < n ? c : 0u);                 // slots behind the last sample: zero bits
        }
        if (act) out.template store<NT>(e, pk_bits_frame(e), plane, g);
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static int fill_rn_args(const csic_plan *pl, RnArgs *a)
{
    RansGeometry G;
    int st = rans_geometry(&pl->p, &G);
    if (st != CSIC_OK) return st;
    const csic_rans_layout &L = G.layout;
    st = pk_fill_args(pl, G.pk, L.tables_offset, L.anchors_offset, L.payload_offset, L.bound_bytes, "csic_rans_pack_device", a);
    for (int p = 0; p < 3; ++p) a->block0[p] = (uint32_t)G.block0[p];
    a->nblocks = (uint32_t)G.nblocks;
    a->keep = a->counts = nullptr;
    a->dir_off = (uint32_t)L.directory_offset;
    a->max_dwords = (uint32_t)((L.bound_bytes - L.payload_offset) / 4);
    return st;
}

// the workspace: [frame][block] chunk dwords (the scan's), [frame][block] words and raw flags, [frame][plane][256] counts
static size_t rn_workspace_need(int32_t nframes, uint32_t nblocks) { return ((size_t)nframes * (2 * (size_t)nblocks + 3 * 256) * sizeof(uint32_t) + 7) / 8 * 8; }

static const auto rans_hist = [](auto q, auto nt) { return k_rans_hist<CSIC_CONST(q), CSIC_CONST(nt)>; };
static const auto rans_size = [](auto q, auto nt) { return k_rans_size<CSIC_CONST(q), CSIC_CONST(nt)>; };
static const auto rans_emit = [](auto q, auto nt) { return k_rans_emit<CSIC_CONST(q), CSIC_CONST(nt)>; };
static const auto rans_unpack = [](auto q, auto nt) { return k_rans_unpack<CSIC_CONST(q), CSIC_CONST(nt)>; };

} // namespace csic

using namespace csic;

extern "C" {

const char *csic_rans_kernel_name(const csic_plan *plan) { return pk_kernel_name("k_rans", plan); }

int csic_rans_workspace_bytes(const csic_plan *plan, int32_t nframes, size_t *bytes) { return pk_workspace_bytes(plan, nframes, bytes, fill_rn_args, rn_workspace_need); }

int csic_rans_pack_device(csic_plan *plan, const void *d_bits, int32_t nframes, void *d_coded, uint64_t *d_sizes, void *d_workspace,
                          size_t workspace_bytes, void *hip_stream)
{
    if (plan && !d_sizes) return set_error(CSIC_EINVAL_NULL, "d_sizes is NULL");
    RnArgs a;
    int st = pk_prepare(plan, d_bits, d_coded, nframes, true, d_workspace, workspace_bytes, fill_rn_args, &a, rn_workspace_need);
    if (st != CSIC_OK) return st;
    if ((uintptr_t)d_sizes & 7u) return set_error(CSIC_EINVAL_SIZE, "d_sizes must be 8-byte aligned");
    a.sizes = reinterpret_cast<unsigned long long *>(d_sizes);
    a.keep = a.ws + (size_t)nframes * a.nblocks;
    a.counts = a.keep + (size_t)nframes * a.nblocks;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    CSIC_DEVICE_SCOPE(plan->device);
    if ((st = launch(k_rans_clear, dim3(1, 1, (unsigned)nframes), dim3(PK_T, 1, 1), stream, a)) != CSIC_OK) return st;
    if ((st = pk_launch_planes(plan, a, nframes, stream, rans_hist)) != CSIC_OK) return st;
    if ((st = launch(k_rans_table, dim3(3, 1, (unsigned)nframes), dim3(RANS_LANES, 1, 1), stream, a)) != CSIC_OK) return st;
    if ((st = pk_launch_planes(plan, a, nframes, stream, rans_size, RANS_BLOCK, RANS_LANES)) != CSIC_OK) return st;
    if ((st = pack_scan_launch(a, nframes, stream)) != CSIC_OK) return st;
    if ((st = pk_launch_planes(plan, a, nframes, stream, rans_emit, RANS_BLOCK, RANS_LANES)) != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

int csic_rans_unpack_device(csic_plan *plan, const void *d_coded, int32_t nframes, void *d_bits, void *hip_stream)
{
    RnArgs a;
    int st = pk_prepare(plan, d_bits, d_coded, nframes, false, nullptr, 0, fill_rn_args, &a);
    if (st != CSIC_OK) return st;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    CSIC_DEVICE_SCOPE(plan->device);
    if ((st = pk_launch_planes(plan, a, nframes, stream, rans_unpack, RANS_BLOCK, RANS_LANES)) != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

} // extern "C"
