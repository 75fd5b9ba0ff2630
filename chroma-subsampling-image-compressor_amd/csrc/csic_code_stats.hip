// csic_code_stats.hip -- csic_code_stats_*: exact histograms of the sample codes of a compressed frame (CSIC_FMT_PLANAR or
// CSIC_FMT_PLANAR_BITS) and of their left-predicted residuals, per plane, in one pass over the compressed frame itself.  The
// definition -- codes, the predictor, storage order, the result's layout -- is in include/csic.h; the entropies and the sizes an
// entropy coder could reach are host arithmetic on these counts (compressor.py, csic.hpp).
//
// Kernels (wave64, 256-thread blocks; plane = plane0 + blockIdx.y, frame = blockIdx.z; a block counts CSTAT_BLOCK_SAMPLES = 65 536
// consecutive samples of its plane, a wave a contiguous quarter of them, so a chroma plane's blocks past its end leave at once):
//   k_cstat_bytes<NT>     CSIC_FMT_PLANAR.  A lane takes CHUNKS of 16 consecutive samples, one 16-byte load each (plane offsets are
//                      multiples of 256, so every chunk is aligned); 4 chunks per lane are in flight, lane l of a wave taking chunk
//                      c0 + 64 k + l of step k, so that a wave-instruction reads 1 KiB and a wave walks its 16 KiB in 4 rounds of 4.
//   k_cstat_bits<Q, NT>   CSIC_FMT_PLANAR_BITS, one instantiation per bit width: a lane takes GROUPS of 32 samples = exactly Q dwords
//                      (no sample straddles a lane), 4 groups in flight, 2 rounds; the codes are cut out of the dwords with
//                      compile-time shifts.  Planes of different widths go out as separate launches (Y, then Cb and Cr).
//   k_cstat_gen        either format, run-time q: one sample per lane and step, 256 steps, the predecessor loaded by the lane
//                      itself, straight from the definition.  CSIC_TUNE_FORCE_GENERIC, CSIC_TUNE_VARIANT 9 (and CSIC_TUNE_NO_VECTOR
//                      for PLANAR): the on-device cross-check of the two fast kernels.
// The predecessor of a lane's first sample in the fast kernels is the last code of the lane to its left (one ds_bpermute move); lane
// 0 takes the last code lane 63 held in the step before, and only at a wave's first step does it load the byte (the dword) in front of
// the wave's span -- nothing at sample 0, whose residual is the code itself.  A plane's last block runs the same body with every
// chunk / group tested against the plane's sample count: whole ones are loaded as above, the one the plane ends in byte by byte
// (dword by dword, up to the last dword that holds a sample), the ones beyond it not at all.
// Counting: one private pair of histograms (codes, residuals; 2 x 256 32-bit bins) per wave in LDS, 8 KiB per block, bumped with LDS
// atomics (a block's 65 536 samples cannot overflow a bin); after one barrier thread t adds the four waves' bins t and, where the sum
// is not zero, issues one 64-bit global atomic add into d_hist, which the entry point cleared with a memset on the same stream.
// Integer adds commute: the result is exact whatever the schedule.  Every global load goes through the accessors of
// csic_kernel_ops.h, which the CSIC_DEBUG build checks -- the forwards below name the limit, the frame's bytes; the flush is checked
// against the result's 3072 bins.
#include <cstdio>
#include <cstring>

#include "csic_kernel_ops.h"

namespace csic {

typedef unsigned long long CSIC_GLOBAL *gchist_t;

constexpr int CS_T = CSTAT_T, CS_WAVES = CS_T / 64;
constexpr int CS_BINS = CSIC_STATS_BINS, CS_HIST = CSIC_STATS_KINDS * CSIC_STATS_PLANES * CSIC_STATS_BINS;
constexpr int CS_K = 4;                                        // loads (chunks / groups) in flight per lane
constexpr uint32_t CS_BLOCK = (uint32_t)CSTAT_BLOCK_SAMPLES, CS_WAVE = CS_BLOCK / CS_WAVES;
static_assert(CSIC_STATS_KINDS == 2 && CSIC_STATS_BINS == 256 && CS_T == 256, "one thread per bin flushes both kinds");
static_assert(CS_WAVE % (16 * 64 * CS_K) == 0 && CS_WAVE % (32 * 64 * CS_K) == 0, "a wave's span is whole rounds of either fast kernel");

// the kernels' argument
struct CsArgs {
    const uint8_t *src;            // source frames, frame_bytes apart
    unsigned long long *hist;      // [frame][kind][plane][bin]
    int64_t frame_bytes;
    int64_t off[3];                // plane offsets
    uint32_t n[3];                 // samples per plane
    uint32_t ndw[3];               // PLANAR_BITS: dwords that hold a plane's samples
    int32_t q[3];                  // bits per code
    int32_t plane0;                // plane of blockIdx.y = 0
    int32_t bits_form;             // k_cstat_gen: 1 = PLANAR_BITS, 0 = PLANAR
};

// source: 16 bytes (16-byte aligned), a dword (4-byte aligned) or a byte at a byte offset into the frame_bytes of the frame
template <bool NT> __device__ __forceinline__ u32x4 cs_ld16(const CsArgs &e, gcbyte_t fb, int64_t off) { return by_ld16<NT>(e.frame_bytes, fb, off); }
template <bool NT> __device__ __forceinline__ uint32_t cs_ld4(const CsArgs &e, gcbyte_t fb, int64_t off) { return by_ld4<NT>(e.frame_bytes, fb, off); }
__device__ __forceinline__ uint32_t cs_ld1(const CsArgs &e, gcbyte_t fb, int64_t off) { return by_ld1(e.frame_bytes, fb, off); }

__device__ __forceinline__ gcbyte_t cs_frame(const CsArgs &e) { return frame_at_z(e.src, e.frame_bytes); }

// ------------------------------------------------------------------------------------------------
// the LDS histograms
// ------------------------------------------------------------------------------------------------
struct CsLds { uint32_t h[CS_WAVES][CSIC_STATS_KINDS][CS_BINS]; };

// clears the block's histograms and returns this wave's pair
__device__ __forceinline__ uint32_t *cs_begin(CsLds &s)
{
    uint32_t *all = &s.h[0][0][0];
#pragma unroll
    for (int i = 0; i < CS_WAVES * CSIC_STATS_KINDS; ++i) all[i * CS_BINS + threadIdx.x] = 0;
    __syncthreads();
    return &s.h[threadIdx.x >> 6][0][0];
}

// one sample: code c after code prev (0 in front of sample 0)
__device__ __forceinline__ void cs_count(uint32_t *wh, uint32_t c, uint32_t prev, uint32_t mask)
{
    __hip_atomic_fetch_add(&wh[c], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(&wh[CS_BINS + ((c - prev) & mask)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the four waves' bins -> d_hist: thread t owns bin t of both kinds
__device__ __forceinline__ void cs_flush(const CsArgs &e, CsLds &s, int plane)
{
    __syncthreads();
    const gchist_t hist = (gchist_t)(uintptr_t)e.hist;
#pragma unroll
    for (int kind = 0; kind < CSIC_STATS_KINDS; ++kind) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < CS_WAVES; ++w) t += s.h[w][kind][threadIdx.x];
        if (t) {
            const uint32_t at = (uint32_t)(kind * CSIC_STATS_PLANES + plane) * CS_BINS + threadIdx.x;
            CSIC_CHECK(at < (uint32_t)CS_HIST && blockIdx.z < 65535u);
            __hip_atomic_fetch_add(hist + ((uint64_t)blockIdx.z * CS_HIST + at), (unsigned long long)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The code in front of this lane's first sample of a step: `last` is the lane's own last code of the step, `carry` (wave-uniform)
// what was in front of the wave's first sample of the step; afterwards carry is what is in front of the next step's.
__device__ __forceinline__ uint32_t cs_pred(uint32_t last, uint32_t &carry)
{
    const uint32_t up = (uint32_t)__shfl_up((int)last, 1, 64);
    const uint32_t pred = (threadIdx.x & 63u) == 0 ? carry : up;
    carry = (uint32_t)__shfl((int)last, 63, 64);
    return pred;
}

// ------------------------------------------------------------------------------------------------
// k_cstat_bytes
// ------------------------------------------------------------------------------------------------
// chunk `ch` of a plane of n samples as four dwords: CHECK = the plane may end in or before it
template <bool NT, bool CHECK>
__device__ __forceinline__ u32x4 bytes_chunk(const CsArgs &e, gcbyte_t fb, int64_t plane_off, uint32_t ch, uint32_t n)
{
    if (!CHECK || 16u * ch + 16u <= n) return cs_ld16<NT>(e, fb, plane_off + 16 * (int64_t)ch);
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t i = 16u * ch; i < n; ++i) w[(i >> 2) & 3u] |= cs_ld1(e, fb, plane_off + i) << (8u * (i & 3u));
    return u32x4{w[0], w[1], w[2], w[3]};
}

template <bool NT, bool CHECK>
__device__ __forceinline__ void bytes_body(const CsArgs &e, gcbyte_t fb, uint32_t *wh, int plane, uint32_t i0)
{
    const uint32_t n = e.n[plane], sh = 8u - (uint32_t)e.q[plane], mask = (1u << e.q[plane]) - 1u, lane = threadIdx.x & 63u;
    const int64_t off = e.off[plane];
    // in front of the wave's span: the byte before it, nothing at sample 0 (and nothing for a wave past the plane's end)
    uint32_t carry = 0;
    if (i0 > 0 && (!CHECK || i0 < n)) carry = cs_ld1(e, fb, off + i0 - 1) >> sh;
    for (uint32_t c0 = i0 / 16u; c0 < (i0 + CS_WAVE) / 16u; c0 += 64u * CS_K) {
        if (CHECK && 16u * c0 >= n) break;                                  // wave-uniform
        u32x4 v[CS_K];
#pragma unroll
        for (int k = 0; k < CS_K; ++k) v[k] = bytes_chunk<NT, CHECK>(e, fb, off, c0 + 64u * (uint32_t)k + lane, n);
#pragma unroll
        for (int k = 0; k < CS_K; ++k) {
            const uint32_t first = 16u * (c0 + 64u * (uint32_t)k + lane);
            const uint32_t w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
            uint32_t prev = cs_pred((w[3] >> 24) >> sh, carry);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t c = ((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) >> sh;
                if (!CHECK || first + (uint32_t)j < n) cs_count(wh, c, prev, mask);
                prev = c;
            }
        }
    }
}

template <bool NT>
__global__ void __launch_bounds__(CS_T) k_cstat_bytes(CsArgs e)
{
    __shared__ CsLds lds;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t b0 = blockIdx.x * CS_BLOCK;
    if (b0 >= e.n[plane]) return;                                           // block-uniform, before any barrier
    uint32_t *wh = cs_begin(lds);
    const uint32_t i0 = b0 + (threadIdx.x >> 6) * CS_WAVE;
    if (e.n[plane] - b0 >= CS_BLOCK) bytes_body<NT, false>(e, cs_frame(e), wh, plane, i0);
    else                             bytes_body<NT, true>(e, cs_frame(e), wh, plane, i0);
    cs_flush(e, lds, plane);
}

// ------------------------------------------------------------------------------------------------
// k_cstat_bits
// ------------------------------------------------------------------------------------------------
template <int Q, bool NT, bool CHECK>
__device__ __forceinline__ void bits_body(const CsArgs &e, gcbyte_t fb, uint32_t *wh, int plane, uint32_t i0)
{
    constexpr uint32_t MASK = (1u << Q) - 1u;
    const uint32_t n = e.n[plane], ndw = e.ndw[plane], lane = threadIdx.x & 63u;
    const int64_t off = e.off[plane];
    // in front of the wave's span: the top Q bits of the dword before its first group
    uint32_t carry = 0;
    if (i0 > 0 && (!CHECK || i0 < n)) carry = cs_ld4<NT>(e, fb, off + 4 * ((int64_t)(i0 / 32u) * Q - 1)) >> (32 - Q);
    for (uint32_t g0 = i0 / 32u; g0 < (i0 + CS_WAVE) / 32u; g0 += 64u * CS_K) {
        if (CHECK && 32u * g0 >= n) break;                                  // wave-uniform
        uint32_t d[CS_K][Q];
#pragma unroll
        for (int k = 0; k < CS_K; ++k) {
            const uint32_t dw0 = (g0 + 64u * (uint32_t)k + lane) * (uint32_t)Q;     // < 2^26 * 8
#pragma unroll
            for (int i = 0; i < Q; ++i)
                d[k][i] = (!CHECK || dw0 + (uint32_t)i < ndw) ? cs_ld4<NT>(e, fb, off + 4 * (int64_t)(dw0 + (uint32_t)i)) : 0u;
        }
#pragma unroll
        for (int k = 0; k < CS_K; ++k) {
            const uint32_t first = 32u * (g0 + 64u * (uint32_t)k + lane);
            uint32_t prev = cs_pred(d[k][Q - 1] >> (32 - Q), carry);
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const int w = (j * Q) >> 5, s = (j * Q) & 31;
                uint32_t c = d[k][w] >> s;
                if (s + Q > 32) c |= d[k][(w + 1) % Q] << ((32 - s) & 31);   // (w + 1 < Q whenever a code straddles)
                c &= MASK;
                if (!CHECK || first + (uint32_t)j < n) cs_count(wh, c, prev, MASK);
                prev = c;
            }
        }
    }
}

template <int Q, bool NT>
__global__ void __launch_bounds__(CS_T) k_cstat_bits(CsArgs e)
{
    __shared__ CsLds lds;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t b0 = blockIdx.x * CS_BLOCK;
    if (b0 >= e.n[plane]) return;
    uint32_t *wh = cs_begin(lds);
    const uint32_t i0 = b0 + (threadIdx.x >> 6) * CS_WAVE;
    if (e.n[plane] - b0 >= CS_BLOCK) bits_body<Q, NT, false>(e, cs_frame(e), wh, plane, i0);
    else                             bits_body<Q, NT, true>(e, cs_frame(e), wh, plane, i0);
    cs_flush(e, lds, plane);
}

// ------------------------------------------------------------------------------------------------
// k_cstat_gen: the definition, one sample per lane and step
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t gen_code(const CsArgs &e, gcbyte_t fb, int plane, uint32_t i)
{
    const uint32_t q = (uint32_t)e.q[plane];
    if (!e.bits_form) return cs_ld1(e, fb, e.off[plane] + i) >> (8u - q);
    const uint64_t bit = (uint64_t)i * q;
    const int64_t at = e.off[plane] + 4 * (int64_t)(bit >> 5);
    const uint32_t s = (uint32_t)bit & 31u;
    const uint32_t lo = cs_ld4<false>(e, fb, at), hi = s + q > 32u ? cs_ld4<false>(e, fb, at + 4) : 0u;
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> s) & ((1u << q) - 1u);
}

__global__ void __launch_bounds__(CS_T) k_cstat_gen(CsArgs e)
{
    __shared__ CsLds lds;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t b0 = blockIdx.x * CS_BLOCK, n = e.n[plane];
    if (b0 >= n) return;
    uint32_t *wh = cs_begin(lds);
    const gcbyte_t fb = cs_frame(e);
    const uint32_t end = n - b0 < CS_BLOCK ? n : b0 + CS_BLOCK, mask = (1u << e.q[plane]) - 1u;
    for (uint32_t i = b0 + threadIdx.x; i < end; i += CS_T)
        cs_count(wh, gen_code(e, fb, plane, i), i ? gen_code(e, fb, plane, i - 1u) : 0u, mask);
    cs_flush(e, lds, plane);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
using CsFn = void (*)(CsArgs);

static int cs_check_format(int32_t src_format)
{
    if (src_format != CSIC_FMT_PLANAR && src_format != CSIC_FMT_PLANAR_BITS)
        return set_error(CSIC_EINVAL_FORMAT, "csic_code_stats reads PLANAR(2) or PLANAR_BITS(3). Got %d", src_format);
    return CSIC_OK;
}

static void fill_cs_args(const csic_plan *pl, int src_format, CsArgs *e)
{
    std::memset(e, 0, sizeof *e);
    csic_planar_bits_layout B;
    planar_bits_layout(pl->g, &pl->p, &B);
    const csic_planar_layout &G = B.geometry;
    e->n[0] = (uint32_t)((int64_t)G.y_width * G.y_height);
    e->n[1] = e->n[2] = (uint32_t)G.chroma_samples;
    e->q[0] = B.y_bits; e->q[1] = B.cb_bits; e->q[2] = B.cr_bits;
    if (src_format == CSIC_FMT_PLANAR_BITS) {
        e->off[0] = B.y_offset; e->off[1] = B.cb_offset; e->off[2] = B.cr_offset;
        e->ndw[0] = (uint32_t)((B.y_bytes + 3) / 4); e->ndw[1] = (uint32_t)((B.cb_bytes + 3) / 4); e->ndw[2] = (uint32_t)((B.cr_bytes + 3) / 4);
        e->frame_bytes = B.frame_bytes;
        e->bits_form = 1;
    } else {
        e->off[0] = G.y_offset; e->off[1] = G.cb_offset; e->off[2] = G.cr_offset;
        e->frame_bytes = G.frame_bytes;
    }
}

static CsFn cs_kernel(CodeStatsKind kind, int q, bool nt)
{
    if (kind == CSTAT_GEN) return k_cstat_gen;
    return with_const<true, false>(nt, [&](auto n) -> CsFn {
        constexpr bool NT = CSIC_CONST(n);
        if (kind == CSTAT_BYTES) return k_cstat_bytes<NT>;
        return with_const<1, 2, 3, 4, 5, 6, 7, 8>(q, [](auto qq) -> CsFn { return k_cstat_bits<CSIC_CONST(qq), NT>; });
    });
}

} // namespace csic

using namespace csic;

extern "C" {

const char *csic_code_stats_kernel_name(const csic_plan *plan, int32_t src_format)
{
    static thread_local char buf[96];
    if (!plan || (src_format != CSIC_FMT_PLANAR && src_format != CSIC_FMT_PLANAR_BITS)) return "";
    code_stats_kernel_name(code_stats_kind(src_format, plan->tune), src_format, plan->p, plan->tune, buf, sizeof buf);
    return buf;
}

int csic_code_stats_block_samples(const csic_plan *plan, int32_t src_format, int64_t *samples)
{
    if (!plan || !samples) return set_error(CSIC_EINVAL_NULL, "plan or samples is NULL");
    const int st = cs_check_format(src_format);
    if (st != CSIC_OK) return st;
    *samples = CSTAT_BLOCK_SAMPLES;
    clear_error();
    return CSIC_OK;
}

int csic_code_stats_device(csic_plan *plan, const void *d_src, int32_t src_format, int32_t nframes, uint64_t *d_hist, void *hip_stream)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    if (!d_src || !d_hist) return set_error(CSIC_EINVAL_NULL, "device buffer is NULL");
    int st = cs_check_format(src_format);
    if (st != CSIC_OK) return st;
    if (nframes < 1 || nframes > 65535) return set_error(CSIC_EINVAL_SIZE, "nframes must be 1..65535. Got %d", nframes);
    if ((uintptr_t)d_src & 255u) return set_error(CSIC_EINVAL_SIZE, "a planar frame buffer must be 256-byte aligned");
    if ((uintptr_t)d_hist & 7u) return set_error(CSIC_EINVAL_SIZE, "d_hist must be 8-byte aligned");
    const Geometry &g = plan->g;
    if ((int64_t)g.W * g.H >= ((int64_t)1 << 31)) return set_error(CSIC_EINVAL_SIZE, "frame too large for csic_code_stats_device");
    CsArgs e;
    fill_cs_args(plan, src_format, &e);
    e.src = static_cast<const uint8_t *>(d_src);
    e.hist = reinterpret_cast<unsigned long long *>(d_hist);
    const CodeStatsKind kind = code_stats_kind(src_format, plan->tune);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    CSIC_DEVICE_SCOPE(plan->device);
    HIP_TRY(hipMemsetAsync(d_hist, 0, (size_t)nframes * CS_HIST * sizeof(uint64_t), stream));
    // one launch over the three planes; k_cstat_bits is compiled per bit width, so there one launch per run of planes of equal width
    for (int p0 = 0; p0 < CSIC_STATS_PLANES;) {
        int p1 = p0 + 1;
        while (p1 < CSIC_STATS_PLANES && (kind != CSTAT_BITS || e.q[p1] == e.q[p0])) ++p1;
        uint32_t nmax = 0;
        for (int p = p0; p < p1; ++p) nmax = e.n[p] > nmax ? e.n[p] : nmax;
        if (nmax > 0) {
            e.plane0 = p0;
            const CsFn fn = cs_kernel(kind, e.q[p0], !plan->tune.no_nt);
            const unsigned blocks = (unsigned)(((uint64_t)nmax + CS_BLOCK - 1) / CS_BLOCK);
            st = launch(fn, dim3(blocks, (unsigned)(p1 - p0), (unsigned)nframes), dim3(CS_T, 1, 1), stream, e);
            if (st != CSIC_OK) return st;
        }
        p0 = p1;
    }
    clear_error();
    return CSIC_OK;
}

int csic_code_stats_host(csic_plan *plan, const void *src, size_t src_bytes, int32_t src_format, int32_t nframes, uint64_t *hist)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    if (!src || !hist) return set_error(CSIC_EINVAL_NULL, "host buffer is NULL");
    int st = cs_check_format(src_format);
    if (st != CSIC_OK) return st;
    if (nframes < 1 || nframes > 65535) return set_error(CSIC_EINVAL_SIZE, "nframes must be 1..65535. Got %d", nframes);
    CsArgs e;
    fill_cs_args(plan, src_format, &e);
    const size_t need = (size_t)nframes * (size_t)e.frame_bytes, hist_bytes = (size_t)nframes * CS_HIST * sizeof(uint64_t);
    if (src_bytes != need) return set_error(CSIC_EINVAL_SIZE, "expected %zu source bytes (%d frames), got %zu", need, nframes, src_bytes);
    CSIC_DEVICE_SCOPE(plan->device);
    DeviceStaging dev;
    void *d_src = dev.alloc(need), *d_hist = dev.alloc(hist_bytes);
    dev.to_device(d_src, src, need);
    if (dev.ok()) {
        st = csic_code_stats_device(plan, d_src, src_format, nframes, static_cast<uint64_t *>(d_hist), nullptr);
        if (st == CSIC_OK) { dev.to_host(hist, d_hist, hist_bytes); dev.sync(); }
    }
    if (st != CSIC_OK) return st;
    if (!dev.ok()) return set_error(CSIC_EHIP, "csic_code_stats_host: %s", hipGetErrorString(dev.error()));
    clear_error();
    return CSIC_OK;
}

} // extern "C"
