// csic_code_stats.hip -- csic_code_stats_*: exact histograms of the sample codes of a compressed frame (CSIC_FMT_PLANAR or
// CSIC_FMT_PLANAR_BITS) and of their left-predicted residuals, per plane, in one pass over the compressed frame itself.  The
// definition -- codes, the predictor, storage order, the result's layout -- is in include/csic.h; the entropies and the sizes an
// entropy coder could reach are host arithmetic on these counts (compressor.py, csic.hpp).
//
// The blocks, the LDS bins, the flush, the predecessor move, the ragged end and the byte walk are csic_count.h's (shared with
// csic_qsweep.hip); plane = plane0 + blockIdx.y.  This unit's own:
//   CsCount            what is counted: the code of a PLANAR byte is byte >> (8 - q); a sample bumps two bins, its code's (kind 0,
//                      LDS bins 0..255) and its residual's (kind 1, bins 256..511); LDS bin k is word [k >> 8][plane][k & 255] of the
//                      frame's 1536.
//   k_cstat_bytes<NT>     CSIC_FMT_PLANAR: the byte walk under CsCount.
//   k_cstat_bits<Q, NT>   CSIC_FMT_PLANAR_BITS, one instantiation per bit width: a lane takes GROUPS of 32 samples = exactly Q dwords
//                      (no sample straddles a lane), 4 groups in flight, 2 rounds; the codes are cut out of the dwords with
//                      compile-time shifts.  Planes of different widths go out as separate launches (Y, then Cb and Cr).  In front
//                      of a wave's span it loads the dword before its first group; a plane's last block reads dword by dword up to
//                      the last dword that holds a sample.
//   k_cstat_gen        either format, run-time q: one sample per lane and step, 256 steps, the predecessor loaded by the lane
//                      itself, straight from the definition.  CSIC_TUNE_FORCE_GENERIC, CSIC_TUNE_VARIANT 9 (and CSIC_TUNE_NO_VECTOR
//                      for PLANAR): the on-device cross-check of the two fast kernels.
// d_hist is cleared by the entry point with a memset on the same stream.
#include <cstdio>

#include "csic_count.h"

namespace csic {

constexpr int CS_BINS = CSIC_STATS_BINS, CS_HIST = CSIC_STATS_KINDS * CSIC_STATS_PLANES * CSIC_STATS_BINS;
static_assert(CSIC_STATS_KINDS == 2 && CSIC_STATS_BINS == 256 && CNT_T == 256, "one thread per bin flushes both kinds");

// the kernels' argument
struct CsArgs : CountArgs {        // res: [frame][kind][plane][bin]
    uint32_t ndw[3];               // PLANAR_BITS: dwords that hold a plane's samples
    int32_t q[3];                  // bits per code
    int32_t plane0;                // plane of blockIdx.y = 0
    int32_t bits_form;             // k_cstat_gen: 1 = PLANAR_BITS, 0 = PLANAR
};

// one sample: code c after code prev (0 in front of sample 0)
__device__ __forceinline__ void cs_count(uint32_t *wh, uint32_t c, uint32_t prev, uint32_t mask)
{
    __hip_atomic_fetch_add(&wh[c], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(&wh[CS_BINS + ((c - prev) & mask)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// csic_count.h's policy (the byte walk of a plane of q bits; k_cstat_bits and k_cstat_gen take its flush)
struct CsCount {
    uint32_t sh, mask;
    __device__ __forceinline__ explicit CsCount(int q) : sh(8u - (uint32_t)q), mask((1u << q) - 1u) {}
    __device__ __forceinline__ uint32_t code(uint32_t byte) const { return byte >> sh; }
    __device__ __forceinline__ void bump(uint32_t *wh, uint32_t c, uint32_t prev) const { cs_count(wh, c, prev, mask); }
    static constexpr uint32_t STRIDE = CS_HIST;
    static __device__ __forceinline__ bool has_word(uint32_t) { return true; }
    static __device__ __forceinline__ uint32_t index(int plane, uint32_t k0, uint32_t t)          // kind = k0 / 256, bin t
    {
        return (uint32_t)((int)(k0 / CS_BINS) * CSIC_STATS_PLANES + plane) * CS_BINS + t;
    }
};

// ------------------------------------------------------------------------------------------------
// k_cstat_bytes
// ------------------------------------------------------------------------------------------------
template <bool NT>
__global__ void __launch_bounds__(CNT_T) k_cstat_bytes(CsArgs e)
{
    const int plane = e.plane0 + (int)blockIdx.y;
    count_block<CsCount>(e, plane, [&](auto check, gcbyte_t fb, uint32_t *wh, uint32_t i0) {
        count_bytes_body<NT, CSIC_CONST(check)>(e, fb, wh, plane, i0, CsCount(e.q[plane]));
    });
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
    if (i0 > 0 && (!CHECK || i0 < n)) carry = count_ld4<NT>(e, fb, off + 4 * ((int64_t)(i0 / 32u) * Q - 1)) >> (32 - Q);
    for (uint32_t g0 = i0 / 32u; g0 < (i0 + CNT_WAVE) / 32u; g0 += 64u * CNT_K) {
        if (CHECK && 32u * g0 >= n) break;                                  // wave-uniform
        uint32_t d[CNT_K][Q];
#pragma unroll
        for (int k = 0; k < CNT_K; ++k) {
            const uint32_t dw0 = (g0 + 64u * (uint32_t)k + lane) * (uint32_t)Q;     // < 2^26 * 8
#pragma unroll
            for (int i = 0; i < Q; ++i)
                d[k][i] = (!CHECK || dw0 + (uint32_t)i < ndw) ? count_ld4<NT>(e, fb, off + 4 * (int64_t)(dw0 + (uint32_t)i)) : 0u;
        }
#pragma unroll
        for (int k = 0; k < CNT_K; ++k) {
            const uint32_t first = 32u * (g0 + 64u * (uint32_t)k + lane);
            uint32_t prev = count_pred(d[k][Q - 1] >> (32 - Q), carry);
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
__global__ void __launch_bounds__(CNT_T) k_cstat_bits(CsArgs e)
{
    const int plane = e.plane0 + (int)blockIdx.y;
    count_block<CsCount>(e, plane, [&](auto check, gcbyte_t fb, uint32_t *wh, uint32_t i0) {
        bits_body<Q, NT, CSIC_CONST(check)>(e, fb, wh, plane, i0);
    });
}

// ------------------------------------------------------------------------------------------------
// k_cstat_gen: the definition, one sample per lane and step
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t gen_code(const CsArgs &e, gcbyte_t fb, int plane, uint32_t i)
{
    const uint32_t q = (uint32_t)e.q[plane];
    if (!e.bits_form) return count_ld1(e, fb, e.off[plane] + i) >> (8u - q);
    const uint64_t bit = (uint64_t)i * q;
    const int64_t at = e.off[plane] + 4 * (int64_t)(bit >> 5);
    const uint32_t s = (uint32_t)bit & 31u;
    const uint32_t lo = count_ld4<false>(e, fb, at), hi = s + q > 32u ? count_ld4<false>(e, fb, at + 4) : 0u;
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> s) & ((1u << q) - 1u);
}

__global__ void __launch_bounds__(CNT_T) k_cstat_gen(CsArgs e)
{
    __shared__ CountLds lds;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t b0 = blockIdx.x * CNT_BLOCK, n = e.n[plane];
    if (b0 >= n) return;
    uint32_t *wh = count_begin(lds);
    const gcbyte_t fb = count_frame(e);
    const uint32_t end = n - b0 < CNT_BLOCK ? n : b0 + CNT_BLOCK, mask = (1u << e.q[plane]) - 1u;
    for (uint32_t i = b0 + threadIdx.x; i < end; i += CNT_T)
        cs_count(wh, gen_code(e, fb, plane, i), i ? gen_code(e, fb, plane, i - 1u) : 0u, mask);
    count_flush<CsCount>(e, lds, plane);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
using CsFn = void (*)(CsArgs);

static const char *const CS_FRAMES_FMT = "nframes must be 1..65535. Got %d";

static int cs_check_format(int32_t src_format)
{
    if (src_format != CSIC_FMT_PLANAR && src_format != CSIC_FMT_PLANAR_BITS)
        return set_error(CSIC_EINVAL_FORMAT, "csic_code_stats reads PLANAR(2) or PLANAR_BITS(3). Got %d", src_format);
    return CSIC_OK;
}

static void fill_cs_args(const csic_plan *pl, int src_format, CsArgs *e)
{
    *e = CsArgs{};
    count_fill_planar(pl, e);
    e->q[0] = pl->p.y_bits; e->q[1] = pl->p.cb_bits; e->q[2] = pl->p.cr_bits;
    if (src_format == CSIC_FMT_PLANAR_BITS) {              // the same samples, each plane at its own width
        csic_planar_bits_layout B;
        planar_bits_layout(pl->g, &pl->p, &B);
        e->off[0] = B.y_offset; e->off[1] = B.cb_offset; e->off[2] = B.cr_offset;
        e->ndw[0] = (uint32_t)((B.y_bytes + 3) / 4); e->ndw[1] = (uint32_t)((B.cb_bytes + 3) / 4); e->ndw[2] = (uint32_t)((B.cr_bytes + 3) / 4);
        e->frame_bytes = B.frame_bytes;
        e->bits_form = 1;
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
    st = count_check_buffers(nframes, CS_FRAMES_FMT, d_src, d_hist, "d_hist must be 8-byte aligned");
    if (st == CSIC_OK) st = count_check_size(plan->g, "frame too large for csic_code_stats_device");
    if (st != CSIC_OK) return st;
    CsArgs e;
    fill_cs_args(plan, src_format, &e);
    e.src = static_cast<const uint8_t *>(d_src);
    e.res = reinterpret_cast<unsigned long long *>(d_hist);
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
            const unsigned blocks = (unsigned)(((uint64_t)nmax + CNT_BLOCK - 1) / CNT_BLOCK);
            st = launch(fn, dim3(blocks, (unsigned)(p1 - p0), (unsigned)nframes), dim3(CNT_T, 1, 1), stream, e);
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
    st = count_check_frames(nframes, CS_FRAMES_FMT);
    if (st != CSIC_OK) return st;
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
