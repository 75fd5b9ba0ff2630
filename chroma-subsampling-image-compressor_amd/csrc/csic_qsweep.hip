// csic_qsweep.hip -- csic_qsweep_device: rate and distortion of all 512 (y_bits, cb_bits, cr_bits) of a plan from one pass over the
// input and one pass over its 8/8/8 planes (definition in include/csic.h).  The quantiser is three AND masks that commute with every
// other stage, and Y, Cb and Cr are independent, so 8 widths x 3 planes = 24 sums of squared errors and 24 residual histograms say
// what csic_distortion_* and csic_code_stats_* say about every bit set.
//
// Kernels (wave64, 256-thread blocks; integer byte work, no MFMA):
//   k_qsweep_sse_fast<ROUND, F, HH, VV, VEC, NT>   the plans measure_kind gives k_dist_fast: the same units (F input rows x 4 columns),
//                      the same loads (all issued before any arithmetic, the 4:x:0 odd row's one row-uniform load), the same clamped
//                      last block.
//   k_qsweep_sse_gen<ROUND, AVG>   everything else with an ARGB input: one output pixel per lane (measure_out_pixel), then its f x f
//                      input block, as k_dist_gen.
//   k_qsweep_sum       one block per frame: the frame's partials of 24 words, summed in a fixed order (sum_partials, csic_measure.h),
//                      -> the frame's sse[3][8].
//   k_qsweep_hist<NT>  csic_count.h's byte walk over the CSIC_FMT_PLANAR frame (the blocks, the LDS bins, the flush, the predecessor move
//                      and the ragged end are that header's, shared with csic_code_stats.hip) under QhCount: eight residual bins are
//                      bumped per sample, width q's residual being ((b >> (8 - q)) - (prev >> (8 - q))) mod 2^q of the 8-bit sample b
//                      and its predecessor.
//   k_qsweep_clear     zeroes the 6144 bins of every frame's hist (a kernel, not a memset of an interior pointer: DESIGN.md 4.13).
// Both SSE kernels run with the masks at 0xFF: the output value o they see is the unquantised one.  At width q the output is o - t_q
// with t_q = o & (0xFF >> q), constant over the n input pixels paired with o, and with e = ref - o their squared errors sum to
//     sum (e + t_q)^2 = sum e^2 + t_q (2 sum e + n t_q)
// an exact integer identity: a lane keeps two running sums per channel while it walks a block and touches its 24 accumulators once per
// output value (qs_block).
// Accumulation widths: every term qs_block adds IS the sum of squared errors of those n pixels at width q, each error in -255..255, so
// the bound in csic_distortion.hip's header holds as it stands: a lane sees at most 64 input pixels (16 in the fast kernel, f * f <= 64
// in the general one) and a wave at most 4096 (2^32 / 255^2 = 66 051), and 32 bits hold both.  The intermediate t_q (2 sum e + n t_q)
// may be negative (|.| <= 127 * (2 * 64 * 255 + 64 * 127) < 2^23); it is added modulo 2^32 to a total that is not.  The block sum, the
// partials and the frame's sums are 64-bit.  No atomics on this side: each block writes its own 192-byte partial with plain vector
// stores.
// Counting: 510 of csic_count.h's 512 LDS bins per wave (2^q bins of width q at offset 2^q - 2).  No loop of any kernel has a length
// that depends on buffer contents.  Every global access goes through the checked accessors of csic_kernel_ops.h or sits behind a
// CSIC_CHECK.
#include <cstdio>

#include "csic_count.h"
#include "csic_measure.h"

namespace csic {

constexpr int QS_T = MEAS_T, QS_WAVES = QS_T / 64;
constexpr int QS_W = CSIC_QSWEEP_WIDTHS, QS_CH = CSIC_STATS_PLANES * QS_W;           // 24 sums per frame
constexpr int QS_RES_WORDS = (int)(sizeof(csic_qsweep_result) / sizeof(uint64_t));   // 6168
constexpr int QS_HIST_WORDS = QS_CH * CSIC_STATS_BINS;                               // 6144
static_assert(QS_W == 8 && CSIC_STATS_BINS == 256 && QS_T == CNT_T, "the eight widths' 510 bins fit csic_count.h's 512");
static_assert(QS_RES_WORDS == QS_CH + QS_HIST_WORDS && offsetof(csic_qsweep_result, hist) == QS_CH * sizeof(uint64_t), "sse, then hist");

struct QExtra {
    uint64_t *part;                  // workspace: nblk partials of QS_CH uint64 per frame, frames back to back
    uint32_t nblk;                   // blocks (= partials) per frame
    uint32_t nunits;                 // k_qsweep_sse_fast: units per frame; k_qsweep_sse_gen: output pixels per frame
};

typedef uint64_t CSIC_GLOBAL *gqpart_t;

// ------------------------------------------------------------------------------------------------
// the 24 sums
// ------------------------------------------------------------------------------------------------
// One unquantised output value o and the n reference values paired with it, e = ref - o: se2 = sum e^2, se = sum e.  Adds the sum of
// squared errors at every width (the identity and the widths: header).
__device__ __forceinline__ void qs_block(uint32_t (&s)[QS_W], uint32_t o, uint32_t se2, int se, int n)
{
#pragma unroll
    for (int q = 1; q <= QS_W; ++q) {
        const int t = (int)(o & (0xFFu >> q));
        s[q - 1] += se2 + (uint32_t)__mul24(t, 2 * se + __mul24(n, t));
    }
}

// one reference value against its output value
__device__ __forceinline__ void qs_px(uint32_t &se2, int &se, uint32_t ref, uint32_t o)
{
    const int e = (int)ref - (int)o;
    se2 += (uint32_t)__mul24(e, e);
    se += e;
}

// lane sums -> wave sums (32-bit, see the header) -> this block's 64-bit partial
__device__ __forceinline__ void qs_block_partial(const QExtra &e, uint32_t (&s)[CSIC_STATS_PLANES][QS_W])
{
    __shared__ uint64_t red[QS_WAVES][QS_CH];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int p = 0; p < CSIC_STATS_PLANES; ++p)
#pragma unroll
        for (int q = 0; q < QS_W; ++q) {
            uint32_t v = s[p][q];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
            if (lane == 0) red[wave][p * QS_W + q] = v;
        }
    __syncthreads();
    if (threadIdx.x < (unsigned)QS_CH) {
        uint64_t t = 0;
#pragma unroll
        for (int w = 0; w < QS_WAVES; ++w) t += red[w][threadIdx.x];
        CSIC_CHECK(blockIdx.x < e.nblk);
        ((gqpart_t)(uintptr_t)e.part)[((uint64_t)blockIdx.z * e.nblk + blockIdx.x) * QS_CH + threadIdx.x] = t;
    }
}

// ------------------------------------------------------------------------------------------------
// k_qsweep_sse_fast
// ------------------------------------------------------------------------------------------------
template <int ROUND, int F, int HH, int VV, bool VEC, bool NT, bool CHECK>
__device__ __forceinline__ void qs_fast_body(const KArgs &a, gin_t in, uint32_t u0, uint32_t nunits, uint32_t (&s)[CSIC_STATS_PLANES][QS_W])
{
    constexpr int K = 4 / F;
    const uint32_t W = (uint32_t)a.W;
    uint32_t off[K], cpx[K];
    bool odd[K];
    u32x4 p[K][F];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        // the frame's last block: clamp instead of branching, so that every load still issues ahead of the arithmetic
        const uint32_t u = CHECK ? min(u0 + (uint32_t)(k * QS_T), nunits - 1u) : u0 + (uint32_t)(k * QS_T);
        const uint32_t j0 = 4u * u;                                         // < 2^30 (measure_kind)
        const uint32_t ur = (uint32_t)(((uint64_t)j0 * a.mW) >> a.kW);      // unit row = j0 / W, exact
        off[k] = F == 1 ? j0 : j0 + __umul24(ur, W);                        // rows F * ur .. : (F * ur) * W + (j0 - ur * W)
        odd[k] = F == 1 && VV == 2 && (ur & 1u);
        cpx[k] = 0;
        if constexpr (F == 1 && VV == 2) {
            // 4:x:0 odd row: every pixel holds the chroma latched at the last sample of the row above
            if (__builtin_amdgcn_ballot_w64(odd[k]) != 0)
                cpx[k] = in1n<false>(a, in, odd[k] ? __umul24(ur - 1u, W) + (uint32_t)a.last_sample_col : off[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int i = 0; i < F; ++i) p[k][i] = in4n_or_1n<VEC, NT>(a, in, off[k] + (uint32_t)i * W);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (CHECK && u0 + (uint32_t)(k * QS_T) >= nunits) continue;
        const uint32_t q0[4] = {p[k][0].x, p[k][0].y, p[k][0].z, p[k][0].w};
        uint32_t ry[4], rcb[4], rcr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { ry[i] = fwd_y(q0[i]); fwd_c<ROUND>(q0[i], rcb[i], rcr[i]); }
        if constexpr (F == 1) {
            uint32_t ocb = 0, ocr = 0;
            if (VV == 2) fwd_c<ROUND>(cpx[k], ocb, ocr);
#pragma unroll
            for (int g = 0; g < 4; g += HH) {
                const uint32_t cb = (VV == 2 && odd[k]) ? ocb : rcb[g];          // held chroma, unquantised
                const uint32_t cr = (VV == 2 && odd[k]) ? ocr : rcr[g];
                uint32_t b2 = 0, c2 = 0;
                int b1 = 0, c1 = 0;
#pragma unroll
                for (int i = g; i < g + HH; ++i) {
                    qs_block(s[0], ry[i], 0u, 0, 1);                             // the pixel's own Y: e = 0
                    qs_px(b2, b1, rcb[i], cb);
                    qs_px(c2, c1, rcr[i], cr);
                }
                qs_block(s[1], cb, b2, b1, HH);
                qs_block(s[2], cr, c2, c1, HH);
            }
        } else {
            const uint32_t q1[4] = {p[k][1].x, p[k][1].y, p[k][1].z, p[k][1].w};
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                // output (ro, co) = (ur, 2 ug + o): Y of input column 2 co = unit column 2 o; chroma held from column 2 co & ~(h - 1)
                const int src = HH == 4 ? 0 : 2 * o;
                const uint32_t y = ry[2 * o], cb = rcb[src], cr = rcr[src];
                uint32_t y2 = 0, b2 = 0, c2 = 0;
                int y1 = 0, b1 = 0, c1 = 0;
#pragma unroll
                for (int i = 2 * o; i < 2 * o + 2; ++i) {
                    qs_px(y2, y1, ry[i], y);
                    qs_px(b2, b1, rcb[i], cb);
                    qs_px(c2, c1, rcr[i], cr);
                    uint32_t rb, rc;
                    fwd_c<ROUND>(q1[i], rb, rc);
                    qs_px(y2, y1, fwd_y(q1[i]), y);
                    qs_px(b2, b1, rb, cb);
                    qs_px(c2, c1, rc, cr);
                }
                qs_block(s[0], y, y2, y1, 4);
                qs_block(s[1], cb, b2, b1, 4);
                qs_block(s[2], cr, c2, c1, 4);
            }
        }
    }
}

template <int ROUND, int F, int HH, int VV, bool VEC, bool NT>
__global__ void __launch_bounds__(QS_T) k_qsweep_sse_fast(KArgs a, QExtra e)
{
    pin_args(a);
    const gin_t in = frame_in(a);
    constexpr uint32_t per_block = QS_T * (4 / F);
    const uint32_t b0 = blockIdx.x * per_block;
    uint32_t s[CSIC_STATS_PLANES][QS_W] = {};
    if (b0 + per_block <= e.nunits) qs_fast_body<ROUND, F, HH, VV, VEC, NT, false>(a, in, b0 + threadIdx.x, e.nunits, s);
    else                            qs_fast_body<ROUND, F, HH, VV, VEC, NT, true>(a, in, b0 + threadIdx.x, e.nunits, s);
    qs_block_partial(e, s);
}

// ------------------------------------------------------------------------------------------------
// k_qsweep_sse_gen
// ------------------------------------------------------------------------------------------------
template <int ROUND, bool AVG>
__global__ void __launch_bounds__(QS_T) k_qsweep_sse_gen(KArgs a, QExtra e)
{
    pin_args(a);
    const gin_t in = frame_in(a);
    const uint32_t j = blockIdx.x * (uint32_t)QS_T + threadIdx.x;
    uint32_t s[CSIC_STATS_PLANES][QS_W] = {};
    if (j < e.nunits) {
        const int ro = (int)(((uint64_t)j * a.mWo) >> a.kWo), co = (int)j - ro * a.Wo;      // j / Wo, exact for j < 2^31
        const Ycc o = measure_out_pixel<ROUND, AVG, F_ARGB>(a, in, ro, co);                 // masks 0xFF: the unquantised output pixel
        const int r0 = ro * a.f, c0 = co * a.f, r1 = min(r0 + a.f, a.H), c1 = min(c0 + a.f, a.W);
        uint32_t y2 = 0, b2 = 0, c2 = 0;
        int y1 = 0, b1 = 0, cc1 = 0;
        for (int r = r0; r < r1; ++r) {
            for (int c = c0; c < c1; ++c) {
                uint32_t ref[MEAS_CH];
                ref_channels<ROUND, F_ARGB>(in1<false>(a, in, (int64_t)r * a.ip + c), ref);
                qs_px(y2, y1, ref[3], o.y);
                qs_px(b2, b1, ref[4], o.cb);
                qs_px(c2, cc1, ref[5], o.cr);
            }
        }
        const int n = (r1 - r0) * (c1 - c0);                                                // <= 64
        qs_block(s[0], o.y, y2, y1, n);
        qs_block(s[1], o.cb, b2, b1, n);
        qs_block(s[2], o.cr, c2, cc1, n);
    }
    qs_block_partial(e, s);
}

// frame blockIdx.x's partials -> its sse[3][8]
static __global__ void __launch_bounds__(QS_T) k_qsweep_sum(const uint64_t *part, uint32_t nblk, uint64_t *result)
{
    sum_partials<QS_CH, QS_RES_WORDS>(part, nblk, result);
}

// ------------------------------------------------------------------------------------------------
// k_qsweep_hist
// ------------------------------------------------------------------------------------------------
// csic_count.h's policy: the code of a byte is the byte; a sample bumps eight residual bins, width q's at 2^q - 2 (510 bins, the
// last two of the 512 unused); LDS bin k is word hist[plane][q - 1][r] of the frame's csic_qsweep_result
struct QhCount {
    __device__ __forceinline__ uint32_t code(uint32_t byte) const { return byte; }
    // 8-bit value b after 8-bit value prev (0 in front of sample 0)
    __device__ __forceinline__ void bump(uint32_t *wh, uint32_t b, uint32_t prev) const
    {
#pragma unroll
        for (int q = 1; q <= QS_W; ++q) {
            const uint32_t r = ((b >> (8 - q)) - (prev >> (8 - q))) & ((1u << q) - 1u);
            __hip_atomic_fetch_add(&wh[(1u << q) - 2u + r], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    static constexpr uint32_t STRIDE = QS_RES_WORDS;
    static __device__ __forceinline__ bool has_word(uint32_t k) { return k < 510u; }
    static __device__ __forceinline__ uint32_t index(int plane, uint32_t k0, uint32_t t)
    {
        const uint32_t k = k0 + t;
        const uint32_t q = 31u - (uint32_t)__builtin_clz(k + 2u), r = k + 2u - (1u << q);
        CSIC_CHECK(q >= 1u && q <= 8u && r < (1u << q) && plane < CSIC_STATS_PLANES);
        return (uint32_t)QS_CH + ((uint32_t)plane * QS_W + (q - 1u)) * CSIC_STATS_BINS + r;
    }
};

template <bool NT>
__global__ void __launch_bounds__(QS_T) k_qsweep_hist(CountArgs e)
{
    const int plane = (int)blockIdx.y;
    count_block<QhCount>(e, plane, [&](auto check, gcbyte_t fb, uint32_t *wh, uint32_t i0) {
        count_bytes_body<NT, CSIC_CONST(check)>(e, fb, wh, plane, i0, QhCount{});
    });
}

// grid (24, 1, nframes): one 256-bin histogram per block
static __global__ void __launch_bounds__(QS_T) k_qsweep_clear(unsigned long long *res)
{
    const uint32_t at = (uint32_t)QS_CH + blockIdx.x * (uint32_t)CSIC_STATS_BINS + threadIdx.x;
    CSIC_CHECK(at < (uint32_t)QS_RES_WORDS);
    ((gcount_t)(uintptr_t)res)[(uint64_t)blockIdx.z * QS_RES_WORDS + at] = 0ull;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
using QsFn = MeasureFn<QExtra>;

// The plan whose planar output carries every width: the caller's with all three widths 8 and out_format PLANAR.  Its geometry has
// the masks at 0xFF; its staging pointers are not the copy's to free.
static int qs_plan888(const csic_plan *pl, csic_plan *q)
{
    *q = *pl;
    q->p.y_bits = q->p.cb_bits = q->p.cr_bits = 8;
    q->p.out_format = CSIC_FMT_PLANAR;
    q->d_in = q->d_out = nullptr;
    q->d_sum = nullptr;
    return derive_geometry(&q->p, &q->g);
}

static int qs_check_format(const csic_plan *pl)
{
    if (pl->p.in_format != CSIC_FMT_ARGB8888)
        return set_error(CSIC_EINVAL_FORMAT, "csic_qsweep reads ARGB8888(0) input. Got %d", pl->p.in_format);
    return CSIC_OK;
}

static const char *const QS_FRAMES_FMT = "nframes must be in 1..65535. Got %d";
static int qs_check_frames(int32_t nframes) { return count_check_frames(nframes, QS_FRAMES_FMT); }

// k_qsweep_sse_fast: units per frame; k_qsweep_sse_gen: output pixels per frame (as DistUnit)
static uint32_t qs_units(const Geometry &g, int kind)
{
    if (kind == 0) return (uint32_t)((int64_t)g.Wo * g.Ho);
    return (uint32_t)((int64_t)(g.W / 4) * (g.H / kind));
}
static uint32_t qs_blocks(const Geometry &g, int kind)
{
    const int64_t per_block = kind == 0 ? QS_T : (int64_t)QS_T * (4 / kind);
    return (uint32_t)((qs_units(g, kind) + per_block - 1) / per_block);
}
static int qs_kind(const csic_plan *pl) { return measure_kind(pl->p, pl->g, pl->tune, MEASURE_DIST); }

static QsFn qs_kernel(const csic_plan *pl, int kind, bool vec)
{
    return measure_kernel<QsFn>(
        pl, kind, vec, [](auto round, auto avg, auto) { return k_qsweep_sse_gen<CSIC_CONST(round), CSIC_CONST(avg)>; },
        [](auto round, auto f, auto h, auto v, auto v16, auto nt) {
            return k_qsweep_sse_fast<CSIC_CONST(round), CSIC_CONST(f), CSIC_CONST(h), CSIC_CONST(v), CSIC_CONST(v16), CSIC_CONST(nt)>;
        });
}

// bytes of the partials (a multiple of 256, so that the planar frames behind them are aligned) and of the planar frames
static int qs_workspace(const csic_plan *pl, int32_t nframes, size_t *part_bytes, size_t *bytes)
{
    int st = qs_check_frames(nframes);
    if (st == CSIC_OK) st = qs_check_format(pl);
    if (st != CSIC_OK) return st;
    csic_plan q;
    st = qs_plan888(pl, &q);
    if (st != CSIC_OK) return st;
    csic_planar_layout L;
    planar_layout(q.g, &q.p, &L);
    const size_t part = (size_t)nframes * qs_blocks(q.g, qs_kind(&q)) * QS_CH * sizeof(uint64_t);
    *part_bytes = (part + 255u) & ~(size_t)255u;
    *bytes = *part_bytes + (size_t)nframes * (size_t)L.frame_bytes;
    return CSIC_OK;
}

// the clear and k_qsweep_hist over nframes planar frames (arguments checked by the callers)
static int qs_hist_launch(const csic_plan *pl, const void *d_planar, int32_t nframes, csic_qsweep_result *d_result, hipStream_t stream)
{
    CountArgs e;
    count_fill_planar(pl, &e);
    e.src = static_cast<const uint8_t *>(d_planar);
    e.res = reinterpret_cast<unsigned long long *>(d_result);
    int st = launch(k_qsweep_clear, dim3(QS_CH, 1, (unsigned)nframes), dim3(QS_T, 1, 1), stream, e.res);
    if (st != CSIC_OK) return st;
    const uint32_t nmax = e.n[0] > e.n[1] ? e.n[0] : e.n[1];
    if (nmax == 0) return CSIC_OK;
    const unsigned blocks = (unsigned)(((uint64_t)nmax + CNT_BLOCK - 1) / CNT_BLOCK);
    const auto fn = pl->tune.no_nt ? k_qsweep_hist<false> : k_qsweep_hist<true>;
    return launch(fn, dim3(blocks, CSIC_STATS_PLANES, (unsigned)nframes), dim3(QS_T, 1, 1), stream, e);
}

} // namespace csic

using namespace csic;

extern "C" {

int csic_qsweep_workspace_bytes(const csic_plan *plan, int32_t nframes, size_t *bytes)
{
    if (!plan || !bytes) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    size_t part = 0;
    const int st = qs_workspace(plan, nframes, &part, bytes);
    if (st == CSIC_OK) clear_error();
    return st;
}

const char *csic_qsweep_kernel_name(const csic_plan *plan)
{
    if (!plan) return "";
    static const char *const names[4] = {"k_qsweep_sse_gen<hold>", "k_qsweep_sse_gen<avg>", "k_qsweep_sse_fast<f1>", "k_qsweep_sse_fast<f2>"};
    const int kind = qs_kind(plan);
    return names[kind == 0 ? (plan->p.sampling == CSIC_SAMPLING_AVG ? 1 : 0) : 1 + kind];
}

int csic_qsweep_block_samples(const csic_plan *plan, int64_t *samples)
{
    if (!plan || !samples) return set_error(CSIC_EINVAL_NULL, "plan or samples is NULL");
    *samples = CNT_BLOCK;
    clear_error();
    return CSIC_OK;
}

int csic_qsweep_hist_device(csic_plan *plan, const void *d_planar, int32_t nframes, csic_qsweep_result *d_result, void *hip_stream)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    if (!d_planar || !d_result) return set_error(CSIC_EINVAL_NULL, "device buffer is NULL");
    int st = count_check_buffers(nframes, QS_FRAMES_FMT, d_planar, d_result, "d_result must be 8-byte aligned");
    if (st == CSIC_OK) st = qs_check_format(plan);
    if (st != CSIC_OK) return st;
    st = csic_device_count();
    if (st < 0) return st;
    st = count_check_size(plan->g, "frame too large for csic_qsweep_hist_device");
    if (st != CSIC_OK) return st;
    CSIC_DEVICE_SCOPE(plan->device);
    st = qs_hist_launch(plan, d_planar, nframes, d_result, static_cast<hipStream_t>(hip_stream));
    if (st != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

int csic_qsweep_device(csic_plan *plan, const void *d_in, int32_t nframes, csic_qsweep_result *d_result, void *d_workspace,
                       size_t workspace_bytes, void *hip_stream)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    if (!d_in || !d_result || !d_workspace) return set_error(CSIC_EINVAL_NULL, "device buffer is NULL");
    int st = qs_check_frames(nframes);
    if (st != CSIC_OK) return st;
    if ((uintptr_t)d_in & 3u) return set_error(CSIC_EINVAL_SIZE, "the input must be 4-byte aligned");
    if ((uintptr_t)d_result & 7u) return set_error(CSIC_EINVAL_SIZE, "d_result must be 8-byte aligned");
    if ((uintptr_t)d_workspace & 255u) return set_error(CSIC_EINVAL_SIZE, "the workspace must be 256-byte aligned");
    st = qs_check_format(plan);
    if (st != CSIC_OK) return st;
    st = csic_device_count();
    if (st < 0) return st;
    size_t part_bytes = 0, need = 0;
    st = qs_workspace(plan, nframes, &part_bytes, &need);
    if (st != CSIC_OK) return st;
    if (workspace_bytes < need)
        return set_error(CSIC_EINVAL_SIZE, "workspace of %zu bytes is smaller than the %zu bytes csic_qsweep_workspace_bytes asks for",
                         workspace_bytes, need);
    csic_plan q;
    st = qs_plan888(plan, &q);
    if (st != CSIC_OK) return st;
    const Geometry &g = q.g;
    if ((int64_t)g.W * g.H >= ((int64_t)1 << 31)) return set_error(CSIC_EINVAL_SIZE, "frame too large for csic_qsweep_device");
    const int kind = qs_kind(&q);
    // 16-byte loads only for a 16-byte aligned d_in (the frame stride W * H * 4 is a multiple of 16 whenever width % 4 == 0)
    const bool vec = ((uintptr_t)d_in & 15u) == 0 && !q.tune.no_vec;
    const QsFn fn = qs_kernel(&q, kind, vec);
    CSIC_DEVICE_SCOPE(plan->device);
    KArgs a;
    fill_base_args(g, g.W, g.Wo, &a);                       // my = mcb = mcr = 0xFF
    a.in = static_cast<const uint32_t *>(d_in);
    a.bdx = QS_T; a.bdy = 1; a.row_step = 1;
    QExtra e{};
    e.part = static_cast<uint64_t *>(d_workspace);
    e.nblk = qs_blocks(g, kind);
    e.nunits = qs_units(g, kind);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    uint8_t *d_planar = static_cast<uint8_t *>(d_workspace) + part_bytes;
    st = launch(fn, dim3(e.nblk, 1, (unsigned)nframes), dim3(QS_T, 1, 1), stream, a, e);
    if (st == CSIC_OK)
        st = launch(k_qsweep_sum, dim3((unsigned)nframes, 1, 1), dim3(QS_T, 1, 1), stream, static_cast<const uint64_t *>(d_workspace), e.nblk,
                    reinterpret_cast<uint64_t *>(d_result));
    if (st == CSIC_OK) st = planar_forward(&q, d_in, d_planar, nframes, stream);
    if (st == CSIC_OK) st = qs_hist_launch(&q, d_planar, nframes, d_result, stream);
    if (st != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

int csic_qsweep_host(csic_plan *plan, const uint32_t *in, size_t in_px, int32_t nframes, csic_qsweep_result *result)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    if (!in || !result) return set_error(CSIC_EINVAL_NULL, "host buffer is NULL");
    int st = qs_check_frames(nframes);
    if (st == CSIC_OK) st = qs_check_format(plan);
    if (st != CSIC_OK) return st;
    st = csic_device_count();
    if (st < 0) return st;
    size_t part = 0, ws = 0;
    st = qs_workspace(plan, nframes, &part, &ws);
    if (st != CSIC_OK) return st;
    const Geometry &g = plan->g;
    const size_t need = (size_t)nframes * (size_t)g.W * (size_t)g.H;
    if (in_px != need) return set_error(CSIC_EINVAL_SIZE, "expected %zu input pixels (%d frames), got %zu", need, nframes, in_px);
    CSIC_DEVICE_SCOPE(plan->device);
    const size_t res_bytes = (size_t)nframes * sizeof(csic_qsweep_result);
    DeviceStaging dev;
    void *d_in = dev.alloc(need * 4), *d_ws = dev.alloc(ws), *d_res = dev.alloc(res_bytes);
    dev.to_device(d_in, in, need * 4);
    if (dev.ok()) {
        st = csic_qsweep_device(plan, d_in, nframes, static_cast<csic_qsweep_result *>(d_res), d_ws, ws, nullptr);
        if (st == CSIC_OK) { dev.to_host(result, d_res, res_bytes); dev.sync(); }
    }
    if (st != CSIC_OK) return st;
    if (!dev.ok()) return set_error(CSIC_EHIP, "csic_qsweep_host: %s", hipGetErrorString(dev.error()));
    clear_error();
    return CSIC_OK;
}

} // extern "C"
