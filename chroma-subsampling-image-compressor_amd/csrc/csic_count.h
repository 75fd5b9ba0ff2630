// csic_count.h -- what the counting units (csic_code_stats.hip, csic_qsweep.hip's k_qsweep_hist) share: the walk over the byte
// planes of a CSIC_FMT_PLANAR frame that counts in LDS, and everything around it.  Both units give a block CNT_BLOCK = 65 536
// consecutive samples of one plane (plane from blockIdx.y, frame = blockIdx.z), a wave a contiguous quarter of them, and count into
// one private set of 512 32-bit LDS bins per wave, 8 KiB per block, bumped with LDS atomics (a block's 65 536 samples cannot overflow
// a bin); after one barrier thread t adds the four waves' bins t and t + 256 and, where a sum is not zero, issues one 64-bit global
// atomic add into the frame's result.  Integer adds commute: the result is exact whatever the schedule.
// The byte walk: a lane takes CHUNKS of 16 consecutive samples, one 16-byte load each (plane offsets are multiples of 256, so every
// chunk is aligned); CNT_K = 4 chunks per lane are in flight, lane l of a wave taking chunk c0 + 64 k + l of step k, so that a
// wave-instruction reads 1 KiB and a wave walks its 16 KiB in 4 rounds of 4.  The predecessor of a lane's first sample is the last
// code of the lane to its left (one ds_bpermute move); lane 0 takes the last code lane 63 held in the step before, and only at a wave's
// first step does it load the byte in front of the wave's span -- nothing at sample 0.
// THE RAGGED END, stated here and nowhere else: a plane's last block runs the same body with every chunk tested against the plane's
// sample count -- whole ones are loaded as above, the one the plane ends in is read byte by byte, the ones beyond it are not loaded
// at all, and nothing behind the last sample is counted.
// A unit says what it counts with a policy P (everything in it a compile-time constant or wave-uniform):
//   uint32_t code(uint32_t byte) const;                          the code of a sample byte
//   void bump(uint32_t *wh, uint32_t c, uint32_t prev) const;    one sample: code c after code prev (0 in front of sample 0)
//   static constexpr uint32_t STRIDE;                            64-bit words of one frame's result
//   static bool has_word(uint32_t k);                            LDS bin k (0..511) has a word in the result
//   static uint32_t index(int plane, uint32_t k0, uint32_t t);   which one, for bin k = k0 + t of thread t (k0 = 0 or 256, a constant
//                                                                once the flush is unrolled; with the CSIC_CHECK of the unit's own bound)
// Host side: the argument base's filler for a PLANAR frame, and the refusals the two device entry points share.  Every global load
// goes through the accessors of csic_kernel_ops.h, which the CSIC_DEBUG build checks against the frame's bytes.
#pragma once
#include "csic_kernel_ops.h"

namespace csic {

constexpr int CNT_T = CSTAT_T, CNT_WAVES = CNT_T / 64;
constexpr int CNT_LDS_BINS = 512;                              // per wave
constexpr int CNT_K = 4;                                       // loads (chunks / groups) in flight per lane
constexpr uint32_t CNT_BLOCK = (uint32_t)CSTAT_BLOCK_SAMPLES, CNT_WAVE = CNT_BLOCK / CNT_WAVES;
static_assert(CNT_T == 256 && CNT_LDS_BINS == 2 * CNT_T, "thread t flushes bins t and t + 256");
static_assert(CNT_WAVE % (16 * 64 * CNT_K) == 0 && CNT_WAVE % (32 * 64 * CNT_K) == 0, "a wave's span is whole rounds of either fast kernel");

typedef unsigned long long CSIC_GLOBAL *gcount_t;

// The kernels' argument, or its base.  The initialisers are also what lets a struct that extends it start in its tail padding, so
// that CsArgs keeps the layout it had (ndw at byte 60): the assertion below fails if an edit takes that away.
struct CountArgs {
    const uint8_t *src = nullptr;          // source frames, frame_bytes apart
    unsigned long long *res = nullptr;     // the result as 64-bit words, P::STRIDE per frame
    int64_t frame_bytes = 0;
    int64_t off[3] = {};                   // plane offsets
    uint32_t n[3] = {};                    // samples per plane
};
struct CountArgsTailProbe : CountArgs { uint32_t first; };
static_assert(sizeof(CountArgs) == 64 && sizeof(CountArgsTailProbe) == 64, "a derived struct's first dword sits in CountArgs' tail padding");

// ------------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------------
// source: 16 bytes (16-byte aligned), a dword (4-byte aligned) or a byte at a byte offset into the frame_bytes of the frame
template <bool NT> __device__ __forceinline__ u32x4 count_ld16(const CountArgs &e, gcbyte_t fb, int64_t off) { return by_ld16<NT>(e.frame_bytes, fb, off); }
template <bool NT> __device__ __forceinline__ uint32_t count_ld4(const CountArgs &e, gcbyte_t fb, int64_t off) { return by_ld4<NT>(e.frame_bytes, fb, off); }
__device__ __forceinline__ uint32_t count_ld1(const CountArgs &e, gcbyte_t fb, int64_t off) { return by_ld1(e.frame_bytes, fb, off); }

__device__ __forceinline__ gcbyte_t count_frame(const CountArgs &e) { return frame_at_z(e.src, e.frame_bytes); }

struct CountLds { uint32_t h[CNT_WAVES][CNT_LDS_BINS]; };

// clears the block's bins and returns this wave's
__device__ __forceinline__ uint32_t *count_begin(CountLds &s)
{
    uint32_t *all = &s.h[0][0];
#pragma unroll
    for (int i = 0; i < CNT_WAVES * CNT_LDS_BINS / CNT_T; ++i) all[i * CNT_T + threadIdx.x] = 0;
    __syncthreads();
    return &s.h[threadIdx.x >> 6][0];
}

// the four waves' bins -> the frame's result: thread t owns bins t and t + 256
template <class P>
__device__ __forceinline__ void count_flush(const CountArgs &e, CountLds &s, int plane)
{
    __syncthreads();
    const gcount_t res = (gcount_t)(uintptr_t)e.res;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const uint32_t k0 = (uint32_t)half * CNT_T, k = k0 + threadIdx.x;
        if (!P::has_word(k)) continue;
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < CNT_WAVES; ++w) t += s.h[w][k];
        if (t) {
            const uint32_t at = P::index(plane, k0, threadIdx.x);
            CSIC_CHECK(at < P::STRIDE && blockIdx.z < 65535u);
            __hip_atomic_fetch_add(res + ((uint64_t)blockIdx.z * P::STRIDE + at), (unsigned long long)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The code in front of this lane's first sample of a step: `last` is the lane's own last code of the step, `carry` (wave-uniform)
// what was in front of the wave's first sample of the step; afterwards carry is what is in front of the next step's.
__device__ __forceinline__ uint32_t count_pred(uint32_t last, uint32_t &carry)
{
    const uint32_t up = (uint32_t)__shfl_up((int)last, 1, 64);
    const uint32_t pred = (threadIdx.x & 63u) == 0 ? carry : up;
    carry = (uint32_t)__shfl((int)last, 63, 64);
    return pred;
}

// chunk `ch` of a plane of n samples as four dwords: CHECK = the plane may end in or before it
template <bool NT, bool CHECK>
__device__ __forceinline__ u32x4 count_chunk(const CountArgs &e, gcbyte_t fb, int64_t plane_off, uint32_t ch, uint32_t n)
{
    if (!CHECK || 16u * ch + 16u <= n) return count_ld16<NT>(e, fb, plane_off + 16 * (int64_t)ch);
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t i = 16u * ch; i < n; ++i) w[(i >> 2) & 3u] |= count_ld1(e, fb, plane_off + i) << (8u * (i & 3u));
    return u32x4{w[0], w[1], w[2], w[3]};
}

// the byte walk of one wave over the CNT_WAVE samples from i0 on
template <bool NT, bool CHECK, class P>
__device__ __forceinline__ void count_bytes_body(const CountArgs &e, gcbyte_t fb, uint32_t *wh, int plane, uint32_t i0, const P &p)
{
    const uint32_t n = e.n[plane], lane = threadIdx.x & 63u;
    const int64_t off = e.off[plane];
    // in front of the wave's span: the byte before it, nothing at sample 0 (and nothing for a wave past the plane's end)
    uint32_t carry = 0;
    if (i0 > 0 && (!CHECK || i0 < n)) carry = p.code(count_ld1(e, fb, off + i0 - 1));
    for (uint32_t c0 = i0 / 16u; c0 < (i0 + CNT_WAVE) / 16u; c0 += 64u * CNT_K) {
        if (CHECK && 16u * c0 >= n) break;                                  // wave-uniform
        u32x4 v[CNT_K];
#pragma unroll
        for (int k = 0; k < CNT_K; ++k) v[k] = count_chunk<NT, CHECK>(e, fb, off, c0 + 64u * (uint32_t)k + lane, n);
#pragma unroll
        for (int k = 0; k < CNT_K; ++k) {
            const uint32_t first = 16u * (c0 + 64u * (uint32_t)k + lane);
            const uint32_t w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
            uint32_t prev = count_pred(p.code(w[3] >> 24), carry);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t c = p.code((w[j >> 2] >> (8 * (j & 3))) & 0xFFu);
                if (!CHECK || first + (uint32_t)j < n) p.bump(wh, c, prev);
                prev = c;
            }
        }
    }
}

// The shell of a counting kernel whose waves walk spans: the block-uniform exit before any barrier, begin, the wave's first sample,
// the plane's last block through the checked body, flush.  body(check, fb, wh, i0) walks CNT_WAVE samples from i0 on with
// CHECK = decltype(check)::value.
template <class P, class Body>
__device__ __forceinline__ void count_block(const CountArgs &e, int plane, Body body)
{
    __shared__ CountLds lds;
    const uint32_t b0 = blockIdx.x * CNT_BLOCK;
    if (b0 >= e.n[plane]) return;                                           // block-uniform, before any barrier
    uint32_t *wh = count_begin(lds);
    const uint32_t i0 = b0 + (threadIdx.x >> 6) * CNT_WAVE;
    const gcbyte_t fb = count_frame(e);
    if (e.n[plane] - b0 >= CNT_BLOCK) body(std::false_type{}, fb, wh, i0);
    else                              body(std::true_type{}, fb, wh, i0);
    count_flush<P>(e, lds, plane);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// the three planes of the plan's CSIC_FMT_PLANAR frame
inline void count_fill_planar(const csic_plan *pl, CountArgs *e)
{
    csic_planar_layout G;
    planar_layout(pl->g, &pl->p, &G);
    e->n[0] = (uint32_t)((int64_t)G.y_width * G.y_height);
    e->n[1] = e->n[2] = (uint32_t)G.chroma_samples;
    e->off[0] = G.y_offset; e->off[1] = G.cb_offset; e->off[2] = G.cr_offset;
    e->frame_bytes = G.frame_bytes;
}

// What csic_code_stats_device and csic_qsweep_hist_device refuse alike.  The units word three of the messages differently, so each
// passes its own whole text: `frames_fmt` (with one %d for nframes), `res_msg`, `size_msg`.
inline int count_check_frames(int32_t nframes, const char *frames_fmt)
{
    if (nframes < 1 || nframes > 65535) return set_error(CSIC_EINVAL_SIZE, frames_fmt, nframes);
    return CSIC_OK;
}
inline int count_check_buffers(int32_t nframes, const char *frames_fmt, const void *d_src, const void *d_res, const char *res_msg)
{
    const int st = count_check_frames(nframes, frames_fmt);
    if (st != CSIC_OK) return st;
    if ((uintptr_t)d_src & 255u) return set_error(CSIC_EINVAL_SIZE, "a planar frame buffer must be 256-byte aligned");
    if ((uintptr_t)d_res & 7u) return set_error(CSIC_EINVAL_SIZE, "%s", res_msg);
    return CSIC_OK;
}
inline int count_check_size(const Geometry &g, const char *size_msg)
{
    if ((int64_t)g.W * g.H >= ((int64_t)1 << 31)) return set_error(CSIC_EINVAL_SIZE, "%s", size_msg);
    return CSIC_OK;
}

} // namespace csic
