// csic_decode.hip -- csic_decode_*: a compressed frame (bit-packed planar, planar, or the packed output itself) back to a frame of
// the ORIGINAL size, width x height packed pixels, by replication: decode(r, c) = o(r / f, c / f), o = the packed output of the
// plan's parameters (definition in include/csic.h).  The pairing is the one csic_distortion_* measures, so
// SSE(x, decode(compress(x))) == distortion(x).
//
// Kernels (wave64; a write stream of 4 W H bytes behind a small read; no LDS, no MFMA):
//   k_decode<SRC, FMT, F, NT>   the fast kernel.  One lane owns one 16-byte PIECE of the output -- 4 consecutive pixels of an output row
//                      -- and stores it to the F output rows that its source row expands to: F 16-byte non-temporal stores, and the
//                      64 lanes of a wave write one contiguous 1 KiB run per store.  The piece comes from NP = 4 / 2 / 1 / 1 consecutive
//                      source positions at F = 1 / 2 / 4 / 8 (planar sources: the two dwords that hold their codes in each plane,
//                      k_rbits' replay rule, PLANAR being the bit-packed frame at 8 / 8 / 8; packed sources: one 16 / 8 / 4-byte load),
//                      so the inverse transform runs once per source pixel up to F = 4 and twice at F = 8.  K = 4 / 2 / 1 pieces per
//                      lane, spaced by the block size, all loads issued before any arithmetic.  Conditions (plan_decode, csic_select.cpp): width % 4 == 0
//                      (pieces tile the rows; the NP positions of a piece then start at a multiple of NP in a chroma row whose length
//                      is a multiple of NP, whatever the order class), width * height <= 2^30 (32-bit byte offsets), output and packed source
//                      16-byte aligned.  The height is free: a ragged last source row stores fewer rows.
//                      (The first version had a lane decode 4 source pixels and store their whole F x F expansion, F 16-byte stores
//                      per row at a lane stride of 16 F bytes: 27.8 % of 8 TB/s at factor 2 and 8.6 % at factor 4 on 8192 x 8192,
//                      DESIGN.md 4.4 -- partial-line non-temporal stores do not combine.)
//   k_decode_gen<SRC, FMT>      the general kernel: one output pixel per lane straight from the definition, 4-byte accesses.  Ragged
//                      shapes, buffers that are only 4-byte aligned, CSIC_TUNE_VARIANT 9, CSIC_TUNE_NO_VECTOR, CSIC_TUNE_FORCE_GENERIC.
//   At factor 1 a planar source IS a reconstruct: csic_reconstruct_bits_device / csic_reconstruct_device (k_rbits / k_recon) are
//   called, and csic_decode_kernel_name says so.  (Not for a batch of frames whose W * H is not a multiple of 4: those kernels store
//   16 bytes at a time from each frame's base, which only the first frame's alignment check covers.)
//   k_view<LS, SRC, FMT, NT>, k_view_gen<SRC, FMT>   csic_decode_view_*: a window of the decoded frame under an s x s box, without the
//                      frame -- described in front of them, below.
// The planes are read through csic_plane_read.h (the chroma sample of a position, the window of a bit plane, the per-position read of
// k_decode_gen), which k_recon and k_rbits use too.  Every global access goes through the accessors of csic_kernel_ops.h, which the
// CSIC_DEBUG build range-checks; the forwards below name the limits: loads against the source frame's bytes, stores against the
// W * H pixels of the output frame.
#include <cstdio>
#include <cstring>

#include "csic_kernel_ops.h"
#include "csic_plane_read.h"

namespace csic {

enum { S_ARGB = CSIC_FMT_ARGB8888, S_YCC = CSIC_FMT_YCBCR888X, S_PLANAR = CSIC_FMT_PLANAR, S_BITS = CSIC_FMT_PLANAR_BITS };

// the kernels' argument
struct DecArgs {
    const uint8_t *src;            // source frames, src_frame_bytes apart
    uint32_t *dst;                 // W * H pixels per frame, back to back
    int64_t off[3], nbytes[3];     // planar sources: plane offsets and the bytes each plane's samples occupy (Y, Cb, Cr)
    int64_t src_frame_bytes;       // planar: frame_bytes; packed: 4 n
    int64_t n, out_px;             // source positions (out_width * out_height); output pixels (W * H)
    int32_t q[3];                  // bits per sample (8 for PLANAR)
    int32_t Wm, Wc, lhe, lve, replay_last;
    uint32_t mWm, kWm, mP, kP, mW, kW;     // exact j / Wm, t / P, t / W (magic_div)
    int32_t W, H, Wo, lf, T;       // lf = log2 factor; T = threads per block
    int32_t P;                     // fast kernel: pieces (4 output pixels) per row, W / 4
    int64_t npieces, nwhole;       // fast kernel: P * out_height pieces; those of source rows that expand to F whole output rows
};

// source: a dword at a byte offset (4-byte aligned), 4 or 2 pixels at a pixel offset, all against the source frame's bytes; output: 1 or
// 4 pixels at a pixel offset against the W * H pixels of the output frame
__device__ __forceinline__ uint32_t dsrc4(const DecArgs &e, gcbyte_t fb, int64_t off) { return by_ld4<false>(e.src_frame_bytes, fb, off); }
template <bool NT> __device__ __forceinline__ u32x4 dsrc16(const DecArgs &e, gcbyte_t fb, uint32_t px) { return px_ld4n<NT>(e.src_frame_bytes >> 2, (gin_t)fb, px); }
template <bool NT> __device__ __forceinline__ u32x2 dsrc8(const DecArgs &e, gcbyte_t fb, uint32_t px) { return px_ld2n<NT>(e.src_frame_bytes >> 2, (gin_t)fb, px); }
__device__ __forceinline__ void dout1(const DecArgs &e, gout_t out, int64_t px, uint32_t v) { px_st1<false>(e.out_px, out, px, v); }
template <bool NT> __device__ __forceinline__ void dout4(const DecArgs &e, gout_t out, uint32_t px, u32x4 v) { px_st4n<NT>(e.out_px, out, px, v); }

__device__ __forceinline__ gcbyte_t dec_src(const DecArgs &e) { return frame_at_z(e.src, e.src_frame_bytes); }
__device__ __forceinline__ gout_t dec_dst(const DecArgs &e) { return (gout_t)(uintptr_t)e.dst + (int64_t)blockIdx.z * e.out_px; }

// planar sources: the bit planes of csic_plane_read.h (csic_planar_bits_layout; PLANAR = the same at 8 bits per sample)
template <int SRC> using DecPlanes = BitPlanes<DecArgs, &DecArgs::src_frame_bytes, SRC == S_PLANAR>;

template <int SRC> __device__ __forceinline__ uint32_t dec_q(const DecArgs &e, int p) { return SRC == S_PLANAR ? 8u : (uint32_t)e.q[p]; }

// source position j by the definition: the packed pixel o[j] in FMT
template <int SRC, int FMT>
__device__ __forceinline__ uint32_t dec_pixel(const DecArgs &e, gcbyte_t fb, uint32_t j)
{
    if (SRC == S_ARGB || SRC == S_YCC) {
        const uint32_t v = dsrc4(e, fb, 4 * (int64_t)j);
        if (SRC == S_YCC && FMT == F_ARGB) return finish_y<F_ARGB>(v & 0xFFu, chroma_term_q<F_ARGB>((v >> 8) & 0xFFu, (v >> 16) & 0xFFu));
        return v;
    }
    return plane_pixel<FMT>(e, DecPlanes<SRC>{e, fb}, j);
}

// ------------------------------------------------------------------------------------------------
// the fast kernel
// ------------------------------------------------------------------------------------------------
// A lane owns one PIECE: 4 consecutive output pixels of one output row, written to the F output rows of its source row.  Its NP
// source positions (4 / F of them, at least 1) are consecutive and start at a multiple of NP.
template <int F> constexpr int dec_np() { return F == 1 ? 4 : F == 2 ? 2 : 1; }      // (pieces per lane: dec_pieces_per_lane, csic_select.h)

// what a lane holds of its source positions once its loads are back
struct DecGroup {
    uint32_t px[4];             // packed sources: the NP pixels
    uint32_t yw, bw, rw, sh;    // planar sources: the windows that start at the first Y / Cb / Cr code; position i takes chroma
};                              // code i >> sh

template <int SRC, int NP, bool NT>
__device__ __forceinline__ DecGroup dec_load(const DecArgs &e, gcbyte_t fb, uint32_t j0)
{
    DecGroup g;
    g.px[0] = g.px[1] = g.px[2] = g.px[3] = 0;
    g.yw = g.bw = g.rw = g.sh = 0;
    if (SRC == S_YCC) {
        if (NP == 4) { const u32x4 v = dsrc16<NT>(e, fb, j0); g.px[0] = v.x; g.px[1] = v.y; g.px[2] = v.z; g.px[3] = v.w; }
        else if (NP == 2) { const u32x2 v = dsrc8<NT>(e, fb, j0); g.px[0] = v.x; g.px[1] = v.y; }
        else g.px[0] = dsrc4(e, fb, (int64_t)(uint64_t)(j0 << 2));
        return g;
    }
    // module_width % NP == 0 and j0 % NP == 0: the positions lie in one chroma row at a column that is a multiple of NP -- their
    // samples are consecutive codes, position i taking code i >> log2 hold_h, or ONE code on a row that replays the last sample of
    // the row above
    const uint32_t r = (uint32_t)(((uint64_t)j0 * e.mWm) >> e.kWm), c0 = j0 - r * (uint32_t)e.Wm;
    const bool replay = (r & ((1u << e.lve) - 1u)) != 0 && e.replay_last;
    const uint64_t k0 = chroma_index<uint64_t>(e, r, c0);
    g.sh = replay ? 2u : (uint32_t)e.lhe;
    const DecPlanes<SRC> s{e, fb};
    g.yw = s.template y_word<false>(j0);
    g.bw = s.c_word(1, k0);
    g.rw = s.c_word(2, k0);
    return g;
}

// the NP packed pixels: the chroma half of the inverse transform once per DISTINCT sample
template <int SRC, int FMT, int NP>
__device__ __forceinline__ void dec_group_pixels(const DecArgs &e, const DecGroup &g, uint32_t o[4])
{
    if (SRC == S_YCC) {
#pragma unroll
        for (int i = 0; i < NP; ++i)
            o[i] = FMT == F_ARGB ? finish_y<F_ARGB>(g.px[i] & 0xFFu, chroma_term_q<F_ARGB>((g.px[i] >> 8) & 0xFFu, (g.px[i] >> 16) & 0xFFu))
                                 : g.px[i];
        return;
    }
    const uint32_t qy = dec_q<SRC>(e, 0), qb = dec_q<SRC>(e, 1), qr = dec_q<SRC>(e, 2);
    const ChromaTerm t0 = chroma_term_q<FMT>(code_at(g.bw, 0, qb), code_at(g.rw, 0, qr));
    o[0] = finish_y<FMT>(code_at(g.yw, 0, qy), t0);
    if (NP == 1) return;
    if (g.sh != 0u) {                                                     // positions 0 and 1 share a sample
        o[1] = finish_y<FMT>(code_at(g.yw, 1, qy), t0);
        if (NP == 2) return;
        const ChromaTerm t1 = g.sh == 2u ? t0 : chroma_term_q<FMT>(code_at(g.bw, 1, qb), code_at(g.rw, 1, qr));
        o[2] = finish_y<FMT>(code_at(g.yw, 2, qy), t1);
        o[3] = finish_y<FMT>(code_at(g.yw, 3, qy), t1);
        return;
    }
#pragma unroll
    for (int i = 1; i < NP; ++i)
        o[i] = finish_y<FMT>(code_at(g.yw, i, qy), chroma_term_q<FMT>(code_at(g.bw, i, qb), code_at(g.rw, i, qr)));
}

template <int SRC, int FMT, int F, bool NT, bool CHECK>
__device__ __forceinline__ void decode_body(const DecArgs &e, gcbyte_t fb, gout_t out, uint32_t t0, uint32_t T, uint32_t npieces)
{
    constexpr int K = dec_pieces_per_lane(F), NP = dec_np<F>();
    constexpr int LF = F == 1 ? 0 : F == 2 ? 1 : F == 4 ? 2 : 3;
    DecGroup grp[K];
    uint32_t ro[K], pc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t t = t0 + (uint32_t)k * T, tc = CHECK ? min(t, npieces - 1u) : t;
        // piece tc: source row ro, piece column pc (output columns 4 pc .. 4 pc + 3 <- source columns (4 pc) >> LF ..)
        ro[k] = (uint32_t)(((uint64_t)tc * e.mP) >> e.kP);
        pc[k] = tc - ro[k] * (uint32_t)e.P;
        grp[k] = dec_load<SRC, NP, NT>(e, fb, ro[k] * (uint32_t)e.Wo + ((4u * pc[k]) >> LF));
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (CHECK && t0 + (uint32_t)k * T >= npieces) continue;
        uint32_t o[4];
        dec_group_pixels<SRC, FMT, NP>(e, grp[k], o);
        const u32x4 piece = F == 1 ? u32x4{o[0], o[1], o[2], o[3]} : F == 2 ? u32x4{o[0], o[0], o[1], o[1]} : u32x4{o[0], o[0], o[0], o[0]};
        // the same 16 bytes to the F output rows of the source row (fewer on a ragged last one): lanes of a wave store 1 KiB runs
        const uint32_t row0 = ro[k] << LF, base = row0 * (uint32_t)e.W + 4u * pc[k];
        const uint32_t rows = CHECK ? min((uint32_t)F, (uint32_t)e.H - row0) : (uint32_t)F;
#pragma unroll
        for (int i = 0; i < F; ++i)
            if (!CHECK || (uint32_t)i < rows) dout4<NT>(e, out, base + (uint32_t)i * (uint32_t)e.W, piece);
    }
    if (!CHECK) keep_tail_apart();
}

template <int SRC, int FMT, int F, bool NT>
__global__ void __launch_bounds__(256) k_decode(DecArgs e)
{
    const uint32_t T = (uint32_t)e.T;
    const uint32_t npieces = (uint32_t)e.npieces;                      // (W / 4) * out_height
    const uint32_t per_block = T * (uint32_t)dec_pieces_per_lane(F);
    const uint32_t b0 = blockIdx.x * per_block;
    const gcbyte_t fb = dec_src(e);
    const gout_t out = dec_dst(e);
    // straight-line body: a whole block of pieces, none of them in a ragged last source row
    if (b0 + per_block <= (uint32_t)e.nwhole) decode_body<SRC, FMT, F, NT, false>(e, fb, out, b0 + threadIdx.x, T, npieces);
    else                                       decode_body<SRC, FMT, F, NT, true>(e, fb, out, b0 + threadIdx.x, T, npieces);
}

// ------------------------------------------------------------------------------------------------
// the general kernel: one output pixel per lane, from the definition
// ------------------------------------------------------------------------------------------------
template <int SRC, int FMT>
__global__ void __launch_bounds__(256) k_decode_gen(DecArgs e)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;    // out_px < 2^31 (csic_decode_device)
    if (t >= e.out_px) return;
    const uint32_t r = (uint32_t)(((uint64_t)t * e.mW) >> e.kW), c = (uint32_t)t - r * (uint32_t)e.W;
    const uint32_t j = (r >> e.lf) * (uint32_t)e.Wo + (c >> e.lf);
    dout1(e, dec_dst(e), t, dec_pixel<SRC, FMT>(e, dec_src(e), j));
}

// ------------------------------------------------------------------------------------------------
// view decode: a window of the decoded frame, reduced by an s x s box (csic_decode_view_*, definition in include/csic.h)
// ------------------------------------------------------------------------------------------------
// An output pixel is the rounded mean of the s x s decoded pixels under its box.  decode replicates, so the box is walked over the
// DISTINCT source positions it touches -- decimated rows (ys >> lf) .. ((ys + s - 1) >> lf) and the matching columns -- each
// inverse-transformed once and weighted by the decoded pixels it stands for, wy * wx (the weights add up to s * s).  The four byte
// sums ride in two registers as 16-bit pairs: at most 255 * 256 + 128 = 65 408 each.
//   k_view<LS, SRC, FMT, NT>  the fast kernel: a lane owns 4 consecutive output pixels of a row and stores them as one 16-byte piece,
//                      so a wave's store is one contiguous 1 KiB run.  Per decimated row the 4 boxes are walked in chunks of CH
//                      positions; a chunk is three windows of the planes (Y, Cb, Cr: the codes of CH consecutive positions and of
//                      their chroma samples), and the windows of all 4 boxes are loaded before the first inverse transform.  The
//                      chroma half of the transform runs once per run of equal chroma samples inside a chunk.  Where the view's
//                      origin is a multiple of f and s >= f no position straddles a box: the weights drop out (view_walk, WHOLE).
//   k_view_gen<SRC, FMT>      the general kernel: one output pixel per lane straight from the definition, dec_pixel per position.
struct ViewArgs {
    DecArgs d;                     // the source side, as for k_decode (d.dst, d.T, d.P and the piece counts are not used)
    uint32_t *dst;                 // vw * vh pixels per frame, back to back
    int64_t view_px, units;        // vw * vh; lanes with work (plan_view)
    int32_t x0, y0, vw, vh, ls;
    int32_t ncx, ncy;              // decimated columns / rows a box can touch (plan_view)
    int32_t whole;                 // every position a box touches lies inside it: origin % f == 0 and s >= f
    int32_t U, T;                  // units per output row; threads per block
    uint32_t mU, kU;               // exact t / U
};

__device__ __forceinline__ gout_t view_dst(const ViewArgs &v) { return (gout_t)(uintptr_t)v.dst + (int64_t)blockIdx.z * v.view_px; }

// decoded pixels that decimated cell d -- [d f, d f + f) along one axis -- shares with the box [b, b + s)
__device__ __forceinline__ uint32_t view_overlap(uint32_t d, uint32_t lf, uint32_t b, uint32_t s)
{
    return (uint32_t)max((int)min((d + 1u) << lf, b + s) - (int)max(d << lf, b), 0);
}

// the four byte sums of a box as 16-bit pairs: bytes 0 and 2 in `lo`, 1 and 3 in `hi`
struct ViewSum { uint32_t lo, hi; };
__device__ __forceinline__ void view_add(ViewSum &a, uint32_t px, uint32_t w)
{
    a.lo += (px & 0x00FF00FFu) * w;
    a.hi += ((px >> 8) & 0x00FF00FFu) * w;
}
// (sum + s s / 2) >> 2 log2 s, byte by byte.  Each pair's upper sum shifts into bits the mask drops (2 LS <= 8).
template <int LS> __device__ __forceinline__ uint32_t view_mean(const ViewSum &a)
{
    constexpr uint32_t half = LS == 0 ? 0u : (1u << (2 * LS - 1)) * 0x00010001u;
    return (((a.lo + half) >> (2 * LS)) & 0x00FF00FFu) | ((((a.hi + half) >> (2 * LS)) & 0x00FF00FFu) << 8);
}
__device__ __forceinline__ uint32_t view_mean(const ViewSum &a, int ls)
{
    const uint32_t half = ls == 0 ? 0u : (1u << (2 * ls - 1)) * 0x00010001u;
    return (((a.lo + half) >> (2 * ls)) & 0x00FF00FFu) | ((((a.hi + half) >> (2 * ls)) & 0x00FF00FFu) << 8);
}

template <int SRC, int FMT>
__global__ void __launch_bounds__(256) k_view_gen(ViewArgs v)
{
    const DecArgs &e = v.d;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;    // view_px < 2^31
    if (t >= v.view_px) return;
    const uint32_t r = (uint32_t)(((uint64_t)t * v.mU) >> v.kU), c = (uint32_t)t - r * (uint32_t)v.U;
    const uint32_t s = 1u << v.ls, lf = (uint32_t)e.lf;
    const uint32_t ys = (uint32_t)v.y0 + r * s, xs = (uint32_t)v.x0 + c * s;
    const gcbyte_t fb = dec_src(e);
    ViewSum a = {0u, 0u};
    for (uint32_t dr = ys >> lf; dr <= (ys + s - 1u) >> lf; ++dr) {
        const uint32_t wy = view_overlap(dr, lf, ys, s);
        for (uint32_t dc = xs >> lf; dc <= (xs + s - 1u) >> lf; ++dc)
            view_add(a, dec_pixel<SRC, FMT>(e, fb, dr * (uint32_t)e.Wo + dc), wy * view_overlap(dc, lf, xs, s));
    }
    px_st1<false>(v.view_px, view_dst(v), t, view_mean(a, v.ls));
}

// CH consecutive stream positions from j0 on, none past jlast (positions past it repeat jlast's chroma and are weighted 0)
template <int CH> struct ViewChunk {
    uint32_t px[CH];            // packed sources: the pixels
    uint32_t yw, bw, rw;        // planar sources: the windows that start at the first Y / Cb / Cr code
    uint32_t k0, k[CH];         // the chroma sample of each position
};

template <int SRC, int CH>
__device__ __forceinline__ ViewChunk<CH> view_load(const DecArgs &e, gcbyte_t fb, uint32_t j0, uint32_t jlast)
{
    ViewChunk<CH> g;
    if (SRC == S_YCC) {
#pragma unroll
        for (int i = 0; i < CH; ++i) g.px[i] = dsrc4(e, fb, 4 * (int64_t)min(j0 + (uint32_t)i, jlast));
        g.yw = g.bw = g.rw = g.k0 = 0;
        return g;
    }
    const DecPlanes<SRC> s{e, fb};
    const uint32_t imax = jlast - j0;                                     // the live positions are j0 .. j0 + imax
    const uint32_t r0 = (uint32_t)(((uint64_t)j0 * e.mWm) >> e.kWm), cc0 = j0 - r0 * (uint32_t)e.Wm;
    if (cc0 + min((uint32_t)(CH - 1), imax) < (uint32_t)e.Wm) {           // ... in one row of the chroma counters: one division for the chunk
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            g.k[i] = chroma_index<uint32_t>(e, r0, cc0 + min((uint32_t)i, imax));      // chroma samples <= positions < 2^31
            g.px[i] = 0;
        }
    } else {                                                              // a chunk across rows of the counters (spatial before chroma, narrow frames)
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const uint32_t j = j0 + min((uint32_t)i, imax);
            const uint32_t r = (uint32_t)(((uint64_t)j * e.mWm) >> e.kWm), c = j - r * (uint32_t)e.Wm;
            g.k[i] = chroma_index<uint32_t>(e, r, c);
            g.px[i] = 0;
        }
    }
    g.k0 = g.k[0];
    g.yw = s.template y_word<false>(j0);
    g.bw = s.c_word(1, (uint64_t)g.k0);
    g.rw = s.c_word(2, (uint64_t)g.k0);
    return g;
}

// position i of a chunk as a packed pixel; t / kt: the chroma term of the chunk's previous position and the sample it belongs to
template <int SRC, int FMT, int CH>
__device__ __forceinline__ uint32_t view_chunk_pixel(const DecArgs &e, gcbyte_t fb, const ViewChunk<CH> &g, int i, ChromaTerm &t, uint32_t &kt)
{
    if (SRC == S_YCC)
        return FMT == F_ARGB ? finish_y<F_ARGB>(g.px[i] & 0xFFu, chroma_term_q<F_ARGB>((g.px[i] >> 8) & 0xFFu, (g.px[i] >> 16) & 0xFFu)) : g.px[i];
    const uint32_t qy = dec_q<SRC>(e, 0), qb = dec_q<SRC>(e, 1), qr = dec_q<SRC>(e, 2);
    if (i == 0 || g.k[i] != kt) {
        const uint32_t d = g.k[i] - g.k0;
        uint32_t cb, cr;
        if (d < 4u) { cb = code_at(g.bw, d, qb); cr = code_at(g.rw, d, qr); }          // a window holds 32 / q >= 4 codes
        else { const DecPlanes<SRC> s{e, fb}; cb = s.c_one(1, (uint64_t)g.k[i]); cr = s.c_one(2, (uint64_t)g.k[i]); }   // a chunk across stream rows
        t = chroma_term_q<FMT>(cb, cr);
        kt = g.k[i];
    }
    return finish_y<FMT>(code_at(g.yw, (uint32_t)i, qy), t);
}

// The boxes of a lane: VIEW_PX consecutive output pixels whose boxes start at (xs + m S, ys).  WHOLE: every position a box touches lies
// inside it (the view's origin is a multiple of f, S >= f) and a box row is whole chunks (ncx % CH == 0) -- every weight is f * f, so
// the sums are taken over the positions and the f * f goes into view_mean's shift; no overlap is computed and no load is clamped.
template <int LS, int SRC, int FMT, bool WHOLE>
__device__ __forceinline__ void view_walk(const ViewArgs &v, gcbyte_t fb, uint32_t xs, uint32_t ys, ViewSum a[VIEW_PX])
{
    constexpr uint32_t S = 1u << LS;
    constexpr int CH = S >= 4u ? 4 : (int)S;
    const DecArgs &e = v.d;
    const uint32_t lf = (uint32_t)e.lf;
    const uint32_t dr0 = ys >> lf, dr1 = (ys + S - 1u) >> lf;
    uint32_t c0[VIEW_PX], c1[VIEW_PX];
#pragma unroll
    for (int m = 0; m < VIEW_PX; ++m) {
        c0[m] = (xs + (uint32_t)m * S) >> lf;
        c1[m] = (xs + (uint32_t)m * S + S - 1u) >> lf;
        a[m] = ViewSum{0u, 0u};
    }
    // (neither loop is unrolled: with the cheap YCbCr body hipcc unrolled them eightfold at S = 1 and took all 256 VGPRs)
#pragma unroll 1
    for (uint32_t iy = 0; iy < (uint32_t)v.ncy; ++iy) {
        const uint32_t wy = WHOLE ? 1u : view_overlap(dr0 + iy, lf, ys, S);   // 0 on a row past the box: it loads the box's last row again
        const uint32_t row = (WHOLE ? dr0 + iy : min(dr0 + iy, dr1)) * (uint32_t)e.Wo;
#pragma unroll 1
        for (uint32_t ix = 0; ix < (uint32_t)v.ncx; ix += (uint32_t)CH) {
            ViewChunk<CH> g[VIEW_PX];
#pragma unroll
            for (int m = 0; m < VIEW_PX; ++m)
                g[m] = view_load<SRC, CH>(e, fb, row + (WHOLE ? c0[m] + ix : min(c0[m] + ix, c1[m])), row + c1[m]);
#pragma unroll
            for (int m = 0; m < VIEW_PX; ++m) {
                ChromaTerm ct = {0, 0, 0, 0u};
                uint32_t kt = 0;
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const uint32_t px = view_chunk_pixel<SRC, FMT, CH>(e, fb, g[m], i, ct, kt);
                    if (WHOLE) { a[m].lo += px & 0x00FF00FFu; a[m].hi += (px >> 8) & 0x00FF00FFu; continue; }
                    // column c0 + ix + i of the box; past c1 the weight is 0, whatever the chunk holds there
                    view_add(a[m], px, wy * view_overlap(c0[m] + ix + (uint32_t)i, lf, xs + (uint32_t)m * S, S));
                }
            }
        }
    }
}

template <int LS, int SRC, int FMT, bool NT>
__global__ void __launch_bounds__(256) k_view(ViewArgs v)
{
    constexpr uint32_t S = 1u << LS;
    constexpr int CH = S >= 4u ? 4 : (int)S;
    const uint32_t t = blockIdx.x * (uint32_t)v.T + threadIdx.x;          // units <= 2^28
    if (t >= (uint32_t)v.units) return;
    const uint32_t r = (uint32_t)(((uint64_t)t * v.mU) >> v.kU), pc = t - r * (uint32_t)v.U;
    const uint32_t ys = (uint32_t)v.y0 + r * S, xs = (uint32_t)v.x0 + (uint32_t)VIEW_PX * pc * S;
    const gcbyte_t fb = dec_src(v.d);
    ViewSum a[VIEW_PX];
    u32x4 piece;
    if (v.whole && v.ncx % CH == 0) {                                     // (uniform)
        view_walk<LS, SRC, FMT, true>(v, fb, xs, ys, a);
        const int sh = LS - v.d.lf;                                       // (f f sum + s s / 2) >> 2 LS == (sum + n / 2) >> log2 n, n = (s / f)^2
        piece = u32x4{view_mean(a[0], sh), view_mean(a[1], sh), view_mean(a[2], sh), view_mean(a[3], sh)};
    } else {
        view_walk<LS, SRC, FMT, false>(v, fb, xs, ys, a);
        piece = u32x4{view_mean<LS>(a[0]), view_mean<LS>(a[1]), view_mean<LS>(a[2]), view_mean<LS>(a[3])};
    }
    px_st4n<NT>(v.view_px, view_dst(v), r * (uint32_t)v.vw + (uint32_t)VIEW_PX * pc, piece);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
using DecFn = void (*)(DecArgs);

static bool dec_is_planar(int src_format) { return src_format == CSIC_FMT_PLANAR || src_format == CSIC_FMT_PLANAR_BITS; }

// bytes between the source frames of a batch
static int64_t dec_src_frame_bytes(const csic_plan *pl, int src_format)
{
    if (src_format == CSIC_FMT_PLANAR_BITS) { csic_planar_bits_layout L; planar_bits_layout(pl->g, &pl->p, &L); return L.frame_bytes; }
    if (src_format == CSIC_FMT_PLANAR) { csic_planar_layout L; planar_layout(pl->g, &pl->p, &L); return L.frame_bytes; }
    return 4 * (int64_t)pl->g.Wo * pl->g.Ho;
}

static void fill_dec_args(const csic_plan *pl, int src_format, DecArgs *e)
{
    std::memset(e, 0, sizeof *e);
    const Geometry &g = pl->g;
    csic_planar_bits_layout B;
    planar_bits_layout(g, &pl->p, &B);
    const csic_planar_layout &G = B.geometry;
    if (src_format == CSIC_FMT_PLANAR_BITS) {
        e->off[0] = B.y_offset; e->off[1] = B.cb_offset; e->off[2] = B.cr_offset;
        e->nbytes[0] = B.y_bytes; e->nbytes[1] = B.cb_bytes; e->nbytes[2] = B.cr_bytes;
        e->q[0] = B.y_bits; e->q[1] = B.cb_bits; e->q[2] = B.cr_bits;
    } else if (src_format == CSIC_FMT_PLANAR) {
        e->off[0] = G.y_offset; e->off[1] = G.cb_offset; e->off[2] = G.cr_offset;
        e->nbytes[0] = (int64_t)G.y_width * G.y_height; e->nbytes[1] = e->nbytes[2] = G.chroma_samples;
        e->q[0] = e->q[1] = e->q[2] = 8;
    }
    e->src_frame_bytes = dec_src_frame_bytes(pl, src_format);
    e->n = (int64_t)g.Wo * g.Ho;
    e->out_px = (int64_t)g.W * g.H;
    e->Wm = G.module_width; e->Wc = G.chroma_width; e->lhe = ilog2(G.hold_h); e->lve = ilog2(G.hold_v); e->replay_last = G.replay_last;
    magic_div((uint32_t)G.module_width, &e->mWm, &e->kWm);
    magic_div((uint32_t)g.W, &e->mW, &e->kW);
    e->W = g.W; e->H = g.H; e->Wo = g.Wo; e->lf = ilog2(g.f);
    e->P = g.W / 4 > 0 ? g.W / 4 : 1;
    magic_div((uint32_t)e->P, &e->mP, &e->kP);
    e->npieces = (int64_t)e->P * g.Ho;
    e->nwhole = (int64_t)e->P * (g.H / g.f);
}

static DecFn decode_kernel(DecodeKind kind, int src_format, int out_format, int f, bool nt)
{
    // an ARGB source is only ever replicated (ARGB -> YCbCr is refused): it takes the YCbCr -> YCbCr instantiations, a plain copy
    if (src_format == S_ARGB) { src_format = S_YCC; out_format = F_YCC; }
    return with_const<F_ARGB, F_YCC>(out_format, [&](auto fmt) {
        return with_const<S_BITS, S_PLANAR, S_YCC>(src_format, [&](auto s) -> DecFn {
            constexpr int SRC = CSIC_CONST(s), FMT = CSIC_CONST(fmt);
            if (kind == DEC_GEN) return k_decode_gen<SRC, FMT>;
            return with_const<true, false>(nt, [&](auto n) -> DecFn {
                constexpr bool NT = CSIC_CONST(n);
                if constexpr (SRC == S_YCC)
                    return with_const<1, 2, 4, 8>(f, [](auto ff) -> DecFn { return k_decode<SRC, FMT, CSIC_CONST(ff), NT>; });
                else                                                      // factor 1 from planes is k_rbits / k_recon
                    return with_const<2, 4, 8>(f, [](auto ff) -> DecFn { return k_decode<SRC, FMT, CSIC_CONST(ff), NT>; });
            });
        });
    });
}

using ViewFn = void (*)(ViewArgs);

static ViewFn view_kernel(const ViewPlan &vp, int src_format, int out_format, bool nt)
{
    if (src_format == S_ARGB) { src_format = S_YCC; out_format = F_YCC; }          // as decode_kernel: a plain copy under the box
    return with_const<F_ARGB, F_YCC>(out_format, [&](auto fmt) {
        return with_const<S_BITS, S_PLANAR, S_YCC>(src_format, [&](auto s) -> ViewFn {
            constexpr int SRC = CSIC_CONST(s), FMT = CSIC_CONST(fmt);
            if (vp.kind == VIEW_GEN) return k_view_gen<SRC, FMT>;
            return with_const<true, false>(nt, [&](auto n) -> ViewFn {
                constexpr bool NT = CSIC_CONST(n);
                return with_const<0, 1, 2, 3, 4>(vp.ls, [](auto l) -> ViewFn { return k_view<CSIC_CONST(l), SRC, FMT, NT>; });
            });
        });
    });
}

static int decode_check_formats(int32_t src_format, int32_t out_format)
{
    if (src_format < CSIC_FMT_ARGB8888 || src_format > CSIC_FMT_PLANAR_BITS)
        return set_error(CSIC_EINVAL_FORMAT, "csic_decode reads ARGB8888(0), YCBCR888X(1), PLANAR(2) or PLANAR_BITS(3). Got %d", src_format);
    if (out_format != CSIC_FMT_ARGB8888 && out_format != CSIC_FMT_YCBCR888X)
        return set_error(CSIC_EINVAL_FORMAT, "csic_decode writes ARGB8888(0) or YCBCR888X(1). Got %d", out_format);
    if (src_format == CSIC_FMT_ARGB8888 && out_format == CSIC_FMT_YCBCR888X)
        return set_error(CSIC_EINVAL_FORMAT, "csic_decode cannot turn an ARGB source into YCbCr: the inverse transform has no inverse");
    return CSIC_OK;
}

} // namespace csic

using namespace csic;

extern "C" {

const char *csic_decode_kernel_name(const csic_plan *plan, int32_t src_format, int32_t out_format)
{
    static thread_local char buf[96];
    if (!plan || decode_check_formats(src_format, out_format) != CSIC_OK) return "";
    DecodePlan dp;                                                      // one frame in aligned buffers
    plan_decode(plan->p, plan->g, plan->tune, src_format, 0, 1, &dp);
    decode_kernel_name(dp, plan->g, plan->tune, src_format, out_format, buf, sizeof buf);
    return buf;
}

int csic_decode_device(csic_plan *plan, const void *d_src, int32_t src_format, void *d_out, int32_t out_format, int32_t nframes,
                       void *hip_stream)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    if (!d_src || !d_out) return set_error(CSIC_EINVAL_NULL, "device buffer is NULL");
    if (nframes <= 0) return set_error(CSIC_EINVAL_SIZE, "nframes must be positive. Got %d", nframes);
    int st = decode_check_formats(src_format, out_format);
    if (st != CSIC_OK) return st;
    const bool planar = dec_is_planar(src_format);
    if (planar && ((uintptr_t)d_src & 255u)) return set_error(CSIC_EINVAL_SIZE, "a planar frame buffer must be 256-byte aligned");
    if (((uintptr_t)d_src & 3u) || ((uintptr_t)d_out & 3u)) return set_error(CSIC_EINVAL_SIZE, "source and output must be 4-byte aligned");
    const Geometry &g = plan->g;
    if ((int64_t)g.W * g.H >= ((int64_t)1 << 31)) return set_error(CSIC_EINVAL_SIZE, "frame too large for csic_decode_device");
    DecodePlan dp;                                                      // kind, threads and blocks: csic_select.cpp
    plan_decode(plan->p, g, plan->tune, src_format, (uintptr_t)d_out | (planar ? 0 : (uintptr_t)d_src), nframes, &dp);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (dp.kind == DEC_RECON)
        return src_format == CSIC_FMT_PLANAR_BITS ? csic_reconstruct_bits_device(plan, d_src, d_out, nframes, out_format, hip_stream)
                                                  : csic_reconstruct_device(plan, d_src, d_out, nframes, out_format, hip_stream);
    const DecFn fn = decode_kernel(dp.kind, src_format, out_format, g.f, !plan->tune.no_nt);
    CSIC_DEVICE_SCOPE(plan->device);
    st = for_frame_batches(nframes, [&](int f0, int nz) {
        DecArgs e;
        fill_dec_args(plan, src_format, &e);
        e.src = static_cast<const uint8_t *>(d_src) + (int64_t)f0 * e.src_frame_bytes;
        e.dst = static_cast<uint32_t *>(d_out) + (int64_t)f0 * e.out_px;
        e.T = dp.T;
        return launch(fn, dim3(dp.grid.x, 1, (unsigned)nz), dim3(dp.block.x, 1, 1), stream, e);
    });
    if (st != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

int csic_decode_host(csic_plan *plan, const void *src, size_t src_bytes, int32_t src_format, uint32_t *out, size_t out_px,
                     int32_t out_format, int32_t nframes)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    if (!src || !out) return set_error(CSIC_EINVAL_NULL, "host buffer is NULL");
    if (nframes <= 0) return set_error(CSIC_EINVAL_SIZE, "nframes must be positive. Got %d", nframes);
    int st = decode_check_formats(src_format, out_format);
    if (st != CSIC_OK) return st;
    const Geometry &g = plan->g;
    const size_t need_src = (size_t)nframes * (size_t)dec_src_frame_bytes(plan, src_format);
    const size_t need_out = (size_t)nframes * (size_t)g.W * (size_t)g.H;
    if (src_bytes != need_src) return set_error(CSIC_EINVAL_SIZE, "expected %zu source bytes (%d frames), got %zu", need_src, nframes, src_bytes);
    if (out_px != need_out) return set_error(CSIC_EINVAL_SIZE, "expected room for %zu output pixels (%d frames), got %zu", need_out, nframes, out_px);
    CSIC_DEVICE_SCOPE(plan->device);
    DeviceStaging dev;
    void *d_src = dev.alloc(need_src), *d_out = dev.alloc(need_out * 4);
    dev.to_device(d_src, src, need_src);
    if (dev.ok()) {
        st = csic_decode_device(plan, d_src, src_format, d_out, out_format, nframes, nullptr);
        if (st == CSIC_OK) { dev.to_host(out, d_out, need_out * 4); dev.sync(); }
    }
    if (st != CSIC_OK) return st;
    if (!dev.ok()) return set_error(CSIC_EHIP, "csic_decode_host: %s", hipGetErrorString(dev.error()));
    clear_error();
    return CSIC_OK;
}

const char *csic_decode_view_kernel_name(const csic_plan *plan, int32_t src_format, int32_t out_format, const csic_view *view)
{
    static thread_local char buf[96];
    if (!plan || !view || decode_check_formats(src_format, out_format) != CSIC_OK || check_view(plan->g, *view) != CSIC_OK) return "";
    ViewPlan vp;                                                        // one frame in aligned buffers
    plan_view(plan->g, plan->tune, *view, 0, 1, &vp);
    view_kernel_name(vp, plan->tune, src_format, out_format, buf, sizeof buf);
    return buf;
}

int csic_decode_view_device(csic_plan *plan, const void *d_src, int32_t src_format, const csic_view *view, void *d_out, int32_t out_format,
                            int32_t nframes, void *hip_stream)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    if (!view) return set_error(CSIC_EINVAL_NULL, "view is NULL");
    if (!d_src || !d_out) return set_error(CSIC_EINVAL_NULL, "device buffer is NULL");
    if (nframes <= 0) return set_error(CSIC_EINVAL_SIZE, "nframes must be positive. Got %d", nframes);
    int st = decode_check_formats(src_format, out_format);
    if (st != CSIC_OK) return st;
    const Geometry &g = plan->g;
    st = check_view(g, *view);
    if (st != CSIC_OK) return st;
    const bool planar = dec_is_planar(src_format);
    if (planar && ((uintptr_t)d_src & 255u)) return set_error(CSIC_EINVAL_SIZE, "a planar frame buffer must be 256-byte aligned");
    if (((uintptr_t)d_src & 3u) || ((uintptr_t)d_out & 3u)) return set_error(CSIC_EINVAL_SIZE, "source and output must be 4-byte aligned");
    if ((int64_t)g.W * g.H >= ((int64_t)1 << 31)) return set_error(CSIC_EINVAL_SIZE, "frame too large for csic_decode_view_device");
    ViewPlan vp;                                                        // kind, threads and blocks: csic_select.cpp
    plan_view(g, plan->tune, *view, (uintptr_t)d_out, nframes, &vp);
    const ViewFn fn = view_kernel(vp, src_format, out_format, !plan->tune.no_nt);
    ViewArgs a;
    std::memset(&a, 0, sizeof a);
    fill_dec_args(plan, src_format, &a.d);
    a.view_px = (int64_t)view->width * view->height;
    a.units = vp.units;
    a.x0 = view->x0; a.y0 = view->y0; a.vw = view->width; a.vh = view->height; a.ls = vp.ls;
    a.ncx = vp.ncx; a.ncy = vp.ncy;
    a.whole = view->scale >= g.f && view->x0 % g.f == 0 && view->y0 % g.f == 0;
    a.U = vp.units_per_row; a.T = vp.T;
    magic_div((uint32_t)a.U, &a.mU, &a.kU);
    CSIC_DEVICE_SCOPE(plan->device);
    st = for_frame_batches(nframes, [&](int f0, int nz) {
        a.d.src = static_cast<const uint8_t *>(d_src) + (int64_t)f0 * a.d.src_frame_bytes;
        a.dst = static_cast<uint32_t *>(d_out) + (int64_t)f0 * a.view_px;
        return launch(fn, dim3(vp.grid.x, 1, (unsigned)nz), dim3(vp.block.x, 1, 1), static_cast<hipStream_t>(hip_stream), a);
    });
    if (st != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

int csic_decode_view_host(csic_plan *plan, const void *src, size_t src_bytes, int32_t src_format, const csic_view *view, uint32_t *out,
                          size_t out_px, int32_t out_format, int32_t nframes)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    if (!view) return set_error(CSIC_EINVAL_NULL, "view is NULL");
    if (!src || !out) return set_error(CSIC_EINVAL_NULL, "host buffer is NULL");
    if (nframes <= 0) return set_error(CSIC_EINVAL_SIZE, "nframes must be positive. Got %d", nframes);
    int st = decode_check_formats(src_format, out_format);
    if (st != CSIC_OK) return st;
    st = check_view(plan->g, *view);
    if (st != CSIC_OK) return st;
    const size_t need_src = (size_t)nframes * (size_t)dec_src_frame_bytes(plan, src_format);
    const size_t need_out = (size_t)nframes * (size_t)view->width * (size_t)view->height;
    if (src_bytes != need_src) return set_error(CSIC_EINVAL_SIZE, "expected %zu source bytes (%d frames), got %zu", need_src, nframes, src_bytes);
    if (out_px != need_out) return set_error(CSIC_EINVAL_SIZE, "expected room for %zu output pixels (%d frames), got %zu", need_out, nframes, out_px);
    CSIC_DEVICE_SCOPE(plan->device);
    DeviceStaging dev;
    void *d_src = dev.alloc(need_src), *d_out = dev.alloc(need_out * 4);
    dev.to_device(d_src, src, need_src);
    if (dev.ok()) {
        st = csic_decode_view_device(plan, d_src, src_format, view, d_out, out_format, nframes, nullptr);
        if (st == CSIC_OK) { dev.to_host(out, d_out, need_out * 4); dev.sync(); }
    }
    if (st != CSIC_OK) return st;
    if (!dev.ok()) return set_error(CSIC_EHIP, "csic_decode_view_host: %s", hipGetErrorString(dev.error()));
    clear_error();
    return CSIC_OK;
}

} // extern "C"
