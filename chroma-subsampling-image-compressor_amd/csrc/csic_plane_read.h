// csic_plane_read.h -- the one reader of the planar frame formats (include/csic.h: csic_planar_layout, csic_planar_bits_layout), shared
// by csic_planar.hip (k_recon), csic_planar_bits.hip (k_rbits) and csic_decode.hip (k_decode, k_decode_gen): where a stream position
// comes from in the input image, which chroma sample it takes -- with the "replay the last sample of the row above" rule --, the 32-bit
// window of a bit plane and the code in it, one position read by the definition, and the reconstruct kernels' body.  Device code only.
//
// Functions that read the layout are templates over the kernel's argument struct E (PExtra, BExtra, DecArgs), which supplies
// Wm, Wc, lhe, lve, replay_last, mWm, kWm and, for the bit planes, off[], nbytes[], q[].  What differs between the formats is a PLANE
// SOURCE Src: a small struct, built as Src{e, fb} from the argument struct and the frame's base, that says how samples are fetched
// and picked apart:
//   typedef ... idx;                                     the integer type its chroma sample indices are computed in
//   template <bool NT> uint32_t y_word(uint32_t j0)      the word that starts at the Y sample of position j0
//   uint32_t c_word(int p, idx k0)                       the word that starts at sample k0 of plane p (1 = Cb, 2 = Cr)
//   uint32_t y_at(uint32_t w, uint32_t i), c_at(int p, uint32_t w, uint32_t i)     sample i of a word, as an 8-bit value
//   uint32_t y_one(uint32_t j), c_one(int p, idx k)      one sample on its own
// BytePlanes (csic_planar.hip) reads PLANAR, BitPlanes (below) PLANAR_BITS and -- at 8 bits -- PLANAR for the decode kernels.
//
// The shapes below are the ones under which hipcc emits, instruction for instruction, what the per-unit copies compiled to (compare
// `make asm` before and after a change here): the argument struct is passed next to the source, not through it; recon_body and
// recon_slow each build their own source, which is where the bit widths are read; the fast path states its chroma index in place
// instead of calling chroma_index; and the sample words are read inside each branch of the second loop.
#pragma once
#include "csic_kernel_ops.h"

namespace csic {

// input offset of output stream position j: decimated (ro, co) = (j / Wo, j % Wo) -> image (ro * f, co * f)
__device__ __forceinline__ int64_t stream_in_off(const KArgs &a, uint32_t j)
{
    const uint32_t ro = (uint32_t)(((uint64_t)j * a.mWo) >> a.kWo);
    const uint32_t co = j - ro * (uint32_t)a.Wo;
    return (int64_t)(ro * (uint32_t)a.f) * a.ip + co * (uint32_t)a.f;
}

// chroma sample index of stream position (r, c), computed in I -- csic.h, csic_planar_layout
template <class I, class E> __device__ __forceinline__ I chroma_index(const E &e, uint32_t r, uint32_t c)
{
    if ((r & ((1u << e.lve) - 1u)) == 0 || !e.replay_last) return (I)(r >> e.lve) * e.Wc + (c >> e.lhe);
    return (I)((r - 1u) >> e.lve) * e.Wc + (e.Wc - 1);              // ChromaSubsampler.scala:52-65: the last sample of the row above
}

// bits [bit, bit + 32) of plane p (bit < 8 * nbytes[p]) of the frame of `lim` bytes at fb: the dword that holds `bit` and the next
// one, clamped to the plane's last dword (planes are padded to 256 bytes, so that dword is inside the frame; the bits it cannot
// supply are past the plane's end)
template <class E> __device__ __forceinline__ uint32_t plane_window(const E &e, int64_t lim, gcbyte_t fb, int p, uint64_t bit)
{
    const int64_t dw = (int64_t)(bit >> 5), last = (e.nbytes[p] + 3) / 4 - 1;
    const uint32_t lo = by_ld4<false>(lim, fb, e.off[p] + 4 * dw);
    const uint32_t hi = by_ld4<false>(lim, fb, e.off[p] + 4 * min(dw + 1, last));
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (bit & 31u));
}
// code i of a window of q-bit codes, left-aligned to 8 bits (the sample value it stands for)
__device__ __forceinline__ uint32_t code_at(uint32_t win, uint32_t i, uint32_t q) { return ((win >> (i * q)) & ((1u << q) - 1u)) << (8u - q); }

// bit planes of a frame of `lim` bytes; Q8: every plane holds 8-bit codes (a PLANAR frame read as bit planes)
template <class E, int64_t E::*LIM, bool Q8 = false> struct BitPlanes {
    typedef uint64_t idx;
    const E &e;
    const gcbyte_t fb;
    const int64_t lim;
    const uint32_t qy, qb, qr;
    __device__ __forceinline__ BitPlanes(const E &e_, gcbyte_t fb_)
        : e(e_), fb(fb_), lim(e_.*LIM), qy(Q8 ? 8u : (uint32_t)e_.q[0]), qb(Q8 ? 8u : (uint32_t)e_.q[1]), qr(Q8 ? 8u : (uint32_t)e_.q[2]) {}
    __device__ __forceinline__ uint32_t q(int p) const { return p == 0 ? qy : p == 1 ? qb : qr; }
    template <bool NT> __device__ __forceinline__ uint32_t y_word(uint32_t j0) const { return plane_window(e, lim, fb, 0, (uint64_t)j0 * q(0)); }
    __device__ __forceinline__ uint32_t c_word(int p, idx k0) const { return plane_window(e, lim, fb, p, k0 * q(p)); }
    __device__ __forceinline__ uint32_t y_at(uint32_t w, uint32_t i) const { return code_at(w, i, q(0)); }
    __device__ __forceinline__ uint32_t c_at(int p, uint32_t w, uint32_t i) const { return code_at(w, i, q(p)); }
    __device__ __forceinline__ uint32_t y_one(uint32_t j) const { return y_at(y_word<false>(j), 0); }
    __device__ __forceinline__ uint32_t c_one(int p, idx k) const { return c_at(p, c_word(p, k), 0); }
};

// stream position j by the definition: the packed pixel in FMT
template <int FMT, class E, class Src> __device__ __forceinline__ uint32_t plane_pixel(const E &e, const Src &s, uint32_t j)
{
    const uint32_t r = (uint32_t)(((uint64_t)j * e.mWm) >> e.kWm), c = j - r * (uint32_t)e.Wm;
    const typename Src::idx k = chroma_index<typename Src::idx>(e, r, c);
    return finish_y<FMT>(s.y_one(j), chroma_term_q<FMT>(s.c_one(1, k), s.c_one(2, k)));
}

// ------------------------------------------------------------------------------------------------
// the reconstruct kernels' body: planes -> packed, n pixels per frame at `out`
// ------------------------------------------------------------------------------------------------
// one group of (up to) 4 positions, position by position: the stream's ragged tail, and groups that may straddle chroma rows
template <int FMT, bool NT, class Src, class E>
__device__ __forceinline__ void recon_slow(const E &e, gcbyte_t fb, gout_t out, uint32_t j0, uint32_t n)
{
    uint32_t o[4];
    const uint32_t cnt = min(4u, n - j0);
    const Src s{e, fb};
    for (uint32_t q = 0; q < cnt; ++q) o[q] = plane_pixel<FMT>(e, s, j0 + q);
    if (cnt == 4u) { const u32x4 ov = {o[0], o[1], o[2], o[3]}; px_st4<NT>(e.n, out, (int64_t)j0, ov); }
    else for (uint32_t q = 0; q < cnt; ++q) px_st1<false>(e.n, out, (int64_t)(j0 + q), o[q]);
}

// K groups per lane spaced by the block size: all their loads (the Y word and the chroma words of each) are in flight before the
// first inverse transform starts.  The first version took one group per lane -- 8 bytes in flight per lane -- and ran at 58 % of
// the roofline on a kernel that is three quarters stores.
template <int FMT, bool FAST, bool NT, bool CHECK, int K, class Src, class E>
__device__ __forceinline__ void recon_body(const E &e, gcbyte_t fb, gout_t out, uint32_t g0, uint32_t T, uint32_t ngroups)
{
    const Src s{e, fb};
    const uint32_t n = (uint32_t)e.n;
    uint32_t yw[K], bw[K], rw[K], sh[K];
    bool live[K], fast[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t g = g0 + (uint32_t)k * T;
        live[k] = !CHECK || g < ngroups;
        const uint32_t j0 = 4u * (CHECK ? min(g, ngroups - 1u) : g);
        fast[k] = FAST && (!CHECK || j0 + 3u < n);
        yw[k] = bw[k] = rw[k] = sh[k] = 0;
        if (fast[k]) {
            // module_width % 4 == 0: the group lies in one chroma row at a column that is a multiple of 4, so its samples are 4, 2 or 1
            // consecutive ones (h = 1, 2, 4) -- or ONE on a row that replays the last sample of the row above.  Branch-free: the words
            // that start at the group's first samples are loaded, position q then takes sample q >> sh.  With a branch per case the K
            // groups' loads did not stay in flight together.
            yw[k] = s.template y_word<NT>(j0);
            const uint32_t r = (uint32_t)(((uint64_t)j0 * e.mWm) >> e.kWm), c0 = j0 - r * (uint32_t)e.Wm;
            const bool replay = (r & ((1u << e.lve) - 1u)) != 0 && e.replay_last;
            typedef typename Src::idx idx;
            const idx k0 = replay ? (idx)((r - 1u) >> e.lve) * e.Wc + (e.Wc - 1) : (idx)(r >> e.lve) * e.Wc + (c0 >> e.lhe);
            sh[k] = replay ? 2u : (uint32_t)e.lhe;
            bw[k] = s.c_word(1, k0);
            rw[k] = s.c_word(2, k0);
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (!live[k]) continue;
        const uint32_t j0 = 4u * (g0 + (uint32_t)k * T);
        if (!fast[k]) { recon_slow<FMT, NT, Src>(e, fb, out, j0, n); continue; }
        // the chroma half of the inverse transform once per DISTINCT sample of the group (4, 2 or 1), not once per pixel: the kernel
        // is as much VALU as memory (27 VALU per pixel on 5.5 bytes with a term per pixel; 69 % of the roofline)
        uint32_t o[4];
        const uint32_t y0 = s.y_at(yw[k], 0), y1 = s.y_at(yw[k], 1), y2 = s.y_at(yw[k], 2), y3 = s.y_at(yw[k], 3);
        if (sh[k] == 2u) {
            const ChromaTerm t = chroma_term_q<FMT>(s.c_at(1, bw[k], 0), s.c_at(2, rw[k], 0));
            o[0] = finish_y<FMT>(y0, t); o[1] = finish_y<FMT>(y1, t); o[2] = finish_y<FMT>(y2, t); o[3] = finish_y<FMT>(y3, t);
        } else if (sh[k] == 1u) {
            const ChromaTerm t0 = chroma_term_q<FMT>(s.c_at(1, bw[k], 0), s.c_at(2, rw[k], 0));
            const ChromaTerm t1 = chroma_term_q<FMT>(s.c_at(1, bw[k], 1), s.c_at(2, rw[k], 1));
            o[0] = finish_y<FMT>(y0, t0); o[1] = finish_y<FMT>(y1, t0); o[2] = finish_y<FMT>(y2, t1); o[3] = finish_y<FMT>(y3, t1);
        } else {
            o[0] = finish_y<FMT>(y0, chroma_term_q<FMT>(s.c_at(1, bw[k], 0), s.c_at(2, rw[k], 0)));
            o[1] = finish_y<FMT>(y1, chroma_term_q<FMT>(s.c_at(1, bw[k], 1), s.c_at(2, rw[k], 1)));
            o[2] = finish_y<FMT>(y2, chroma_term_q<FMT>(s.c_at(1, bw[k], 2), s.c_at(2, rw[k], 2)));
            o[3] = finish_y<FMT>(y3, chroma_term_q<FMT>(s.c_at(1, bw[k], 3), s.c_at(2, rw[k], 3)));
        }
        const u32x4 ov = {o[0], o[1], o[2], o[3]};
        px_st4<NT>(e.n, out, (int64_t)j0, ov);
    }
    if (!CHECK) keep_tail_apart();
}

} // namespace csic
