// csic_qsweep_host.cpp -- csic_qsweep_rank: the candidates of a quantiser sweep in rank order (definition in include/csic.h).  Host
// arithmetic on the 24 sums and 24 histograms csic_qsweep_* return: no HIP, no device.
#include <algorithm>
#include <cmath>
#include <tuple>

#include "csic_internal.h"

namespace csic {

// zero-order entropy of 256 counts with total N, in bits per sample: 0 for an empty or single-valued histogram
static double qs_entropy(const uint64_t *h, uint64_t N)
{
    if (N == 0) return 0.0;
    double H = 0.0;
    for (int i = 0; i < CSIC_STATS_BINS; ++i)
        if (h[i]) {
            const double p = (double)h[i] / (double)N;
            H -= p * std::log2(p);
        }
    return H > 0.0 ? H : 0.0;
}

} // namespace csic

using namespace csic;

extern "C" int csic_qsweep_rank(const csic_params *p, const csic_qsweep_result *r, int32_t nframes, int32_t coding, const uint8_t weights[3],
                                const uint8_t max_bits[3], csic_qsweep_candidate *out, int32_t *n)
{
    if (!p || !r || !out || !n) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    if (nframes < 1 || nframes > 65535) return set_error(CSIC_EINVAL_SIZE, "nframes must be in 1..65535. Got %d", nframes);
    if (coding != CSIC_CODING_RAW && coding != CSIC_CODING_GROUPS && coding != CSIC_CODING_RICE && coding != CSIC_CODING_RANS)
        return set_error(CSIC_EINVAL_FORMAT, "coding must be raw(0), groups(1), rice(3) or rans(5). Got %d", coding);
    if (p->in_format != CSIC_FMT_ARGB8888)
        return set_error(CSIC_EINVAL_FORMAT, "csic_qsweep reads ARGB8888(0) input. Got %d", p->in_format);
    uint64_t w[3] = {1, 1, 1};
    int mb[3] = {8, 8, 8};
    for (int c = 0; c < 3; ++c) {
        if (weights) w[c] = weights[c];
        if (max_bits) mb[c] = max_bits[c];
        if (w[c] < 1) return set_error(CSIC_EINVAL_SIZE, "weights must be in 1..255. Got %d", (int)w[c]);
        if (mb[c] < 1 || mb[c] > 8) return set_error(CSIC_EINVAL_BITS, "max_bits must be in 1..8. Got %d", mb[c]);
    }
    csic_params pp = *p;
    pp.y_bits = pp.cb_bits = pp.cr_bits = 8;
    csic_planar_bits_layout B;
    int st = csic_planar_bits_layout_of(&pp, &B);
    if (st != CSIC_OK) return st;
    if ((int64_t)p->width * p->height > ((int64_t)1 << 30))
        return set_error(CSIC_EINVAL_SIZE, "csic_qsweep_rank takes frames of at most 2^30 pixels");
    const int count = mb[0] * mb[1] * mb[2];
    if (*n < count) return set_error(CSIC_EINVAL_SIZE, "out holds %d candidates, %d are listed", *n, count);

    // the frames' sums: weighted distortion per plane and width, coded bytes per plane and width
    uint64_t D[3][8], bytes[3][8];
    for (int c = 0; c < 3; ++c)
        for (int q = 1; q <= mb[c]; ++q) {
            uint64_t sse = 0, h[CSIC_STATS_BINS] = {}, N = 0;
            bool over = false;
            for (int f = 0; f < nframes; ++f) {
                over |= __builtin_add_overflow(sse, r[f].sse[c][q - 1], &sse);
                for (int i = 0; i < CSIC_STATS_BINS; ++i) {
                    over |= __builtin_add_overflow(h[i], r[f].hist[c][q - 1][i], &h[i]);
                    over |= __builtin_add_overflow(N, r[f].hist[c][q - 1][i], &N);
                }
            }
            over |= __builtin_mul_overflow(sse, w[c], &D[c][q - 1]);
            if (over || N > ((uint64_t)1 << 56)) return set_error(CSIC_EINVAL_SIZE, "the sums of plane %d at width %d leave 64 bits", c, q);
            const double raw = (double)N * q, coded = (double)N * qs_entropy(h, N);
            bytes[c][q - 1] = (uint64_t)std::ceil((coded < raw ? coded : raw) / 8.0);
        }
    int k = 0;
    for (int y = 1; y <= mb[0]; ++y)
        for (int cb = 1; cb <= mb[1]; ++cb)
            for (int cr = 1; cr <= mb[2]; ++cr) {
                csic_qsweep_candidate &c = out[k++];
                c.y_bits = y; c.cb_bits = cb; c.cr_bits = cr; c.reserved = 0;
                uint64_t d = D[0][y - 1];
                if (__builtin_add_overflow(d, D[1][cb - 1], &d) || __builtin_add_overflow(d, D[2][cr - 1], &d))
                    return set_error(CSIC_EINVAL_SIZE, "the distortion of %d/%d/%d leaves 64 bits", y, cb, cr);
                c.distortion = d;
                if (coding == CSIC_CODING_RAW) {
                    pp.y_bits = y; pp.cb_bits = cb; pp.cr_bits = cr;
                    st = csic_planar_bits_layout_of(&pp, &B);
                    if (st != CSIC_OK) return st;
                    c.est_bytes = 80u + (uint64_t)nframes * (uint64_t)B.payload_bytes;
                } else {
                    c.est_bytes = 80u + bytes[0][y - 1] + bytes[1][cb - 1] + bytes[2][cr - 1];
                }
            }
    std::sort(out, out + count, [](const csic_qsweep_candidate &a, const csic_qsweep_candidate &b) {
        return std::make_tuple(a.distortion, a.est_bytes, a.y_bits, a.cb_bits, a.cr_bits) <
               std::make_tuple(b.distortion, b.est_bytes, b.y_bits, b.cb_bits, b.cr_bits);
    });
    *n = count;
    clear_error();
    return CSIC_OK;
}
