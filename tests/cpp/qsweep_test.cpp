// qsweep_test.cpp -- csic.hpp's quantiser-sweep API (csic_qsweep_*) from C++.
//   cpu : csic::qsweepRank on a hand-made table against csic_qsweep_rank and against sizes worked by hand, and the refusals that need
//         no device
//   gpu : the same, then ImageCompressorTop::qsweep on a 52 x 20 frame at 4:2:0 against ImageCompressorTop::distortion of the same
//         frame width by width, the totals of its histograms, and its ranking through both entry points
// Prints "all checks passed" and exits 0, or names the first failed check and exits 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "csic.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++failures; } } while (0)

static csic_params params(int w, int h)
{
    csic_params p;
    csic::check(csic_params_default(&p, w, h));
    p.chroma_a = 2; p.chroma_b = 0; p.factor = 1;
    p.op[0] = CSIC_OP_CHROMA; p.op[1] = CSIC_OP_SPATIAL; p.op[2] = CSIC_OP_QUANT;
    return p;
}

static bool same(const std::vector<csic_qsweep_candidate> &a, const csic_qsweep_candidate *b, int n)
{
    if ((int)a.size() != n) return false;
    for (int i = 0; i < n; ++i)
        if (a[i].distortion != b[i].distortion || a[i].est_bytes != b[i].est_bytes || a[i].y_bits != b[i].y_bits ||
            a[i].cb_bits != b[i].cb_bits || a[i].cr_bits != b[i].cr_bits || a[i].reserved != 0) return false;
    return true;
}

static void cpu_checks()
{
    const csic_params p = params(16, 16);
    std::vector<csic_qsweep_result> r(1);
    std::memset(r.data(), 0, sizeof r[0]);
    for (int c = 0; c < 3; ++c)
        for (int q = 0; q < 8; ++q) {
            r[0].sse[c][q] = (uint64_t)(1000 >> q) * (uint64_t)(c + 1);
            r[0].hist[c][q][0] = c == 0 ? 256 : 64;                  // single-valued: no bytes
        }
    for (int i = 0; i < 256; ++i) r[0].hist[0][7][i] = 1;           // Y at 8 bits: flat, 256 bytes
    const std::vector<csic_qsweep_candidate> ranked = csic::qsweepRank(p, r);
    CHECK(ranked.size() == 512);
    CHECK(ranked[0].y_bits == 8 && ranked[0].cb_bits == 8 && ranked[0].cr_bits == 8 && ranked[0].distortion == 7 + 14 + 21 && ranked[0].est_bytes == 80 + 256);
    CHECK(ranked[511].y_bits == 1 && ranked[511].cb_bits == 1 && ranked[511].cr_bits == 1 && ranked[511].distortion == 6000 && ranked[511].est_bytes == 80);
    for (size_t i = 1; i < ranked.size(); ++i) CHECK(ranked[i - 1].distortion <= ranked[i].distortion);
    csic_qsweep_candidate out[CSIC_QSWEEP_MAX_CANDIDATES];
    int32_t n = CSIC_QSWEEP_MAX_CANDIDATES;
    CHECK(csic_qsweep_rank(&p, r.data(), 1, CSIC_CODING_RANS, nullptr, nullptr, out, &n) == CSIC_OK && same(ranked, out, n));
    const uint8_t w[3] = {4, 1, 1}, mb[3] = {6, 5, 5};
    const std::vector<csic_qsweep_candidate> raw = csic::qsweepRank(p, r, CSIC_CODING_RAW, w, mb);
    n = CSIC_QSWEEP_MAX_CANDIDATES;
    CHECK(csic_qsweep_rank(&p, r.data(), 1, CSIC_CODING_RAW, w, mb, out, &n) == CSIC_OK && n == 150 && same(raw, out, n));
    CHECK(raw[0].y_bits == 6 && raw[0].cb_bits == 5 && raw[0].cr_bits == 5 && raw[0].distortion == 4 * 31 + 2 * 62 + 3 * 62);
    CHECK(raw[0].est_bytes == 80 + 256 * 6 / 8 + 2 * (64 * 5 / 8));                         // 4:2:0: 64 chroma samples per plane
    // refusals
    const uint8_t w0[3] = {1, 0, 1}, mb9[3] = {8, 9, 8};
    n = CSIC_QSWEEP_MAX_CANDIDATES;
    CHECK(csic_qsweep_rank(&p, r.data(), 1, CSIC_CODING_RANS, w0, nullptr, out, &n) == CSIC_EINVAL_SIZE);
    CHECK(csic_qsweep_rank(&p, r.data(), 1, CSIC_CODING_RANS, nullptr, mb9, out, &n) == CSIC_EINVAL_BITS);
    CHECK(csic_qsweep_rank(&p, r.data(), 1, 2, nullptr, nullptr, out, &n) == CSIC_EINVAL_FORMAT);
    CHECK(csic_qsweep_rank(nullptr, r.data(), 1, CSIC_CODING_RANS, nullptr, nullptr, out, &n) == CSIC_EINVAL_NULL);
    n = 100;
    CHECK(csic_qsweep_rank(&p, r.data(), 1, CSIC_CODING_RANS, nullptr, nullptr, out, &n) == CSIC_EINVAL_SIZE);
    csic_params ycc = p;
    ycc.in_format = CSIC_FMT_YCBCR888X;
    bool threw = false;
    try { csic::qsweepRank(ycc, r); } catch (const std::exception &) { threw = true; }
    CHECK(threw);
    alignas(256) static unsigned char buf[2048];
    static unsigned char standin_bytes[4096];
    csic_plan *standin = reinterpret_cast<csic_plan *>(standin_bytes);
    csic_qsweep_result *res = reinterpret_cast<csic_qsweep_result *>(buf + 512);
    CHECK(csic_qsweep_device(nullptr, buf, 1, res, buf + 1024, 1024, nullptr) == CSIC_EINVAL_NULL);
    CHECK(csic_qsweep_device(standin, buf, 0, res, buf + 1024, 1024, nullptr) == CSIC_EINVAL_SIZE);
    CHECK(csic_qsweep_device(standin, buf, 1, res, buf + 1024 + 8, 1024, nullptr) == CSIC_EINVAL_SIZE);
    CHECK(csic_qsweep_hist_device(standin, buf + 64, 1, res, nullptr) == CSIC_EINVAL_SIZE);
    CHECK(csic_qsweep_host(standin, nullptr, 256, 1, res) == CSIC_EINVAL_NULL);
    CHECK(std::strcmp(csic_qsweep_kernel_name(nullptr), "") == 0);
    CHECK(sizeof(csic_qsweep_result) == 8 * (24 + 24 * 256) && sizeof(csic_qsweep_candidate) == 32 && CSIC_QSWEEP_MAX_TRIES == 4);
}

static void gpu_checks()
{
    const int W = 52, H = 20;
    std::vector<uint32_t> frame((size_t)W * H);
    uint32_t x = 12345u;
    for (auto &px : frame) { x = x * 1664525u + 1013904223u; px = 0xFF000000u | (x >> 8); }
    using PS = csic::ProcessingStep;
    csic::ImageCompressorTop top(W, H, 2, 0, 6, 5, 5, 1, PS::ChromaSubsampling, PS::SpatialSampling, PS::ColorQuantization);
    const std::vector<csic_qsweep_result> r = top.qsweep(frame.data());
    CHECK(r.size() == 1 && std::strcmp(top.qsweepKernelName(), "k_qsweep_sse_fast<f1>") == 0 && top.qsweepWorkspaceBytes(2) > top.qsweepWorkspaceBytes(1));
    for (int q = 1; q <= 8; ++q) {
        csic::ImageCompressorTop tq(W, H, 2, 0, q, q, q, 1, PS::ChromaSubsampling, PS::SpatialSampling, PS::ColorQuantization);
        const csic::Distortion d = tq.distortion(frame.data())[0];
        for (int c = 0; c < 3; ++c) {
            CHECK(r[0].sse[c][q - 1] == d.sse[3 + c]);
            uint64_t total = 0;
            for (int i = 0; i < 256; ++i) { total += r[0].hist[c][q - 1][i]; if (i >= (1 << q)) CHECK(r[0].hist[c][q - 1][i] == 0); }
            CHECK(total == (uint64_t)(c == 0 ? W * H : W * H / 4));
        }
    }
    csic_params p = params(W, H);
    const std::vector<csic_qsweep_candidate> ranked = csic::qsweepRank(p, r);
    csic_qsweep_candidate out[CSIC_QSWEEP_MAX_CANDIDATES];
    int32_t n = CSIC_QSWEEP_MAX_CANDIDATES;
    CHECK(csic_qsweep_rank(&p, r.data(), 1, CSIC_CODING_RANS, nullptr, nullptr, out, &n) == CSIC_OK && same(ranked, out, n) && n == 512);
    const std::vector<csic_qsweep_result> two = top.qsweep(frame.data());                    // exact sums: the same again
    CHECK(std::memcmp(&two[0], &r[0], sizeof r[0]) == 0);
}

int main(int argc, char **argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    try {
        cpu_checks();
        if (gpu) gpu_checks();
    } catch (const std::exception &e) {
        std::printf("FAILED: exception: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
