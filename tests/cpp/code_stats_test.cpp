// code_stats_test.cpp -- csic.hpp's code-statistics API (csic_code_stats_*) from C++.
//   cpu : the CodeStats arithmetic on hand-made counts and the refusals that need no device
//   gpu : the same, then ImageCompressorTop::codeStats and Plan::codeStats on a 52 x 19 frame at 4:2:0, 6 / 5 / 5 against counts
//         this test takes itself from the bit-packed frame, sample by sample from the definition in csic.h
// Prints "all checks passed" and exits 0, or names the first failed check and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "csic.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++failures; } } while (0)

static void cpu_checks()
{
    csic::CodeStats s;
    s.pixels = 64;
    s.bits[0] = 4; s.bits[1] = 3; s.bits[2] = 2;
    for (int i = 0; i < 16; ++i) s.hist[0][0][i] = 4;           // Y: uniform over 16 codes, residuals single-valued
    s.hist[1][0][1] = 64;
    s.hist[0][1][0] = 16;                                       // Cb: constant
    s.hist[1][1][0] = 16;
    s.hist[0][2][0] = 12; s.hist[0][2][1] = 4;                  // Cr: 3 : 1, residuals uniform over 4
    for (int i = 0; i < 4; ++i) s.hist[1][2][i] = 4;
    const double hcr = -(0.75 * std::log2(0.75) + 0.25 * std::log2(0.25));
    CHECK(s.samples(0) == 64 && s.samples(1) == 16 && s.samples(2) == 16);
    CHECK(std::fabs(s.entropy(csic::CodeStats::Codes, csic::CodeStats::Y) - 4.0) < 1e-12 && s.entropy(csic::CodeStats::Residuals, 0) == 0.0);
    CHECK(s.entropy(0, csic::CodeStats::Cb) == 0.0 && s.entropy(1, 1) == 0.0);
    CHECK(std::fabs(s.entropy(0, csic::CodeStats::Cr) - hcr) < 1e-12 && std::fabs(s.entropy(1, 2) - 2.0) < 1e-12);
    CHECK(s.rawBitsPerPixel() == 5.25);
    CHECK(std::fabs(s.bitsPerPixel(csic::CodeStats::Codes) - (256.0 + 16.0 * hcr) / 64.0) < 1e-12);
    CHECK(std::fabs(s.bitsPerPixel(csic::CodeStats::Residuals) - 32.0 / 64.0) < 1e-12);
    CHECK(std::fabs(s.bitsPerPixel(csic::CodeStats::Best) - 16.0 * hcr / 64.0) < 1e-12);
    CHECK(s.idealBytes(csic::CodeStats::Best) == 2 && s.idealBytes(csic::CodeStats::Codes) == 34 && s.idealBytes(csic::CodeStats::Residuals) == 4);
    csic::CodeStats t = s;
    CHECK(t == s);
    t.hist[1][2][3] = 5;
    CHECK(!(t == s));
    CHECK(CSIC_STATS_KINDS == 2 && CSIC_STATS_PLANES == 3 && CSIC_STATS_BINS == 256);

    // refusals: judged before the plan is read or a device touched (`standin` is zeroed memory in a plan's place)
    alignas(256) static unsigned char buf[1024];
    static unsigned char standin_bytes[4096];
    csic_plan *standin = reinterpret_cast<csic_plan *>(standin_bytes);
    uint64_t *hist = reinterpret_cast<uint64_t *>(buf + 512);
    int64_t n = 0;
    CHECK(csic_code_stats_device(nullptr, buf, CSIC_FMT_PLANAR, 1, hist, nullptr) == CSIC_EINVAL_NULL);
    CHECK(csic_code_stats_device(standin, nullptr, CSIC_FMT_PLANAR, 1, hist, nullptr) == CSIC_EINVAL_NULL);
    CHECK(csic_code_stats_device(standin, buf, CSIC_FMT_PLANAR, 1, nullptr, nullptr) == CSIC_EINVAL_NULL);
    CHECK(csic_code_stats_host(nullptr, buf, 256, CSIC_FMT_PLANAR_BITS, 1, hist) == CSIC_EINVAL_NULL);
    CHECK(csic_code_stats_device(standin, buf, CSIC_FMT_YCBCR888X, 1, hist, nullptr) == CSIC_EINVAL_FORMAT);
    CHECK(csic_code_stats_host(standin, buf, 256, CSIC_FMT_ARGB8888, 1, hist) == CSIC_EINVAL_FORMAT);
    CHECK(csic_code_stats_device(standin, buf, CSIC_FMT_PLANAR_BITS, 0, hist, nullptr) == CSIC_EINVAL_SIZE);
    CHECK(csic_code_stats_device(standin, buf, CSIC_FMT_PLANAR_BITS, 65536, hist, nullptr) == CSIC_EINVAL_SIZE);
    CHECK(csic_code_stats_device(standin, buf + 64, CSIC_FMT_PLANAR_BITS, 1, hist, nullptr) == CSIC_EINVAL_SIZE);
    CHECK(csic_code_stats_device(standin, buf, CSIC_FMT_PLANAR_BITS, 1, reinterpret_cast<uint64_t *>(buf + 516), nullptr) == CSIC_EINVAL_SIZE);
    CHECK(std::strcmp(csic_code_stats_kernel_name(nullptr, CSIC_FMT_PLANAR), "") == 0);
    CHECK(std::strcmp(csic_code_stats_kernel_name(standin, CSIC_FMT_ARGB8888), "") == 0);
    CHECK(csic_code_stats_block_samples(nullptr, CSIC_FMT_PLANAR, &n) == CSIC_EINVAL_NULL);
    CHECK(csic_code_stats_block_samples(standin, 7, &n) == CSIC_EINVAL_FORMAT);
    CHECK(csic_code_stats_block_samples(standin, CSIC_FMT_PLANAR_BITS, &n) == CSIC_OK && n > 0 && n % 2048 == 0);
}

// code i of a bit plane: the q bits at [i q, i q + q), LSB first
static unsigned code_at(const unsigned char *plane, size_t i, int q)
{
    unsigned c = 0;
    for (int b = 0; b < q; ++b) {
        const size_t bit = i * (size_t)q + (size_t)b;
        c |= (unsigned)((plane[bit >> 3] >> (bit & 7)) & 1u) << b;
    }
    return c;
}

static void gpu_checks()
{
    using csic::ProcessingStep;
    const int W = 52, H = 19;
    csic::ImageCompressorTop top(W, H, 2, 0, 6, 5, 5, 1, ProcessingStep::ChromaSubsampling, ProcessingStep::SpatialSampling,
                                 ProcessingStep::ColorQuantization);
    // smooth ramps with a little hash noise: neighbouring samples are close but not equal
    std::vector<uint32_t> argb((size_t)W * H);
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            const uint32_t nz = ((uint32_t)(r * W + c) * 2654435761u) >> 29;
            argb[(size_t)r * W + c] = 0xFF000000u | (uint32_t)((r * 9 + c * 3 + nz) & 255) << 16 | (uint32_t)((r * 5 + c * 4) & 255) << 8
                                      | (uint32_t)((r * 2 + c * 4 + nz) & 255);
        }
    const csic::PlanarBitsFrame fr = top.processPlanarBits(argb);
    const csic_planar_bits_layout &L = fr.layout;
    csic::CodeStats want;
    const int64_t off[3] = {L.y_offset, L.cb_offset, L.cr_offset};
    const int64_t ns[3] = {(int64_t)L.geometry.y_width * L.geometry.y_height, L.geometry.chroma_samples, L.geometry.chroma_samples};
    const int q[3] = {L.y_bits, L.cb_bits, L.cr_bits};
    for (int p = 0; p < 3; ++p) {
        unsigned prev = 0;
        for (int64_t i = 0; i < ns[p]; ++i) {
            const unsigned c = code_at(fr.bytes.data() + off[p], (size_t)i, q[p]);
            ++want.hist[0][p][c];
            ++want.hist[1][p][(c - prev) & ((1u << q[p]) - 1u)];
            prev = c;
        }
        want.bits[p] = q[p];
    }
    want.pixels = (int64_t)W * H;
    CHECK(ns[0] == 52 * 19 && ns[1] == 26 * 10);
    const csic::CodeStats got = top.codeStats(argb);
    CHECK(got == want);
    CHECK(got.samples(0) == (uint64_t)ns[0] && got.samples(1) == (uint64_t)ns[1] && got.samples(2) == (uint64_t)ns[2]);
    CHECK(got.entropy(csic::CodeStats::Residuals, csic::CodeStats::Y) < got.entropy(csic::CodeStats::Codes, csic::CodeStats::Y));
    CHECK(got.bitsPerPixel(csic::CodeStats::Best) < got.rawBitsPerPixel());
    CHECK(std::strcmp(top.codeStatsKernelName(), "k_cstat_bits<q6,5,5,nt>") == 0);
    CHECK(std::strcmp(top.codeStatsKernelName(csic::PixelFormat::PLANAR), "k_cstat_bytes<nt>") == 0);
    // a plan of its own from the parameters, as for a container's frames: two copies of the frame as a batch
    csic::Plan plan(top.params());
    std::vector<unsigned char> two(fr.bytes);
    two.insert(two.end(), fr.bytes.begin(), fr.bytes.end());
    const std::vector<csic::CodeStats> both = plan.codeStats(two.data(), two.size(), csic::PixelFormat::PLANAR_BITS, 2);
    CHECK(both.size() == 2 && both[0] == want && both[1] == want);
    CHECK(plan.codeStatsBlockSamples() > 0);
    bool threw = false;
    try { plan.codeStats(two.data(), two.size() - 1, csic::PixelFormat::PLANAR_BITS, 2); }
    catch (const csic::IllegalArgumentException &e) { threw = e.status == CSIC_EINVAL_SIZE; }
    CHECK(threw);
    threw = false;
    try { plan.codeStats(two.data(), two.size(), csic::PixelFormat::YCBCR888X, 2); }
    catch (const csic::IllegalArgumentException &e) { threw = e.status == CSIC_EINVAL_FORMAT; }
    CHECK(threw);
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::printf("usage: code_stats_test cpu|gpu\n"); return 2; }
    const bool gpu = std::strcmp(argv[1], "gpu") == 0;
    try {
        cpu_checks();
        if (gpu) gpu_checks();
    } catch (const std::exception &e) { std::printf("FAILED: exception %s\n", e.what()); ++failures; }
    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
