// distortion_test.cpp -- csic.hpp's distortion API (csic_distortion_*) from C++.
//   cpu : the Distortion helpers and the refusals that need no device
//   gpu : ImageCompressorTop::distortion on the hand-worked 4x2 frame of tests/test_distortion_host.py (precomputed sums), as one
//         frame and as a batch of two
// Prints "all checks passed" and exits 0, or names the first failed check and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "csic.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++failures; } } while (0)

static bool near(double a, double b) { return std::fabs(a - b) < 1e-9; }

static void cpu_checks()
{
    csic::Distortion d;
    d.pixels = 100;
    CHECK(std::isinf(d.psnr(csic::Distortion::R)) && std::isinf(d.psnrRgb()) && d.mse(csic::Distortion::Y) == 0.0);
    const uint64_t s[6] = {65025, 65025, 65025, 6502500, 650, 0};
    std::memcpy(d.sse, s, sizeof s);
    CHECK(near(d.mse(csic::Distortion::R), 650.25));
    CHECK(near(d.psnr(csic::Distortion::R), 20.0) && near(d.psnrRgb(), 20.0) && near(d.psnr(csic::Distortion::Y), 0.0));
    CHECK(std::isinf(d.psnr(csic::Distortion::Cr)));
    size_t b = 0;
    uint64_t sse[6];
    uint32_t px[8] = {0};
    CHECK(csic_distortion_workspace_bytes(nullptr, 1, &b) == CSIC_EINVAL_NULL);
    CHECK(csic_distortion_device(nullptr, px, 1, sse, px, sizeof px, nullptr) == CSIC_EINVAL_NULL);
    CHECK(csic_distortion_host(nullptr, px, 8, 1, sse) == CSIC_EINVAL_NULL);
    CHECK(std::strcmp(csic_distortion_kernel_name(nullptr), "") == 0);
}

static uint32_t gray(uint32_t v) { return 0xFF000000u | v * 0x010101u; }

static void gpu_checks()
{
    using csic::ProcessingStep;
    csic::ImageCompressorTop top(4, 2, 4, 4, 8, 8, 8, 2, ProcessingStep::ChromaSubsampling, ProcessingStep::SpatialSampling,
                                 ProcessingStep::ColorQuantization);
    const std::vector<uint32_t> frame = {gray(0), 0xFFFF0000u, gray(20), gray(30), gray(40), gray(50), gray(60), gray(70)};
    const uint64_t want[6] = {72761, 7736, 7736, 14229, 1849, 16129};
    std::vector<csic::Distortion> d = top.distortion(frame.data(), 1);
    CHECK(d.size() == 1);
    for (int c = 0; c < 6; ++c) CHECK(d[0].sse[c] == want[c]);
    CHECK(d[0].pixels == 8);
    CHECK(near(d[0].psnrRgb(), 10.0 * std::log10(65025.0 * 3 * 8 / (72761.0 + 7736 + 7736))));
    std::vector<uint32_t> two(frame);
    two.insert(two.end(), frame.begin(), frame.end());
    d = top.distortion(two.data(), 2);
    CHECK(d.size() == 2);
    for (int c = 0; c < 6; ++c) CHECK(d[0].sse[c] == want[c] && d[1].sse[c] == want[c]);
    CHECK(top.distortionWorkspaceBytes(2) >= 2 * 48);
    bool threw = false;
    try { top.distortion(frame.data(), 65536); } catch (const csic::IllegalArgumentException &e) { threw = e.status == CSIC_EINVAL_SIZE; }
    CHECK(threw);
}

int main(int argc, char **argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    cpu_checks();
    if (gpu) {
        try { gpu_checks(); } catch (const std::exception &e) { std::printf("FAILED: exception %s\n", e.what()); ++failures; }
    }
    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
