// ssim_test.cpp -- csic.hpp's structural-similarity API (csic_ssim_*) from C++.
//   cpu : the Ssim helpers and the refusals that need no device
//   gpu : the same, then ImageCompressorTop::ssim on a 24 x 16 frame at 4:2:0, 6 / 5 / 5, factor 2 against the sums and the map that
//         the numpy statement of tests/test_ssim_host.py gives on the oracle's outputs (precomputed), as one frame and as a batch
// Prints "all checks passed" and exits 0, or names the first failed check and exits 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "csic.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++failures; } } while (0)

static void cpu_checks()
{
    csic::Ssim s;
    s.windows = 10;
    s.sums[csic::Ssim::R] = 10 * CSIC_SSIM_ONE; s.sums[csic::Ssim::G] = 5 * CSIC_SSIM_ONE; s.sums[csic::Ssim::B] = 0;
    s.sums[csic::Ssim::Y] = -10 * CSIC_SSIM_ONE;
    CHECK(s.mean(csic::Ssim::R) == 1.0 && s.mean(csic::Ssim::G) == 0.5 && s.mean(csic::Ssim::B) == 0.0 && s.mean(csic::Ssim::Y) == -1.0);
    CHECK(s.meanRgb() == 0.5);
    CHECK(CSIC_SSIM_WINDOW == 8 && CSIC_SSIM_ONE == 65536);
    size_t b = 0;
    uint32_t px[16] = {0};
    int64_t sums[6];
    CHECK(csic_ssim_workspace_bytes(nullptr, 1, &b) == CSIC_EINVAL_NULL);
    CHECK(csic_ssim_device(nullptr, px, 1, sums, nullptr, px, sizeof px, nullptr) == CSIC_EINVAL_NULL);
    CHECK(csic_ssim_host(nullptr, px, 16, 1, sums, nullptr) == CSIC_EINVAL_NULL);
    CHECK(std::strcmp(csic_ssim_kernel_name(nullptr), "") == 0);
}

static void gpu_checks()
{
    using csic::ProcessingStep;
    const int W = 24, H = 16;
    csic::ImageCompressorTop top(W, H, 2, 0, 6, 5, 5, 2, ProcessingStep::ChromaSubsampling, ProcessingStep::SpatialSampling,
                                 ProcessingStep::ColorQuantization);
    // frame 0: multiplicative-hash noise; frame 1: smooth ramps
    std::vector<uint32_t> two((size_t)2 * W * H);
    for (size_t i = 0; i < (size_t)W * H; ++i) two[i] = 0xFF000000u | ((uint32_t)(i * 2654435761u) >> 8);
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c)
            two[(size_t)W * H + (size_t)r * W + c] = 0xFF000000u | (uint32_t)((r * 9 + c * 3) & 255) << 16 | (uint32_t)((r * 5 + c * 7) & 255) << 8
                                                     | (uint32_t)((r * 2 + c * 4) & 255);
    // want0 / map0 and want1: `sums, map = oracle_ssim(oracle, frame, 24, 16, 2, 0, (6, 5, 5), 2)` of tests/test_ssim_host.py on each of
    // the two frames above as a flat uint32 array (`oracle` = conftest's fixture); map0 is `map.reshape(-1)`, [channel][wy][wx]
    const int64_t want0[6] ={24358, 67616, 22744, 64716, 46348, 32368};
    const int64_t want1[6] = {374802, 376049, 350209, 381709, 370784, 373546};
    const int32_t map0[36] = {2432, 12374, 443, 1036, 5746, 2327, 8752, 10034, 10684, 5687, 21686, 10773, 1512, -1939, 10666, 11020, 1851, -366,
                              10608, 14766, 9412, 1459, 16733, 11738, 8643, 4854, 8215, 10384, 4631, 9621, 465, 5468, 4618, 8391, 16534, -3108};
    std::vector<csic::Ssim> s = top.ssim(two.data(), 1, true);
    CHECK(s.size() == 1 && s[0].windows == 6 && s[0].map.size() == 36);
    bool ok = s.size() == 1 && s[0].map.size() == 36;
    for (int c = 0; ok && c < 6; ++c) ok = s[0].sums[c] == want0[c];
    for (int k = 0; ok && k < 36; ++k) ok = s[0].map[(size_t)k] == map0[k];
    CHECK(ok);
    s = top.ssim(two.data(), 2);
    CHECK(s.size() == 2 && s[1].map.empty());
    ok = s.size() == 2;
    for (int c = 0; ok && c < 6; ++c) ok = s[0].sums[c] == want0[c] && s[1].sums[c] == want1[c];
    CHECK(ok);
    CHECK(ok && s[1].mean(csic::Ssim::Y) == 381709.0 / (65536.0 * 6.0));
    CHECK(std::strcmp(top.ssimKernelName(), "k_ssim_fast<f2>") == 0);
    CHECK(top.ssimWorkspaceBytes(2) >= 2 * 48);
    bool threw = false;
    try { top.ssim(two.data(), 65536); } catch (const csic::IllegalArgumentException &e) { threw = e.status == CSIC_EINVAL_SIZE; }
    CHECK(threw);
    csic::ImageCompressorTop small(7, 20, 4, 4, 8, 8, 8, 1, ProcessingStep::ChromaSubsampling, ProcessingStep::SpatialSampling,
                                   ProcessingStep::ColorQuantization);
    threw = false;
    try { small.ssimWorkspaceBytes(1); } catch (const csic::IllegalArgumentException &e) { threw = e.status == CSIC_EINVAL_DIMS; }
    CHECK(threw);
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::printf("usage: ssim_test cpu|gpu\n"); return 2; }
    const bool gpu = std::strcmp(argv[1], "gpu") == 0;
    try {
        cpu_checks();
        if (gpu) gpu_checks();
    } catch (const std::exception &e) { std::printf("FAILED: exception %s\n", e.what()); ++failures; }
    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
