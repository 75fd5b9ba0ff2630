// view_test.cpp -- csic.hpp's view decode (csic_decode_view_*) from C++.
//   cpu : the refusals that touch no device
//   gpu : the same, then ImageCompressorTop::processPlanarBits -> decodeView on a 26 x 18 frame at factor 2 against the definition
//         computed here from decode() of the same frame -- the byte sums of every box, + s s / 2, >> 2 log2 s -- at every scale, on
//         both kernels, and the refused views
// Prints "all checks passed" and exits 0, or names the first failed check and exits 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "csic.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++failures; } } while (0)

template <class Fn> static int status_of(Fn fn)
{
    try { fn(); } catch (const csic::RuntimeError &e) { return e.status; } catch (const csic::IllegalArgumentException &e) { return e.status; }
    return CSIC_OK;
}

static void cpu_checks()
{
    uint32_t px[8] = {0};
    const csic::View v(0, 0, 2, 2, 2);
    CHECK(sizeof(csic::View) == sizeof(csic_view) && v.x0 == 0 && v.width == 2 && v.scale == 2 && csic::View(1, 2, 3, 4).scale == 1);
    CHECK(csic_decode_view_device(nullptr, px, CSIC_FMT_YCBCR888X, &v, px, CSIC_FMT_ARGB8888, 1, nullptr) == CSIC_EINVAL_NULL);
    CHECK(csic_decode_view_host(nullptr, px, sizeof px, CSIC_FMT_YCBCR888X, &v, px, 4, CSIC_FMT_ARGB8888, 1) == CSIC_EINVAL_NULL);
    CHECK(std::strcmp(csic_decode_view_kernel_name(nullptr, CSIC_FMT_PLANAR_BITS, CSIC_FMT_ARGB8888, &v), "") == 0);
}

static std::vector<uint32_t> box(const std::vector<uint32_t> &d, int W, const csic::View &v)
{
    const int s = v.scale;
    int ls = 0;
    while ((1 << ls) < s) ++ls;
    std::vector<uint32_t> out((size_t)v.width * v.height);
    for (int r = 0; r < v.height; ++r)
        for (int c = 0; c < v.width; ++c) {
            uint32_t px = 0;
            for (int b = 0; b < 4; ++b) {
                uint32_t sum = 0;
                for (int i = 0; i < s; ++i)
                    for (int j = 0; j < s; ++j) sum += (d[(size_t)(v.y0 + r * s + i) * W + (size_t)(v.x0 + c * s + j)] >> (8 * b)) & 0xFFu;
                px |= ((sum + (uint32_t)((s * s) >> 1)) >> (2 * ls)) << (8 * b);
            }
            out[(size_t)r * v.width + c] = px;
        }
    return out;
}

static void gpu_checks()
{
    using csic::PixelFormat;
    using csic::ProcessingStep;
    const int W = 26, H = 18;
    csic::ImageCompressorTop top(W, H, 2, 0, 6, 5, 5, 2, ProcessingStep::ChromaSubsampling, ProcessingStep::SpatialSampling,
                                 ProcessingStep::ColorQuantization);
    std::vector<uint32_t> frame((size_t)W * H);
    for (size_t i = 0; i < frame.size(); ++i) frame[i] = 0xFF000000u | (uint32_t)(i * 2654435761u >> 8);
    const csic::PlanarBitsFrame fr = top.processPlanarBits(frame);
    const std::vector<uint32_t> oy = top.processYCbCr(frame);
    for (PixelFormat f : {PixelFormat::ARGB8888, PixelFormat::YCBCR888X}) {
        const std::vector<uint32_t> d = top.decode(fr, f);
        const csic::View views[] = {{0, 0, W, H, 1}, {1, 3, 5, 4, 2}, {3, 1, 4, 3, 4}, {0, 0, 13, 7, 2}, {1, 5, 3, 1, 8}, {10, 0, 1, 1, 16}, {2, 2, 8, 2, 1}};
        for (const csic::View &v : views) {
            CHECK(top.decodeView(fr, v, f) == box(d, W, v));
            CHECK(top.decodeView(oy.data(), oy.size() * 4, v, PixelFormat::YCBCR888X, f) == box(d, W, v));
        }
    }
    CHECK(std::strncmp(top.decodeViewKernelName(PixelFormat::PLANAR_BITS, csic::View(3, 1, 4, 3, 4)), "k_view<s4,bits,argb", 19) == 0);
    CHECK(std::strncmp(top.decodeViewKernelName(PixelFormat::PLANAR_BITS, csic::View(1, 3, 5, 4, 2)), "k_view_gen<bits,argb>", 21) == 0);
    CHECK(status_of([&] { top.decodeView(fr, csic::View(0, 0, 14, 7, 2)); }) == CSIC_EINVAL_SIZE);
    CHECK(status_of([&] { top.decodeView(fr, csic::View(0, 0, 4, 4, 3)); }) == CSIC_EINVAL_SIZE);
    CHECK(status_of([&] { top.decodeView(fr, csic::View(0, 0, 0, 4, 1)); }) == CSIC_EINVAL_SIZE);
    CHECK(status_of([&] { top.decodeView(oy.data(), oy.size() * 4, csic::View(0, 0, 4, 4, 1), PixelFormat::ARGB8888, PixelFormat::YCBCR888X); }) == CSIC_EINVAL_FORMAT);
    CHECK(std::strcmp(top.decodeViewKernelName(PixelFormat::PLANAR_BITS, csic::View(0, 0, 27, 1, 1)), "") == 0);
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::printf("usage: view_test cpu|gpu\n"); return 2; }
    try {
        cpu_checks();
        if (std::strcmp(argv[1], "gpu") == 0) gpu_checks();
    } catch (const std::exception &e) { std::printf("FAILED: exception %s\n", e.what()); ++failures; }
    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
