// decode_test.cpp -- csic.hpp's decode and container API (csic_decode_*, csic_container_*) from C++.
//   cpu <dir> : the container round trip in <dir> (writeContainer / containerInfo / readContainer: payload kept, padding zeroed,
//               a flipped bit and a truncated file refused) and the decode refusals that need no device
//   gpu <dir> : the same, then ImageCompressorTop::processPlanarBits -> container -> decode on a 12 x 6 frame at factor 2 against
//               the replicated packed output, and the refused format pair
// Prints "all checks passed" and exits 0, or names the first failed check and exits 1.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "csic.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++failures; } } while (0)

static std::vector<uint8_t> slurp(const std::string &path)
{
    std::vector<uint8_t> v;
    if (FILE *f = std::fopen(path.c_str(), "rb")) {
        int c;
        while ((c = std::fgetc(f)) != EOF) v.push_back((uint8_t)c);
        std::fclose(f);
    }
    return v;
}
static void spill(const std::string &path, const std::vector<uint8_t> &v)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (f) { std::fwrite(v.data(), 1, v.size(), f); std::fclose(f); }
}
template <class Fn> static int status_of(Fn fn)
{
    try { fn(); } catch (const csic::RuntimeError &e) { return e.status; } catch (const csic::IllegalArgumentException &e) { return e.status; }
    return CSIC_OK;
}

static void cpu_checks(const std::string &dir)
{
    // 20 x 6, 4:2:0, 6 / 5 / 5, factor 1: 120 Y samples (90 bytes), 30 chroma samples (19 bytes each)
    csic_params p;
    csic_params_default(&p, 20, 6);
    p.chroma_a = 2; p.chroma_b = 0; p.y_bits = 6; p.cb_bits = 5; p.cr_bits = 5;
    csic_planar_bits_layout L;
    CHECK(csic_planar_bits_layout_of(&p, &L) == CSIC_OK);
    CHECK(L.y_bytes == 90 && L.cb_bytes == 19 && L.cr_bytes == 19 && L.payload_bytes == 128);
    const int nframes = 2;
    std::vector<uint8_t> frames((size_t)nframes * L.frame_bytes, 0xEE);      // 0xEE: the padding's canary
    const int64_t off[3] = {L.y_offset, L.cb_offset, L.cr_offset}, len[3] = {L.y_bytes, L.cb_bytes, L.cr_bytes};
    for (int k = 0; k < nframes; ++k)
        for (int pl = 0; pl < 3; ++pl)
            for (int64_t i = 0; i < len[pl]; ++i) frames[(size_t)(k * L.frame_bytes + off[pl] + i)] = (uint8_t)((k * 7 + pl * 3 + i) % 0xE0);
    const std::string path = dir + "/cpp_roundtrip.csic";
    p.out_format = CSIC_FMT_ARGB8888;                                          // the container stores PLANAR_BITS whatever this says
    csic::writeContainer(path, p, frames.data(), nframes);
    const csic_container_info info = csic::containerInfo(path);
    CHECK(info.version == 1 && info.nframes == nframes && info.payload_bytes == 128 && info.file_bytes == 80 + 2 * 128);
    CHECK(info.params.out_format == CSIC_FMT_PLANAR_BITS && info.params.width == 20 && info.params.y_bits == 6);
    const std::vector<uint8_t> file = slurp(path);
    CHECK(file.size() == 80 + 2 * 128 && std::memcmp(file.data(), "CSIC", 4) == 0);
    for (uint8_t b : file) if (b == 0xEE) { CHECK(!"a padding byte reached the file"); break; }
    const csic::Container c = csic::readContainer(path);
    CHECK(c.nframes == nframes && c.bytes.size() == frames.size());
    bool same = c.bytes.size() == frames.size();
    for (size_t i = 0; same && i < frames.size(); ++i) same = c.bytes[i] == (frames[i] == 0xEE ? 0 : frames[i]);
    CHECK(same);
    std::vector<uint8_t> bad = file;
    bad[100] ^= 0x10;
    spill(dir + "/cpp_flipped.csic", bad);
    CHECK(status_of([&] { csic::readContainer(dir + "/cpp_flipped.csic"); }) == CSIC_EFORMAT);
    bad = file;
    bad.pop_back();
    spill(dir + "/cpp_short.csic", bad);
    CHECK(status_of([&] { csic::containerInfo(dir + "/cpp_short.csic"); }) == CSIC_EFORMAT);
    CHECK(status_of([&] { csic::containerInfo(dir + "/cpp_missing.csic"); }) == CSIC_EIO);
    CHECK(csic_container_read(path.c_str(), frames.data(), frames.size() - 1) == CSIC_EINVAL_SIZE);
    CHECK(csic_container_write(nullptr, &p, frames.data(), 1) == CSIC_EINVAL_NULL);
    p.in_format = CSIC_FMT_YCBCR888X;
    CHECK(csic_container_write(path.c_str(), &p, frames.data(), 1) == CSIC_EINVAL_FORMAT);

    // decode: NULL arguments are refused before any device is touched (this half runs on machines without one)
    uint32_t px[8] = {0};
    CHECK(csic_decode_device(nullptr, px, CSIC_FMT_YCBCR888X, px, CSIC_FMT_ARGB8888, 1, nullptr) == CSIC_EINVAL_NULL);
    CHECK(csic_decode_host(nullptr, px, sizeof px, CSIC_FMT_YCBCR888X, px, 8, CSIC_FMT_ARGB8888, 1) == CSIC_EINVAL_NULL);
    CHECK(std::strcmp(csic_decode_kernel_name(nullptr, CSIC_FMT_PLANAR_BITS, CSIC_FMT_ARGB8888), "") == 0);
}

static void gpu_checks(const std::string &dir)
{
    using csic::PixelFormat;
    using csic::ProcessingStep;
    const int W = 12, H = 6, f = 2;
    csic::ImageCompressorTop top(W, H, 2, 0, 6, 5, 5, f, ProcessingStep::ChromaSubsampling, ProcessingStep::SpatialSampling,
                                 ProcessingStep::ColorQuantization);
    std::vector<uint32_t> frame((size_t)W * H);
    for (size_t i = 0; i < frame.size(); ++i) frame[i] = 0xFF000000u | (uint32_t)(i * 2654435761u >> 8);
    const std::vector<uint32_t> o = top.process(frame), oy = top.processYCbCr(frame);
    const csic::PlanarBitsFrame fr = top.processPlanarBits(frame);
    const std::string path = dir + "/cpp_frame.csic";
    csic::writeContainer(path, top.params(), fr.bytes.data(), 1);
    const csic::Container c = csic::readContainer(path);
    const std::vector<uint32_t> d = top.decode(c.bytes.data(), c.bytes.size());
    const std::vector<uint32_t> dy = top.decode(fr, PixelFormat::YCBCR888X);
    const std::vector<uint32_t> dp = top.decode(oy.data(), oy.size() * 4, PixelFormat::YCBCR888X, PixelFormat::ARGB8888);
    CHECK(d.size() == frame.size() && dy.size() == frame.size() && dp.size() == frame.size());
    bool ok = d.size() == frame.size() && dy.size() == frame.size() && dp.size() == frame.size();
    for (int r = 0; ok && r < H; ++r)
        for (int x = 0; ok && x < W; ++x) {
            const size_t j = (size_t)(r / f) * top.outWidth() + (size_t)(x / f), i = (size_t)r * W + x;
            ok = d[i] == o[j] && dy[i] == oy[j] && dp[i] == o[j];
        }
    CHECK(ok);
    CHECK(std::strncmp(top.decodeKernelName(PixelFormat::PLANAR_BITS), "k_decode", 8) == 0);
    CHECK(status_of([&] { top.decode(o.data(), o.size() * 4, PixelFormat::ARGB8888, PixelFormat::YCBCR888X); }) == CSIC_EINVAL_FORMAT);
    CHECK(status_of([&] { top.decode(o.data(), o.size() * 4 - 4, PixelFormat::ARGB8888, PixelFormat::ARGB8888); }) == CSIC_EINVAL_SIZE);
    CHECK(std::strcmp(top.decodeKernelName(PixelFormat::ARGB8888, PixelFormat::YCBCR888X), "") == 0);
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::printf("usage: decode_test cpu|gpu <scratch directory>\n"); return 2; }
    const bool gpu = std::strcmp(argv[1], "gpu") == 0;
    try {
        cpu_checks(argv[2]);
        if (gpu) gpu_checks(argv[2]);
    } catch (const std::exception &e) { std::printf("FAILED: exception %s\n", e.what()); ++failures; }
    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
