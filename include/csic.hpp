// csic.hpp -- header-only C++17 host layer over the C ABI of csic.h, keeping the reference's generator
// names and argument lists (Scala originals under /root/reference/src/main/scala/jpeg/):
//   csic::ImageProcessorParams  <- case class ImageProcessorParams           ImageProcessor.scala:15-29
//   csic::ProcessingStep        <- object ProcessingStep extends ChiselEnum   ImageCompressorTop.scala:7-9
//   csic::ImageCompressorTop    <- class ImageCompressorTop(11 parameters)    ImageCompressorTop.scala:11-25
//   csic::ImageProcessor        <- class ImageProcessor(p)                    ImageProcessor.scala:31-63
// Every require() of the reference surfaces as csic::IllegalArgumentException thrown from the
// constructor, device failures as csic::RuntimeError.  No compute happens on the host.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cmath>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "csic.h"

namespace csic {

struct IllegalArgumentException : std::invalid_argument {
    int status;
    IllegalArgumentException(int st, const std::string &m) : std::invalid_argument("requirement failed: " + m), status(st) {}
};

struct RuntimeError : std::runtime_error {
    int status;
    RuntimeError(int st, const std::string &m) : std::runtime_error(m), status(st) {}
};

inline int check(int status)
{
    if (status >= 0) return status;
    std::string msg = csic_last_error();
    if (msg.empty()) msg = csic_strerror(status);
    if (status <= CSIC_EINVAL_NULL && status >= CSIC_EINVAL_SIZE) throw IllegalArgumentException(status, msg);
    throw RuntimeError(status, msg);   // device, memory and file errors
}

enum class ProcessingStep : int32_t { NoOp = 0, SpatialSampling = 1, ColorQuantization = 2, ChromaSubsampling = 3 };
enum class Rounding : int32_t { FLOOR_HW = CSIC_ROUND_FLOOR_HW, TRUNC_SW = CSIC_ROUND_TRUNC_SW };
enum class PixelFormat : int32_t { ARGB8888 = CSIC_FMT_ARGB8888, YCBCR888X = CSIC_FMT_YCBCR888X, PLANAR = CSIC_FMT_PLANAR,
                                   PLANAR_BITS = CSIC_FMT_PLANAR_BITS };

struct ImageProcessorParams {
    int width, height, factor, chromaParamA, chromaParamB;
    ImageProcessorParams(int width_, int height_, int factor_, int chromaParamA_, int chromaParamB_)
        : width(width_), height(height_), factor(factor_), chromaParamA(chromaParamA_), chromaParamB(chromaParamB_)
    {
        csic_params p = c_params();
        check(csic_validate(&p));      // the five require()s of ImageProcessor.scala:22-28
    }
    csic_params c_params(Rounding r = Rounding::FLOOR_HW, PixelFormat f = PixelFormat::ARGB8888) const
    {
        csic_params p;
        csic_params_default(&p, width, height);
        p.chroma_a = chromaParamA; p.chroma_b = chromaParamB; p.factor = factor;
        p.rounding = (int32_t)r; p.out_format = (int32_t)f; p.strict_divisible = 1;
        return p;
    }
};

// Stand-in for scrimage's image objects: width, height, packed ARGB ints (0xAARRGGBB).
struct Image {
    int width = 0, height = 0;
    std::vector<uint32_t> argb;
};

// object ImageProcessorModel, src/test/scala/jpeg/ImageProcessorModel.scala:9-53 -- I/O helpers, no arithmetic.
struct ImageProcessorModel {
    static Image readImage(const std::string &file)                                  // :14-16
    {
        Image im;
        int32_t w = 0, h = 0;
        check(csic_png_info(file.c_str(), &w, &h));
        im.width = w; im.height = h;
        im.argb.resize((size_t)w * h);
        check(csic_png_read_argb(file.c_str(), im.argb.data(), im.argb.size()));
        return im;
    }
    static void writeImage(const Image &im, const std::string &file, int compression = 6)   // :18-22
    {
        check(csic_png_write_argb(file.c_str(), im.argb.data(), im.width, im.height, compression));
    }
    static ImageProcessorParams getImageParams(const Image &im, int numPixelsPerCycle)      // :33-41
    {
        return ImageProcessorParams(im.width, im.height, numPixelsPerCycle, 4, 4);
    }
};

// One frame in the subsampled planar format (CSIC_FMT_PLANAR, csic.h: csic_planar_layout): the frame buffer as the device wrote
// it, and views of its three planes -- Y: y_width x y_height bytes, Cb / Cr: chroma_samples bytes each in sample order.
struct PlanarFrame {
    csic_planar_layout layout{};
    std::vector<uint8_t> bytes;                                   // layout.frame_bytes long
    const uint8_t *y() const { return bytes.data() + layout.y_offset; }
    const uint8_t *cb() const { return bytes.data() + layout.cb_offset; }
    const uint8_t *cr() const { return bytes.data() + layout.cr_offset; }
};

// One frame in the bit-packed planar format (CSIC_FMT_PLANAR_BITS, csic.h: csic_planar_bits_layout): the frame buffer as the device
// wrote it; plane p holds its samples LSB first at layout.y_bits / cb_bits / cr_bits bits each.
struct PlanarBitsFrame {
    csic_planar_bits_layout layout{};
    std::vector<uint8_t> bytes;                                   // layout.frame_bytes long
};

// A window of a decoded frame for ImageCompressorTop::decodeView (csic.h: csic_view): the source rectangle starts at (x0, y0) and
// covers width * scale x height * scale decoded pixels; width and height count OUTPUT pixels; scale is 1, 2, 4, 8 or 16.
struct View : csic_view {
    View(int x0_, int y0_, int width_, int height_, int scale_ = 1) : csic_view{x0_, y0_, width_, height_, scale_} {}
};

// A .csic file (csic.h: csic_container_*): `nframes` bit-packed planar frame buffers of one parameter set, layout.frame_bytes apart
// in `bytes`.  Host only -- none of the three functions needs a GPU.  File and format errors surface as csic::RuntimeError with
// status CSIC_EIO / CSIC_EFORMAT.
struct Container {
    csic_params params{};
    int nframes = 0;
    csic_planar_bits_layout layout{};
    std::vector<uint8_t> bytes;                                   // nframes * layout.frame_bytes, zero outside the planes' payload
};
inline csic_container_info containerInfo(const std::string &file)
{
    csic_container_info info;
    check(csic_container_info_of(file.c_str(), &info));
    return info;
}
// frames: nframes PLANAR_BITS frame buffers of `p`, frame_bytes apart (p.out_format does not matter); coding = CSIC_CODING_RAW writes
// version 1, CSIC_CODING_GROUPS packs every frame on the host and writes version 3, CSIC_CODING_RICE version 4.  readContainer reads all.
inline void writeContainer(const std::string &file, const csic_params &p, const void *frames, int nframes, int coding = CSIC_CODING_RAW)
{
    check(csic_container_write_ex(file.c_str(), &p, frames, nframes, coding));
}
// version 3 (CSIC_CODING_GROUPS), 4 (CSIC_CODING_RICE) or 7 (CSIC_CODING_RANS) from frames that are packed already (csic_pack_device's /
// csic_rice_pack_device's / csic_rans_pack_device's output on the host): frame k at coded + k * stride_bytes
inline void writeContainerCoded(const std::string &file, const csic_params &p, const void *coded, size_t stride_bytes,
                                const std::vector<uint64_t> &sizes, int coding = CSIC_CODING_GROUPS)
{
    check(csic_container_write_coded_ex(file.c_str(), &p, coded, stride_bytes, sizes.data(), (int32_t)sizes.size(), coding));
}
// the stored bytes of each frame: a version-3 or version-4 file's table, payload_bytes per frame for version 1
inline std::vector<uint64_t> containerCodedSizes(const std::string &file)
{
    std::vector<uint64_t> sizes((size_t)containerInfo(file).nframes);
    check(csic_container_coded_sizes(file.c_str(), sizes.data(), (int32_t)sizes.size()));
    return sizes;
}
inline Container readContainer(const std::string &file)
{
    Container c;
    const csic_container_info info = containerInfo(file);
    c.params = info.params;
    c.nframes = info.nframes;
    check(csic_planar_bits_layout_of(&c.params, &c.layout));
    c.bytes.resize((size_t)c.nframes * (size_t)c.layout.frame_bytes);
    check(csic_container_read(file.c_str(), c.bytes.data(), c.bytes.size()));
    return c;
}

// The lossless group coding of PLANAR_BITS frames (csic.h: csic_pack_*), host codec: needs no GPU.  pack: one frame buffer
// (frame_bytes) -> its coded bytes; unpack: coded bytes -> a frame buffer, zero outside the planes' payload.  Damaged input surfaces as
// csic::RuntimeError with status CSIC_EFORMAT.
inline csic_pack_layout packLayout(const csic_params &p)
{
    csic_pack_layout layout;
    check(csic_pack_layout_of(&p, &layout));
    return layout;
}
inline std::vector<uint8_t> pack(const csic_params &p, const void *bitsFrame)
{
    std::vector<uint8_t> coded((size_t)packLayout(p).bound_bytes);
    uint64_t size = 0;
    check(csic_pack_host(&p, bitsFrame, coded.data(), coded.size(), &size));
    coded.resize((size_t)size);
    return coded;
}
inline std::vector<uint8_t> unpack(const csic_params &p, const void *coded, size_t codedBytes)
{
    csic_params q = p;
    q.out_format = CSIC_FMT_PLANAR_BITS;
    csic_planar_bits_layout layout;
    check(csic_planar_bits_layout_of(&q, &layout));
    std::vector<uint8_t> frame((size_t)layout.frame_bytes, 0);
    check(csic_unpack_host(&p, coded, codedBytes, frame.data()));
    return frame;
}
// The same for the Rice coding (csic.h: csic_rice_*).
inline csic_rice_layout riceLayout(const csic_params &p)
{
    csic_rice_layout layout;
    check(csic_rice_layout_of(&p, &layout));
    return layout;
}
inline std::vector<uint8_t> ricePack(const csic_params &p, const void *bitsFrame)
{
    std::vector<uint8_t> coded((size_t)riceLayout(p).bound_bytes);
    uint64_t size = 0;
    check(csic_rice_pack_host(&p, bitsFrame, coded.data(), coded.size(), &size));
    coded.resize((size_t)size);
    return coded;
}
inline std::vector<uint8_t> riceUnpack(const csic_params &p, const void *coded, size_t codedBytes)
{
    csic_params q = p;
    q.out_format = CSIC_FMT_PLANAR_BITS;
    csic_planar_bits_layout layout;
    check(csic_planar_bits_layout_of(&q, &layout));
    std::vector<uint8_t> frame((size_t)layout.frame_bytes, 0);
    check(csic_rice_unpack_host(&p, coded, codedBytes, frame.data()));
    return frame;
}

// The same for the rANS coding (csic.h: csic_rans_*).
inline csic_rans_layout ransLayout(const csic_params &p)
{
    csic_rans_layout layout;
    check(csic_rans_layout_of(&p, &layout));
    return layout;
}
inline std::vector<uint8_t> ransPack(const csic_params &p, const void *bitsFrame)
{
    std::vector<uint8_t> coded((size_t)ransLayout(p).bound_bytes);
    uint64_t size = 0;
    check(csic_rans_pack_host(&p, bitsFrame, coded.data(), coded.size(), &size));
    coded.resize((size_t)size);
    return coded;
}
inline std::vector<uint8_t> ransUnpack(const csic_params &p, const void *coded, size_t codedBytes)
{
    csic_params q = p;
    q.out_format = CSIC_FMT_PLANAR_BITS;
    csic_planar_bits_layout layout;
    check(csic_planar_bits_layout_of(&q, &layout));
    std::vector<uint8_t> frame((size_t)layout.frame_bytes, 0);
    check(csic_rans_unpack_host(&p, coded, codedBytes, frame.data()));
    return frame;
}

// The temporal layer in front of either coding (csic.h: csic_delta_*), host codec: needs no GPU.  delta: nframes frame buffers
// (frame_bytes apart) -> their difference frames (zero outside the planes' payload) and the maps (map_stride apart, map_bytes of each
// written); undelta: the inverse, damaged maps surface as csic::RuntimeError with status CSIC_EFORMAT.
struct DeltaFrames {
    std::vector<uint8_t> diff, maps;
};
inline csic_delta_layout deltaLayout(const csic_params &p)
{
    csic_delta_layout layout;
    check(csic_delta_layout_of(&p, &layout));
    return layout;
}
// nframes zeroed frame buffers of these parameters: the buffer both layers' host codecs write frames or difference frames into
inline std::vector<uint8_t> zeroedFrames(const csic_params &p, int nframes)
{
    csic_params q = p;
    q.out_format = CSIC_FMT_PLANAR_BITS;
    csic_planar_bits_layout layout;
    check(csic_planar_bits_layout_of(&q, &layout));
    return std::vector<uint8_t>((size_t)(nframes > 0 ? nframes : 0) * (size_t)layout.frame_bytes, 0);
}
inline DeltaFrames delta(const csic_params &p, const void *frames, int nframes, int gop)
{
    DeltaFrames d{zeroedFrames(p, nframes), {}};
    d.maps.assign((size_t)(nframes > 0 ? nframes : 0) * (size_t)deltaLayout(p).map_stride, 0);
    check(csic_delta_host(&p, frames, nframes, gop, d.diff.data(), d.maps.data()));
    return d;
}
inline std::vector<uint8_t> undelta(const csic_params &p, const void *diff, const void *maps, int nframes, int gop)
{
    std::vector<uint8_t> frames = zeroedFrames(p, nframes);
    check(csic_undelta_host(&p, diff, maps, nframes, gop, frames.data()));
    return frames;
}
// The motion-compensated temporal layer (csic.h: csic_mc_*), host codec: as delta / undelta with a range of 0..7 and the maps of
// csic_mc_layout_of; the difference frames never share memory with the frames.
inline csic_mc_layout mcLayout(const csic_params &p)
{
    csic_mc_layout layout;
    check(csic_mc_layout_of(&p, &layout));
    return layout;
}
inline DeltaFrames mcDelta(const csic_params &p, const void *frames, int nframes, int gop, int range)
{
    DeltaFrames d{zeroedFrames(p, nframes), {}};
    d.maps.assign((size_t)(nframes > 0 ? nframes : 0) * (size_t)mcLayout(p).map_stride, 0);
    check(csic_mc_delta_host(&p, frames, nframes, gop, range, d.diff.data(), d.maps.data()));
    return d;
}
inline std::vector<uint8_t> mcUndelta(const csic_params &p, const void *diff, const void *maps, int nframes, int gop)
{
    std::vector<uint8_t> frames = zeroedFrames(p, nframes);
    check(csic_mc_undelta_host(&p, diff, maps, nframes, gop, frames.data()));
    return frames;
}
// The row-prediction layer (csic.h: csic_rows_*), host codec: every frame on its own, the maps of csic_rows_layout_of; the difference
// frames never share memory with the frames (unrows may work in place through the C ABI).
inline csic_rows_layout rowsLayout(const csic_params &p)
{
    csic_rows_layout layout;
    check(csic_rows_layout_of(&p, &layout));
    return layout;
}
inline DeltaFrames rows(const csic_params &p, const void *frames, int nframes)
{
    DeltaFrames d{zeroedFrames(p, nframes), {}};
    d.maps.assign((size_t)(nframes > 0 ? nframes : 0) * (size_t)rowsLayout(p).map_stride, 0);
    check(csic_rows_host(&p, frames, nframes, d.diff.data(), d.maps.data()));
    return d;
}
inline std::vector<uint8_t> unrows(const csic_params &p, const void *diff, const void *maps, int nframes)
{
    std::vector<uint8_t> frames = zeroedFrames(p, nframes);
    check(csic_unrows_host(&p, diff, maps, nframes, frames.data()));
    return frames;
}
// version 8: every frame through the row-prediction layer and then `coding` (CSIC_CODING_GROUPS, _RICE or _RANS), on the host;
// containerRows: whether a file uses the layer
inline void writeContainerRows(const std::string &file, const csic_params &p, const void *frames, int nframes, int coding)
{
    check(csic_container_write_rows(file.c_str(), &p, frames, nframes, coding));
}
inline bool containerRows(const std::string &file)
{
    int32_t flag = 0;
    check(csic_container_rows(file.c_str(), &flag));
    return flag != 0;
}
// version 5: the frames as a sequence, delta and packing on the host (coding CSIC_CODING_GROUPS or CSIC_CODING_RICE); readContainer
// returns the frames themselves
inline void writeContainerSeq(const std::string &file, const csic_params &p, const void *frames, int nframes, int coding, int gop)
{
    check(csic_container_write_seq(file.c_str(), &p, frames, nframes, coding, gop));
}
// version 6: the same through the motion-compensated layer at `range` (0..7); containerMotion: a file's range, -1 below version 6
inline void writeContainerSeq(const std::string &file, const csic_params &p, const void *frames, int nframes, int coding, int gop, int range)
{
    check(csic_container_write_seq_ex(file.c_str(), &p, frames, nframes, coding, gop, range));
}
inline int containerMotion(const std::string &file)
{
    int32_t range = -1;
    check(csic_container_motion(file.c_str(), &range));
    return range;
}
inline int containerGop(const std::string &file)
{
    int32_t gop = 0;
    check(csic_container_gop(file.c_str(), &gop));
    return gop;
}

// The six sums of squared errors of one frame (csic.h: csic_distortion_*), in the order R, G, B, Y, Cb, Cr, over `pixels` input
// pixels, with the PSNR helpers (+inf at zero error).
struct Distortion {
    enum Channel { R = 0, G = 1, B = 2, Y = 3, Cb = 4, Cr = 5 };
    uint64_t sse[CSIC_DIST_CHANNELS] = {0, 0, 0, 0, 0, 0};
    int64_t pixels = 0;
    double mse(int ch) const { return (double)sse[ch] / (double)pixels; }
    double psnr(int ch) const { return psnrOf(sse[ch], 1); }
    double psnrRgb() const { return psnrOf(sse[R] + sse[G] + sse[B], 3); }

private:
    double psnrOf(uint64_t e, int channels) const
    {
        if (e == 0) return std::numeric_limits<double>::infinity();
        return 10.0 * std::log10(255.0 * 255.0 * (double)channels * (double)pixels / (double)e);
    }
};

// The six sums of the 8 x 8 block SSIM of one frame (csic.h: csic_ssim_*), in the order R, G, B, Y, Cb, Cr: each the sum of the
// windows' 16.16 fixed-point quotients over `windows` windows; `map`, when asked for, holds the quotients [channel][wy][wx].
struct Ssim {
    enum Channel { R = 0, G = 1, B = 2, Y = 3, Cb = 4, Cr = 5 };
    int64_t sums[CSIC_DIST_CHANNELS] = {0, 0, 0, 0, 0, 0};
    int64_t windows = 0;
    std::vector<int32_t> map;
    double mean(int ch) const { return (double)sums[ch] / ((double)CSIC_SSIM_ONE * (double)windows); }
    double meanRgb() const { return (mean(R) + mean(G) + mean(B)) / 3.0; }
};

// The histograms of one compressed frame (csic.h: csic_code_stats_*): hist[kind][plane][bin], kind 0 = the sample codes, 1 = their
// left-predicted residuals, planes Y, Cb, Cr with bits[plane] bits per code; `pixels` = width * height of the image.  entropy() is
// the zero-order entropy in bits per sample, bitsPerPixel() / idealBytes() what an ideal coder of that kind spends on the frame;
// Best takes per plane the cheapest of raw, codes and residuals.  Double precision, from the counts.
struct CodeStats {
    enum Kind { Codes = 0, Residuals = 1, Best = 2 };
    enum Plane { Y = 0, Cb = 1, Cr = 2 };
    uint64_t hist[CSIC_STATS_KINDS][CSIC_STATS_PLANES][CSIC_STATS_BINS] = {};
    int bits[CSIC_STATS_PLANES] = {0, 0, 0};
    int64_t pixels = 0;
    uint64_t samples(int plane) const
    {
        uint64_t n = 0;
        for (int i = 0; i < CSIC_STATS_BINS; ++i) n += hist[0][plane][i];
        return n;
    }
    double entropy(int kind, int plane) const
    {
        uint64_t total = 0;
        for (int i = 0; i < CSIC_STATS_BINS; ++i) total += hist[kind][plane][i];
        double h = 0.0;
        for (int i = 0; i < CSIC_STATS_BINS; ++i) {
            if (hist[kind][plane][i] == 0) continue;
            const double p = (double)hist[kind][plane][i] / (double)total;
            h -= p * std::log2(p);
        }
        return h > 0.0 ? h : 0.0;
    }
    double totalBits(int kind) const
    {
        double t = 0.0;
        for (int p = 0; p < CSIC_STATS_PLANES; ++p) {
            double b = kind == Best ? std::fmin((double)bits[p], std::fmin(entropy(Codes, p), entropy(Residuals, p))) : entropy(kind, p);
            t += (double)samples(p) * b;
        }
        return t;
    }
    double bitsPerPixel(int kind) const { return totalBits(kind) / (double)pixels; }
    int64_t idealBytes(int kind) const { return (int64_t)std::ceil(totalBits(kind) / 8.0); }
    double rawBitsPerPixel() const
    {
        double t = 0.0;
        for (int p = 0; p < CSIC_STATS_PLANES; ++p) t += (double)samples(p) * (double)bits[p];
        return t / (double)pixels;
    }
    bool operator==(const CodeStats &o) const
    {
        return std::memcmp(hist, o.hist, sizeof hist) == 0 && std::memcmp(bits, o.bits, sizeof bits) == 0 && pixels == o.pixels;
    }
};

// The candidates of a quantiser sweep in rank order (csic.h: csic_qsweep_rank): `results` holds one csic_qsweep_result per frame,
// weights are 1..255, max_bits 1..8; ascending (distortion, est_bytes, y_bits, cb_bits, cr_bits).
inline std::vector<csic_qsweep_candidate> qsweepRank(const csic_params &p, const std::vector<csic_qsweep_result> &results, int coding = CSIC_CODING_RANS,
                                                     const uint8_t (&weights)[3] = {1, 1, 1}, const uint8_t (&max_bits)[3] = {8, 8, 8})
{
    std::vector<csic_qsweep_candidate> out(CSIC_QSWEEP_MAX_CANDIDATES);
    int32_t n = (int32_t)out.size();
    check(csic_qsweep_rank(&p, results.data(), (int32_t)results.size(), coding, weights, max_bits, out.data(), &n));
    out.resize((size_t)n);
    return out;
}

// One validated parameter set bound to one device (csic_plan_create / csic_plan_destroy), for what works on compressed frames of
// known parameters -- a container's, for instance -- rather than on an image.
class Plan {
public:
    explicit Plan(const csic_params &p, int device = 0) : params_(p) { check(csic_plan_create(&params_, device, &plan_)); }
    Plan(const Plan &) = delete;
    Plan &operator=(const Plan &) = delete;
    ~Plan() { csic_plan_destroy(plan_); }
    csic_plan *native() { return plan_; }
    const csic_params &params() const { return params_; }
    // `nframes` compressed frames in host memory (PLANAR_BITS / PLANAR frame buffers, frame_bytes apart) -> one CodeStats per frame
    std::vector<CodeStats> codeStats(const void *src, size_t src_bytes, PixelFormat src_format = PixelFormat::PLANAR_BITS, int nframes = 1)
    {
        const size_t n = (size_t)(nframes > 0 ? nframes : 0);
        std::vector<uint64_t> hist(n * CSIC_STATS_KINDS * CSIC_STATS_PLANES * CSIC_STATS_BINS);
        check(csic_code_stats_host(plan_, src, src_bytes, (int32_t)src_format, nframes, hist.data()));
        std::vector<CodeStats> out(n);
        for (size_t k = 0; k < n; ++k) {
            std::memcpy(out[k].hist, hist.data() + k * CSIC_STATS_KINDS * CSIC_STATS_PLANES * CSIC_STATS_BINS, sizeof out[k].hist);
            out[k].bits[0] = params_.y_bits; out[k].bits[1] = params_.cb_bits; out[k].bits[2] = params_.cr_bits;
            out[k].pixels = (int64_t)params_.width * params_.height;
        }
        return out;
    }
    // device-resident: d_hist receives nframes * 2 * 3 * 256 counts (8-byte aligned); asynchronous on `hip_stream`, no workspace,
    // no allocation, capturable
    void codeStatsDevice(const void *d_src, PixelFormat src_format, int nframes, uint64_t *d_hist, void *hip_stream)
    {
        check(csic_code_stats_device(plan_, d_src, (int32_t)src_format, nframes, d_hist, hip_stream));
    }
    const char *codeStatsKernelName(PixelFormat src_format = PixelFormat::PLANAR_BITS)
    {
        return csic_code_stats_kernel_name(plan_, (int32_t)src_format);
    }
    int64_t codeStatsBlockSamples(PixelFormat src_format = PixelFormat::PLANAR_BITS)
    {
        int64_t n = 0;
        check(csic_code_stats_block_samples(plan_, (int32_t)src_format, &n));
        return n;
    }
    // the group coding of this plan's PLANAR_BITS frames: on the host (csic::pack / csic::unpack of the plan's parameters) ...
    csic_pack_layout packLayout() const { return csic::packLayout(params_); }
    std::vector<uint8_t> pack(const void *bitsFrame) const { return csic::pack(params_, bitsFrame); }
    std::vector<uint8_t> unpack(const void *coded, size_t codedBytes) const { return csic::unpack(params_, coded, codedBytes); }
    // ... and device-resident: frames frame_bytes / bound_bytes apart, 256-byte aligned, through a workspace of packWorkspaceBytes;
    // asynchronous on `hip_stream`, no allocation, capturable.  unpackDevice does not validate (csic.h).
    size_t packWorkspaceBytes(int nframes = 1)
    {
        size_t bytes = 0;
        check(csic_pack_workspace_bytes(plan_, nframes, &bytes));
        return bytes;
    }
    void packDevice(const void *d_bits, int nframes, void *d_coded, uint64_t *d_sizes, void *d_workspace, size_t workspace_bytes, void *hip_stream)
    {
        check(csic_pack_device(plan_, d_bits, nframes, d_coded, d_sizes, d_workspace, workspace_bytes, hip_stream));
    }
    void unpackDevice(const void *d_coded, int nframes, void *d_bits, void *d_workspace, size_t workspace_bytes, void *hip_stream)
    {
        check(csic_unpack_device(plan_, d_coded, nframes, d_bits, d_workspace, workspace_bytes, hip_stream));
    }
    const char *packKernelName() { return csic_pack_kernel_name(plan_); }
    // the Rice coding of this plan's PLANAR_BITS frames, host and device; riceUnpackDevice is one pass and takes no workspace
    csic_rice_layout riceLayout() const { return csic::riceLayout(params_); }
    std::vector<uint8_t> ricePack(const void *bitsFrame) const { return csic::ricePack(params_, bitsFrame); }
    std::vector<uint8_t> riceUnpack(const void *coded, size_t codedBytes) const { return csic::riceUnpack(params_, coded, codedBytes); }
    size_t riceWorkspaceBytes(int nframes = 1)
    {
        size_t bytes = 0;
        check(csic_rice_workspace_bytes(plan_, nframes, &bytes));
        return bytes;
    }
    void ricePackDevice(const void *d_bits, int nframes, void *d_coded, uint64_t *d_sizes, void *d_workspace, size_t workspace_bytes, void *hip_stream)
    {
        check(csic_rice_pack_device(plan_, d_bits, nframes, d_coded, d_sizes, d_workspace, workspace_bytes, hip_stream));
    }
    void riceUnpackDevice(const void *d_coded, int nframes, void *d_bits, void *hip_stream)
    {
        check(csic_rice_unpack_device(plan_, d_coded, nframes, d_bits, hip_stream));
    }
    const char *riceKernelName() { return csic_rice_kernel_name(plan_); }
    // the rANS coding of this plan's PLANAR_BITS frames, host and device; ransUnpackDevice is one pass and takes no workspace
    csic_rans_layout ransLayout() const { return csic::ransLayout(params_); }
    std::vector<uint8_t> ransPack(const void *bitsFrame) const { return csic::ransPack(params_, bitsFrame); }
    std::vector<uint8_t> ransUnpack(const void *coded, size_t codedBytes) const { return csic::ransUnpack(params_, coded, codedBytes); }
    size_t ransWorkspaceBytes(int nframes = 1)
    {
        size_t bytes = 0;
        check(csic_rans_workspace_bytes(plan_, nframes, &bytes));
        return bytes;
    }
    void ransPackDevice(const void *d_bits, int nframes, void *d_coded, uint64_t *d_sizes, void *d_workspace, size_t workspace_bytes, void *hip_stream)
    {
        check(csic_rans_pack_device(plan_, d_bits, nframes, d_coded, d_sizes, d_workspace, workspace_bytes, hip_stream));
    }
    void ransUnpackDevice(const void *d_coded, int nframes, void *d_bits, void *hip_stream)
    {
        check(csic_rans_unpack_device(plan_, d_coded, nframes, d_bits, hip_stream));
    }
    const char *ransKernelName() { return csic_rans_kernel_name(plan_); }
    // the temporal layer over this plan's PLANAR_BITS frames, host and device (no workspace; d_diff may be d_frames, in place)
    csic_delta_layout deltaLayout() const { return csic::deltaLayout(params_); }
    DeltaFrames delta(const void *frames, int nframes, int gop) const { return csic::delta(params_, frames, nframes, gop); }
    std::vector<uint8_t> undelta(const void *diff, const void *maps, int nframes, int gop) const { return csic::undelta(params_, diff, maps, nframes, gop); }
    void deltaDevice(const void *d_frames, int nframes, int gop, void *d_diff, void *d_maps, void *hip_stream)
    {
        check(csic_delta_device(plan_, d_frames, nframes, gop, d_diff, d_maps, hip_stream));
    }
    void undeltaDevice(const void *d_diff, const void *d_maps, int nframes, int gop, void *d_frames, void *hip_stream)
    {
        check(csic_undelta_device(plan_, d_diff, d_maps, nframes, gop, d_frames, hip_stream));
    }
    const char *deltaKernelName() { return csic_delta_kernel_name(plan_); }
    // the motion-compensated layer, host and device (d_workspace: nframes * mcLayout().workspace_frame_bytes bytes; never in place)
    csic_mc_layout mcLayout() const { return csic::mcLayout(params_); }
    DeltaFrames rows(const void *frames, int nframes) const { return csic::rows(params_, frames, nframes); }
    std::vector<uint8_t> unrows(const void *diff, const void *maps, int nframes) const { return csic::unrows(params_, diff, maps, nframes); }
    void rowsDevice(const void *d_frames, int nframes, void *d_diff, void *d_maps, void *hip_stream) { check(csic_rows_device(plan_, d_frames, nframes, d_diff, d_maps, hip_stream)); }
    void unrowsDevice(const void *d_diff, const void *d_maps, int nframes, void *d_frames, void *hip_stream) { check(csic_unrows_device(plan_, d_diff, d_maps, nframes, d_frames, hip_stream)); }
    DeltaFrames mcDelta(const void *frames, int nframes, int gop, int range) const { return csic::mcDelta(params_, frames, nframes, gop, range); }
    std::vector<uint8_t> mcUndelta(const void *diff, const void *maps, int nframes, int gop) const { return csic::mcUndelta(params_, diff, maps, nframes, gop); }
    void mcDeltaDevice(const void *d_frames, int nframes, int gop, int range, void *d_diff, void *d_maps, void *d_workspace, size_t workspace_bytes,
                       void *hip_stream)
    {
        check(csic_mc_delta_device(plan_, d_frames, nframes, gop, range, d_diff, d_maps, d_workspace, workspace_bytes, hip_stream));
    }
    void mcUndeltaDevice(const void *d_diff, const void *d_maps, int nframes, int gop, void *d_frames, void *hip_stream)
    {
        check(csic_mc_undelta_device(plan_, d_diff, d_maps, nframes, gop, d_frames, hip_stream));
    }
    const char *mcKernelName() { return csic_mc_kernel_name(plan_); }

private:
    csic_params params_;
    csic_plan *plan_ = nullptr;
};

class ImageCompressorTop {
public:
    ImageCompressorTop(int width, int height, int chroma_param_a_config, int chroma_param_b_config,
                       int yTargetQuantBitsConfig, int cbTargetQuantBitsConfig, int crTargetQuantBitsConfig,
                       int downFactorConfig, ProcessingStep op1Type, ProcessingStep op2Type, ProcessingStep op3Type,
                       Rounding rounding = Rounding::FLOOR_HW, int device = 0)
        : device_(device)
    {
        csic_params_default(&params_, width, height);
        params_.chroma_a = chroma_param_a_config; params_.chroma_b = chroma_param_b_config;
        params_.y_bits = yTargetQuantBitsConfig; params_.cb_bits = cbTargetQuantBitsConfig; params_.cr_bits = crTargetQuantBitsConfig;
        params_.factor = downFactorConfig;
        params_.op[0] = (int32_t)op1Type; params_.op[1] = (int32_t)op2Type; params_.op[2] = (int32_t)op3Type;
        params_.rounding = (int32_t)rounding;
        check(csic_validate(&params_));                       // construction-time require()s
        check(csic_out_dims(&params_, &out_w_, &out_h_));
    }
    ImageCompressorTop(const ImageCompressorTop &) = delete;
    ImageCompressorTop &operator=(const ImageCompressorTop &) = delete;
    virtual ~ImageCompressorTop()
    {
        for (csic_plan *pl : plan_) csic_plan_destroy(pl);
    }

    int outWidth() const { return out_w_; }
    int outHeight() const { return out_h_; }

    // ARGB frame in -> reconstructed ARGB frame out (the DUT output put through YCbCrUtils.ycbcr2rgb,
    // ImageCompressorTopApp.scala:118)
    std::vector<uint32_t> process(const std::vector<uint32_t> &argb) { return run(PixelFormat::ARGB8888, argb); }
    // ARGB frame in -> io.out's PixelYCbCrBundle stream, packed Y | Cb << 8 | Cr << 16
    std::vector<uint32_t> processYCbCr(const std::vector<uint32_t> &argb) { return run(PixelFormat::YCBCR888X, argb); }
    // device-resident, asynchronous on `hip_stream`
    void processDevice(const void *d_in, void *d_out, void *hip_stream, PixelFormat f = PixelFormat::ARGB8888)
    {
        check(csic_process_device(plan(f), d_in, d_out, hip_stream));
    }
    // The subsampled wire format the reference's README describes and its code never builds (README.md:35-46,
    // ChromaSubsampler.scala:57-65): planarLayout() needs no GPU; processPlanar() moves one host frame; on the device,
    // processDevice(..., PixelFormat::PLANAR) writes layout.frame_bytes bytes per frame (256-byte aligned) and
    // reconstructDevice() turns planar frames back into the packed stream -- reconstruct(planar(x)) == process(x).
    csic_planar_layout planarLayout() const
    {
        csic_planar_layout lay;
        check(csic_planar_layout_of(&params_, &lay));
        return lay;
    }
    PlanarFrame processPlanar(const std::vector<uint32_t> &argb)
    {
        PlanarFrame fr;
        fr.layout = planarLayout();
        std::vector<uint32_t> words((size_t)(fr.layout.frame_bytes / 4));
        check(csic_process_host(plan(PixelFormat::PLANAR), argb.data(), argb.size(), words.data(), words.size()));
        fr.bytes.resize((size_t)fr.layout.frame_bytes);
        std::memcpy(fr.bytes.data(), words.data(), fr.bytes.size());
        return fr;
    }
    void reconstructDevice(const void *d_planar, void *d_out, int nframes, void *hip_stream, PixelFormat f = PixelFormat::ARGB8888)
    {
        check(csic_reconstruct_device(plan(PixelFormat::PLANAR), d_planar, d_out, nframes, (int32_t)f, hip_stream));
    }
    // The same planes with every sample at its quantised bit width (CSIC_FMT_PLANAR_BITS): planarBitsLayout() needs no GPU,
    // processPlanarBits() moves one host frame, reconstructBitsDevice() is reconstructDevice() for such frames.
    csic_planar_bits_layout planarBitsLayout() const
    {
        csic_planar_bits_layout lay;
        check(csic_planar_bits_layout_of(&params_, &lay));
        return lay;
    }
    PlanarBitsFrame processPlanarBits(const std::vector<uint32_t> &argb)
    {
        PlanarBitsFrame fr;
        fr.layout = planarBitsLayout();
        std::vector<uint32_t> words((size_t)(fr.layout.frame_bytes / 4));
        check(csic_process_host(plan(PixelFormat::PLANAR_BITS), argb.data(), argb.size(), words.data(), words.size()));
        fr.bytes.resize((size_t)fr.layout.frame_bytes);
        std::memcpy(fr.bytes.data(), words.data(), fr.bytes.size());
        return fr;
    }
    void reconstructBitsDevice(const void *d_bits, void *d_out, int nframes, void *hip_stream, PixelFormat f = PixelFormat::ARGB8888)
    {
        check(csic_reconstruct_bits_device(plan(PixelFormat::PLANAR_BITS), d_bits, d_out, nframes, (int32_t)f, hip_stream));
    }
    // Full-resolution decode (csic_decode_*): a compressed frame -> width x height packed pixels, every pixel of the packed output
    // replicated factor x factor times.  decode() moves `nframes` host frames in `src` format (PLANAR_BITS / PLANAR frame buffers,
    // or the packed YCBCR888X / ARGB8888 output); decodeDevice() is device-resident and asynchronous on `hip_stream`.
    std::vector<uint32_t> decode(const void *src, size_t src_bytes, PixelFormat src_format = PixelFormat::PLANAR_BITS,
                                 PixelFormat f = PixelFormat::ARGB8888, int nframes = 1)
    {
        std::vector<uint32_t> out((size_t)params_.width * (size_t)params_.height * (size_t)(nframes > 0 ? nframes : 0));
        check(csic_decode_host(plan(PixelFormat::ARGB8888), src, src_bytes, (int32_t)src_format, out.data(), out.size(), (int32_t)f, nframes));
        return out;
    }
    std::vector<uint32_t> decode(const PlanarBitsFrame &fr, PixelFormat f = PixelFormat::ARGB8888)
    {
        return decode(fr.bytes.data(), fr.bytes.size(), PixelFormat::PLANAR_BITS, f, 1);
    }
    void decodeDevice(const void *d_src, PixelFormat src_format, void *d_out, int nframes, void *hip_stream, PixelFormat f = PixelFormat::ARGB8888)
    {
        check(csic_decode_device(plan(PixelFormat::ARGB8888), d_src, (int32_t)src_format, d_out, (int32_t)f, nframes, hip_stream));
    }
    const char *decodeKernelName(PixelFormat src_format, PixelFormat f = PixelFormat::ARGB8888)
    {
        return csic_decode_kernel_name(plan(PixelFormat::ARGB8888), (int32_t)src_format, (int32_t)f);
    }
    // View decode (csic_decode_view_*): the window of the decoded frame that starts at (view.x0, view.y0), reduced by a view.scale x
    // view.scale box -- view.width x view.height pixels per frame, each the rounded mean of the decoded pixels under its box.
    std::vector<uint32_t> decodeView(const void *src, size_t src_bytes, const View &view, PixelFormat src_format = PixelFormat::PLANAR_BITS,
                                     PixelFormat f = PixelFormat::ARGB8888, int nframes = 1)
    {
        const bool sized = view.width > 0 && view.height > 0 && nframes > 0;
        std::vector<uint32_t> out(sized ? (size_t)view.width * (size_t)view.height * (size_t)nframes : 1);   // (1: a view without pixels is the library's to refuse)
        check(csic_decode_view_host(plan(PixelFormat::ARGB8888), src, src_bytes, (int32_t)src_format, &view, out.data(), out.size(), (int32_t)f, nframes));
        return out;
    }
    std::vector<uint32_t> decodeView(const PlanarBitsFrame &fr, const View &view, PixelFormat f = PixelFormat::ARGB8888)
    {
        return decodeView(fr.bytes.data(), fr.bytes.size(), view, PixelFormat::PLANAR_BITS, f, 1);
    }
    void decodeViewDevice(const void *d_src, PixelFormat src_format, const View &view, void *d_out, int nframes, void *hip_stream,
                          PixelFormat f = PixelFormat::ARGB8888)
    {
        check(csic_decode_view_device(plan(PixelFormat::ARGB8888), d_src, (int32_t)src_format, &view, d_out, (int32_t)f, nframes, hip_stream));
    }
    const char *decodeViewKernelName(PixelFormat src_format, const View &view, PixelFormat f = PixelFormat::ARGB8888)
    {
        return csic_decode_view_kernel_name(plan(PixelFormat::ARGB8888), (int32_t)src_format, (int32_t)f, &view);
    }
    const csic_params &params() const { return params_; }
    // what row pitch (pixels, input / output) a caller that owns its surfaces should allocate for csic_process_pitched_device
    std::pair<int, int> preferredPitch(PixelFormat f = PixelFormat::ARGB8888)
    {
        int32_t ip = 0, op = 0;
        check(csic_plan_preferred_pitch(plan(f), &ip, &op));
        return {ip, op};
    }
    const char *kernelName(PixelFormat f = PixelFormat::ARGB8888) { return csic_plan_kernel_name(plan(f)); }
    // What these parameters cost in image quality: `nframes` ARGB frames back to back (host memory) -> one Distortion per frame.
    std::vector<Distortion> distortion(const uint32_t *argb, int nframes = 1)
    {
        std::vector<uint64_t> sse((size_t)nframes * CSIC_DIST_CHANNELS);
        const size_t px = (size_t)params_.width * (size_t)params_.height;
        check(csic_distortion_host(plan(PixelFormat::ARGB8888), argb, px * (size_t)(nframes > 0 ? nframes : 0), nframes, sse.data()));
        return toDistortion(sse, nframes);
    }
    // device-resident: d_in holds `nframes` frames, d_sse receives nframes * 6 sums (8-byte aligned), d_workspace at least
    // distortionWorkspaceBytes(nframes) bytes; asynchronous on `hip_stream`, no allocation, capturable.
    size_t distortionWorkspaceBytes(int nframes = 1)
    {
        size_t b = 0;
        check(csic_distortion_workspace_bytes(plan(PixelFormat::ARGB8888), nframes, &b));
        return b;
    }
    void distortionDevice(const void *d_in, int nframes, uint64_t *d_sse, void *d_workspace, size_t workspace_bytes, void *hip_stream)
    {
        check(csic_distortion_device(plan(PixelFormat::ARGB8888), d_in, nframes, d_sse, d_workspace, workspace_bytes, hip_stream));
    }
    // the sums of distortionDevice, copied to the host by the caller -> one Distortion per frame
    std::vector<Distortion> toDistortion(const std::vector<uint64_t> &sse, int nframes) const
    {
        std::vector<Distortion> out((size_t)(nframes > 0 ? nframes : 0));
        for (size_t k = 0; k < out.size(); ++k) {
            for (int c = 0; c < CSIC_DIST_CHANNELS; ++c) out[k].sse[c] = sse[k * CSIC_DIST_CHANNELS + (size_t)c];
            out[k].pixels = (int64_t)params_.width * params_.height;
        }
        return out;
    }
    // How much of the structure of `nframes` ARGB frames back to back (host memory) these parameters keep: one Ssim per frame,
    // with the per-window map if `want_map`.
    std::vector<Ssim> ssim(const uint32_t *argb, int nframes = 1, bool want_map = false)
    {
        const size_t n = (size_t)(nframes > 0 ? nframes : 0), px = (size_t)params_.width * (size_t)params_.height;
        const size_t windows = (size_t)(params_.width / CSIC_SSIM_WINDOW) * (size_t)(params_.height / CSIC_SSIM_WINDOW);
        std::vector<int64_t> sums(n * CSIC_DIST_CHANNELS);
        std::vector<int32_t> map(want_map ? n * CSIC_DIST_CHANNELS * windows : 0);
        check(csic_ssim_host(plan(PixelFormat::ARGB8888), argb, px * n, nframes, sums.data(), want_map ? map.data() : nullptr));
        std::vector<Ssim> out(n);
        for (size_t k = 0; k < n; ++k) {
            for (int c = 0; c < CSIC_DIST_CHANNELS; ++c) out[k].sums[c] = sums[k * CSIC_DIST_CHANNELS + (size_t)c];
            out[k].windows = (int64_t)windows;
            if (want_map) out[k].map.assign(map.begin() + (ptrdiff_t)(k * CSIC_DIST_CHANNELS * windows), map.begin() + (ptrdiff_t)((k + 1) * CSIC_DIST_CHANNELS * windows));
        }
        return out;
    }
    // device-resident: d_in holds `nframes` frames, d_ssim receives nframes * 6 sums (8-byte aligned), d_map (or NULL) the
    // quotients, d_workspace at least ssimWorkspaceBytes(nframes) bytes; asynchronous on `hip_stream`, no allocation, capturable.
    size_t ssimWorkspaceBytes(int nframes = 1)
    {
        size_t b = 0;
        check(csic_ssim_workspace_bytes(plan(PixelFormat::ARGB8888), nframes, &b));
        return b;
    }
    void ssimDevice(const void *d_in, int nframes, int64_t *d_ssim, int32_t *d_map, void *d_workspace, size_t workspace_bytes, void *hip_stream)
    {
        check(csic_ssim_device(plan(PixelFormat::ARGB8888), d_in, nframes, d_ssim, d_map, d_workspace, workspace_bytes, hip_stream));
    }
    const char *ssimKernelName() { return csic_ssim_kernel_name(plan(PixelFormat::ARGB8888)); }
    // Rate and distortion of every (y, cb, cr) bit set of these parameters in one pass (csic.h: csic_qsweep_*): `nframes` ARGB frames
    // back to back (host memory) -> one csic_qsweep_result per frame; csic::qsweepRank ranks them.  The three bit widths this object
    // was built with do not matter.
    std::vector<csic_qsweep_result> qsweep(const uint32_t *argb, int nframes = 1)
    {
        std::vector<csic_qsweep_result> out((size_t)(nframes > 0 ? nframes : 0));
        const size_t px = (size_t)params_.width * (size_t)params_.height;
        check(csic_qsweep_host(plan(PixelFormat::ARGB8888), argb, px * out.size(), nframes, out.data()));
        return out;
    }
    // device-resident: d_result receives nframes results (8-byte aligned), d_workspace (256-byte aligned) at least
    // qsweepWorkspaceBytes(nframes) bytes; asynchronous on `hip_stream`, no allocation, capturable.
    size_t qsweepWorkspaceBytes(int nframes = 1)
    {
        size_t b = 0;
        check(csic_qsweep_workspace_bytes(plan(PixelFormat::ARGB8888), nframes, &b));
        return b;
    }
    void qsweepDevice(const void *d_in, int nframes, csic_qsweep_result *d_result, void *d_workspace, size_t workspace_bytes, void *hip_stream)
    {
        check(csic_qsweep_device(plan(PixelFormat::ARGB8888), d_in, nframes, d_result, d_workspace, workspace_bytes, hip_stream));
    }
    const char *qsweepKernelName() { return csic_qsweep_kernel_name(plan(PixelFormat::ARGB8888)); }
    // What the samples of an ARGB frame's compressed form really carry: compresses to bit-packed planes, then measures them
    // (csic_code_stats_*), host memory in, CodeStats out.
    CodeStats codeStats(const std::vector<uint32_t> &argb)
    {
        const PlanarBitsFrame fr = processPlanarBits(argb);
        CodeStats out;
        check(csic_code_stats_host(plan(PixelFormat::PLANAR_BITS), fr.bytes.data(), fr.bytes.size(), CSIC_FMT_PLANAR_BITS, 1, &out.hist[0][0][0]));
        out.bits[0] = params_.y_bits; out.bits[1] = params_.cb_bits; out.bits[2] = params_.cr_bits;
        out.pixels = (int64_t)params_.width * params_.height;
        return out;
    }
    const char *codeStatsKernelName(PixelFormat src_format = PixelFormat::PLANAR_BITS)
    {
        return csic_code_stats_kernel_name(plan(PixelFormat::PLANAR_BITS), (int32_t)src_format);
    }
    // the plan behind process(): what FrameGraph records launches of (owned by this object)
    csic_plan *nativePlan(PixelFormat f = PixelFormat::ARGB8888) { return plan(f); }

private:
    csic_plan *plan(PixelFormat f)
    {
        csic_plan *&pl = plan_[(int)f];
        if (!pl) {
            csic_params p = params_;
            p.out_format = (int32_t)f;
            check(csic_plan_create(&p, device_, &pl));
        }
        return pl;
    }
    std::vector<uint32_t> run(PixelFormat f, const std::vector<uint32_t> &argb)
    {
        std::vector<uint32_t> out((size_t)out_w_ * out_h_);
        check(csic_process_host(plan(f), argb.data(), argb.size(), out.data(), out.size()));
        return out;
    }
    csic_params params_{};
    csic_plan *plan_[4] = {nullptr, nullptr, nullptr, nullptr};     // one per PixelFormat
    int32_t out_w_ = 0, out_h_ = 0;
    int device_;
};

// Pre-recorded per-frame launches (csic_frame_graph_*): frames in separate device buffers, recorded once and replayed
// so that small launches overlap.  HIP = hipGraph chains ordered with the caller's stream; DIRECT = AQL packets without
// barrier bits on the library's own queues -- launch(stream) orders them with a HIP stream on the device, submit()/wait()
// by the host.  The reference processes one image at a time (ImageCompressorTopApp.scala:53-68).
enum class FrameGraphBackend : int32_t { HIP = CSIC_FRAME_GRAPH_HIP, DIRECT = CSIC_FRAME_GRAPH_DIRECT, FUSED = CSIC_FRAME_GRAPH_FUSED,
                                         AUTO = CSIC_FRAME_GRAPH_AUTO };

class FrameGraph {
public:
    FrameGraph(csic_plan *plan, const std::vector<const void *> &d_in, const std::vector<void *> &d_out,
               FrameGraphBackend backend = FrameGraphBackend::AUTO, int branches = 0)
    {
        if (d_in.size() != d_out.size() || d_in.empty())
            throw IllegalArgumentException(CSIC_EINVAL_SIZE, "need as many output as input frames (> 0)");
        check(csic_frame_graph_create_ex(plan, d_in.data(), d_out.data(), (int32_t)d_in.size(), branches, (int32_t)backend, &g_));
    }
    FrameGraph(const FrameGraph &) = delete;
    FrameGraph &operator=(const FrameGraph &) = delete;
    ~FrameGraph() { csic_frame_graph_destroy(g_); }
    void launch(void *hip_stream) { check(csic_frame_graph_launch(g_, hip_stream)); }
    int64_t submit() { int64_t t = 0; check(csic_frame_graph_submit(g_, &t)); return t; }
    void wait(int64_t ticket = -1) { check(csic_frame_graph_wait(g_, ticket)); }
    bool streamOrdered() const { return csic_frame_graph_stream_ordered(g_) == 1; }
    int branches() const { int32_t n = 0, b = 0; csic_frame_graph_count(g_, &n, &b); return b; }
    int launchBranches() const { return csic_frame_graph_launch_branches(g_); }
    FrameGraphBackend backend() const { return (FrameGraphBackend)csic_frame_graph_backend(g_); }   // the resolved one, never AUTO

private:
    csic_frame_graph *g_ = nullptr;
};

// Cycle-level model of the Decoupled pixel stream (csic_stream_*): the generated hardware's ready/valid interface, one clock
// edge per step() -- chiseltest's poke / peek / step on the reference's modules (SpatialDownsamplerSpec.scala:48-58).  Host only;
// a simulator of interface timing, never a compute path.
class StreamModel {
public:
    StreamModel(const csic_params &p, int32_t kind) { check(csic_stream_create(&p, kind, &s_)); }
    StreamModel(const StreamModel &) = delete;
    StreamModel &operator=(const StreamModel &) = delete;
    ~StreamModel() { csic_stream_destroy(s_); }
    csic_stream_in in{0, 0, 0, 0, 0};                                       // poked inputs hold their value (un-poked: 0)
    csic_stream_out peek() const { csic_stream_out o; check(csic_stream_eval(s_, &in, &o)); return o; }
    csic_stream_out step() { csic_stream_out o; check(csic_stream_step(s_, &in, &o)); return o; }
    void reset() { check(csic_stream_reset(s_)); in = csic_stream_in{0, 0, 0, 0, 0}; }
    int64_t cycles() const { return csic_stream_cycles(s_); }
    // the app's driver + collector loops (ImageCompressorTopApp.scala:76-124); max_cycles < 0 = until drained
    std::vector<uint32_t> run(const std::vector<uint32_t> &pixels, size_t max_out, int64_t max_cycles = -1, int64_t *cycles_used = nullptr)
    {
        std::vector<uint32_t> out(max_out ? max_out : 1);
        size_t n = 0;
        check(csic_stream_run(s_, pixels.data(), pixels.size(), out.data(), max_out, max_cycles, nullptr, 0, nullptr, 0, &n, cycles_used));
        out.resize(n);
        return out;
    }

private:
    csic_stream *s_ = nullptr;
};

class ImageProcessor : public ImageCompressorTop {
public:
    explicit ImageProcessor(const ImageProcessorParams &p, Rounding rounding = Rounding::FLOOR_HW, int device = 0)
        : ImageCompressorTop(p.width, p.height, p.chromaParamA, p.chromaParamB, 8, 8, 8, p.factor,
                             ProcessingStep::ChromaSubsampling, ProcessingStep::SpatialSampling,
                             ProcessingStep::ColorQuantization, rounding, device) {}
};

} // namespace csic
