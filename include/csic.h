/*
 * csic.h -- C ABI of libcsic_hip.so: the MI355X (gfx950) implementation of the reference's
 * pixel-stream hot path
 *
 *     RGB2YCbCr -> {ChromaSubsampler, SpatialDownsampler, ColorQuantizer in any order} -> YCbCr2RGB
 *
 * The reference (Scala/Chisel, /root/reference) has no FFI: its "interface" for this path is the
 * generator surface -- constructor parameter lists and require()s.  Each entry point below names the
 * reference interface it stands in for (paths relative to /root/reference/).  INTEGRATION.md shows the
 * JNI / Panama binding a maintainer of the reference would add on the Scala side.
 *
 * Conventions: plain C, no C++ types, no exceptions across the boundary.  Every function returning
 * `int` returns CSIC_OK (0) or a negative csic_status; a human-readable message for the calling
 * thread's last failure is available from csic_last_error().  The caller owns every pixel buffer; the
 * library owns only the opaque plan.  A plan is not thread-safe; distinct plans are independent.
 * There is NO CPU fallback: compute entry points fail with CSIC_ENODEVICE when no HIP device exists.
 *
 * Pixel layout (one uint32 per pixel, little endian):
 *   CSIC_FMT_ARGB8888 : byte0=B byte1=G byte2=R byte3=A  == Java `int` ARGB, what scrimage /
 *                       BufferedImage hand out (ImageProcessorModel.scala:47-48).  Input alpha is
 *                       ignored; output alpha is 255 (ImageCompressorTopApp.scala:139).
 *   CSIC_FMT_YCBCR888X: byte0=Y byte1=Cb byte2=Cr byte3=0 -- the PixelYCbCrBundle that
 *                       ImageCompressorTop.io.out carries (ImageCompressorTop.scala:35,
 *                       PixelBundle.scala:11-15), i.e. the pipeline WITHOUT the host-side inverse.  As
 *                       in_format it feeds a YCbCr stream straight into op1 (forward transform skipped):
 *                       how the reference's specs drive ONE stage (ChromaSubsamplerImageSpec.scala:150-170,
 *                       ColorQuantizerSpec.scala:72-100, SpatialDownsamplerSpec.scala:20-45).
 * Frames are row-major, tightly packed (row pitch = width * 4 bytes).
 */
#ifndef CSIC_H
#define CSIC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSIC_ABI_VERSION 1

/* ---- status codes ------------------------------------------------------------------------------
 * Every CSIC_EINVAL_* corresponds to a require() that throws IllegalArgumentException when the
 * reference's generator is constructed; a host binding maps them to IllegalArgumentException. */
typedef enum csic_status {
    CSIC_OK                     =   0,
    CSIC_EINVAL_NULL            =  -1, /* null pointer argument                                       */
    CSIC_EINVAL_DIMS            =  -2, /* ImageProcessor.scala:22-23, ChromaSubsampler.scala:13-14     */
    CSIC_EINVAL_FACTOR          =  -3, /* ImageProcessor.scala:24, SpatialDownsampler.scala:8          */
    CSIC_EINVAL_CHROMA_A        =  -4, /* ImageProcessor.scala:27, ChromaSubsampler.scala:17           */
    CSIC_EINVAL_CHROMA_B        =  -5, /* ImageProcessor.scala:28, ChromaSubsampler.scala:18           */
    CSIC_EINVAL_BITS            =  -6, /* ColorQuantizer.scala:12-15                                   */
    CSIC_EINVAL_OP_PERMUTATION  =  -7, /* ImageCompressorTop.scala:27-31                               */
    CSIC_EINVAL_ROUNDING        =  -8,
    CSIC_EINVAL_FORMAT          =  -9,
    CSIC_EINVAL_NOT_DIVISIBLE   = -10, /* ImageProcessor.scala:25 (only when strict_divisible != 0)    */
    CSIC_EINVAL_SAMPLING        = -11,
    CSIC_EINVAL_STRIPE          = -12, /* row-stripe request that cannot be made independent           */
    CSIC_EINVAL_SIZE            = -13, /* buffer size does not match the plan                          */
    CSIC_ENODEVICE              = -20, /* no HIP device / bad device ordinal                           */
    CSIC_EHIP                   = -21, /* a HIP runtime call failed (message has the HIP error string) */
    CSIC_ENOMEM                 = -22,
    CSIC_ECAPTURE               = -23, /* the HIP stream is capturing and this operation cannot be captured */
    CSIC_EIO                    = -30, /* file cannot be opened / read / written                       */
    CSIC_EFORMAT                = -31  /* not a PNG / .csic file, corrupt, or an unsupported feature   */
} csic_status;

/* ---- enumerations -------------------------------------------------------------------------------*/
/* ProcessingStep ordinals, ImageCompressorTop.scala:7-9 */
#define CSIC_OP_NOOP      0
#define CSIC_OP_SPATIAL   1   /* ProcessingStep.SpatialSampling   */
#define CSIC_OP_QUANT     2   /* ProcessingStep.ColorQuantization */
#define CSIC_OP_CHROMA    3   /* ProcessingStep.ChromaSubsampling */

/* Forward-transform rounding: both exist in the reference and both are pinned by
 * committed golden images. */
#define CSIC_ROUND_FLOOR_HW 0 /* RTL + ReferenceModel: (x+128) >> 8     RGB2YCbCr.scala:50-65       */
#define CSIC_ROUND_TRUNC_SW 1 /* YCbCrUtils.rgbToYCbCr: (x+128) / 256   RGB2YCbCr.scala:111-118     */

/* Sampling semantics.
 * HOLD_DECIMATE (default) is the reference's: chroma sample-and-hold (ChromaSubsampler.scala:47-65) and
 *   top-left decimation (SpatialDownsampler.scala:33-55).  Everything "bit-exact" refers to this mode.
 * AVG is an EXTENSION with no counterpart in the reference code (its README and the project brief describe
 *   it): box-filter chroma over h x v blocks, then f x f average pooling, each (sum + n/2) >> log2 n on 8-bit
 *   values, edge coordinates clamped; defined for op = {CHROMA, SPATIAL, QUANT} only.  Its normative
 *   statement is oracle/csic_oracle.c:orc_process_avg; it has no reference parity by construction. */
#define CSIC_SAMPLING_HOLD_DECIMATE 0
#define CSIC_SAMPLING_AVG           1

#define CSIC_FMT_ARGB8888  0
#define CSIC_FMT_YCBCR888X 1
#define CSIC_FMT_PLANAR    2   /* out_format only: Y plane + Cb / Cr planes at the chroma sample points (csic_planar_layout) */
#define CSIC_FMT_PLANAR_BITS 3 /* out_format only, ARGB input only: the same planes, each sample at its quantised bit width (csic_planar_bits_layout) */

/* ---- parameters ---------------------------------------------------------------------------------
 * Field-for-field the constructor list of
 *   class ImageCompressorTop(width, height, chroma_param_a_config, chroma_param_b_config,
 *                            yTargetQuantBitsConfig, cbTargetQuantBitsConfig, crTargetQuantBitsConfig,
 *                            downFactorConfig, op1Type, op2Type, op3Type)   ImageCompressorTop.scala:11-25
 * (ImageProcessorParams, ImageProcessor.scala:15-21, is the subset width/height/factor/a/b with
 * bits = 8,8,8, op = {CHROMA, SPATIAL, QUANT} and strict_divisible = 1.) */
typedef struct csic_params {
    int32_t width, height;
    int32_t chroma_a, chroma_b;          /* J:a:b with J = 4: a in {4,2,1}, b in {a,0}                */
    int32_t y_bits, cb_bits, cr_bits;    /* 1..8 significant bits kept per channel                    */
    int32_t factor;                      /* spatial decimation factor 1,2,4,8                         */
    int32_t op[3];                       /* permutation of CSIC_OP_{SPATIAL,QUANT,CHROMA}             */
    int32_t rounding;                    /* CSIC_ROUND_*                                              */
    int32_t sampling;                    /* CSIC_SAMPLING_HOLD_DECIMATE (reference) or CSIC_SAMPLING_AVG  */
    int32_t in_format, out_format;       /* CSIC_FMT_* (CSIC_FMT_PLANAR: out_format only)             */
    int32_t strict_divisible;            /* 1 = enforce ImageProcessorParams' divisibility require()  */
} csic_params;

typedef struct csic_plan csic_plan;      /* opaque */

/* ---- host-only logic (usable without a GPU) -----------------------------------------------------*/
int  csic_abi_version(void);

/* Fills *p with 4:4:4, 8/8/8 bits, factor 1, order chroma->spatial->quant (the north-star order),
 * FLOOR_HW rounding, ARGB in/out, non-strict.  Mirrors ImageProcessorModel.getImageParams
 * (ImageProcessorModel.scala:33-41), which defaults chroma to 4:4:4. */
int  csic_params_default(csic_params *p, int32_t width, int32_t height);

/* All the reference's require()s in one call (see csic_status).  Replaces the construction-time checks
 * of ImageProcessorParams / ChromaSubsampler / SpatialDownsampler / ColorQuantizer / ImageCompressorTop. */
int  csic_validate(const csic_params *p);

/* Output frame size: ceil(W/f) x ceil(H/f) -- what SpatialDownsampler emits
 * (SpatialDownsampler.scala:33-55; 5x3,f=2 -> 3x2, SpatialDownsamplerSpec.scala:120-122). */
int  csic_out_dims(const csic_params *p, int32_t *out_width, int32_t *out_height);

/* Algorithmic HBM bytes of one frame, the roofline numerator of SURVEY.md 8(d):
 *   A = 4*W*ceil(H/f) + 4*ceil(W/f)*ceil(H/f)
 * (every input row that holds a surviving pixel, plus the output; rows r % f != 0 are dead).
 * With CSIC_SAMPLING_AVG every row is live: A = 4*W*H + 4*ceil(W/f)*ceil(H/f). */
int  csic_algorithmic_bytes(const csic_params *p, int64_t *bytes);

/* Row-stripe partition for `nranks` devices.  Stripe boundaries are aligned to
 * L = lcm(v, f) input rows (chroma before spatial) or v*f*f rows (spatial before chroma), which makes
 * every stripe an independent image of height *nrows: no halo, no collective.  Fails with
 * CSIC_EINVAL_STRIPE when the order class/shape cannot be split independently (spatial-before-chroma
 * with width % factor != 0).  Empty stripes (nrows == 0) are possible when nranks exceeds the number
 * of aligned row blocks. */
int  csic_stripe_rows(const csic_params *p, int32_t nranks, int32_t rank,
                      int32_t *row0, int32_t *nrows, int32_t *out_row0, int32_t *out_nrows);

/* Halo plan for stripes that are ALREADY partitioned at arbitrary rows (row_splits[0..nranks], with
 * row_splits[0] = 0 and row_splits[nranks] = height): rank r holds input rows [row_splits[r], row_splits[r+1]).
 * Every rank processes whole aligned L-row blocks [*proc_row0, *proc_row0 + *proc_nrows): it RECEIVES the
 * *halo_above = row_splits[r] - *proc_row0 rows in front of its stripe from rank r-1 and SENDS its trailing
 * *tail_below rows (those past its last aligned boundary) to rank r+1 -- one neighbour exchange of fewer than
 * L rows (the north star's "single RCCL halo exchange"; L as in csic_stripe_rows).  The processed range is an
 * independent image; its output rows are [*out_row0, *out_row0 + *out_nrows).  Fails with
 * CSIC_EINVAL_STRIPE if a stripe is shorter than the halo its successor needs. */
int  csic_stripe_halo(const csic_params *p, int32_t nranks, int32_t rank, const int32_t *row_splits,
                      int32_t *proc_row0, int32_t *proc_nrows, int32_t *halo_above, int32_t *tail_below,
                      int32_t *out_row0, int32_t *out_nrows);

/* ---- planar, genuinely subsampled output (out_format = CSIC_FMT_PLANAR) ------------------------------------------
 * Every packed output of the path is 4 bytes per pixel whatever the chroma mode: ChromaSubsampler re-emits the held Cb / Cr
 * with every pixel (ChromaSubsampler.scala:57-65), so nothing the reference produces is smaller than its input -- its README
 * describes the subsampled wire format (README.md:35-46), its code never builds it.  This format
 * stores each value the stream really carries ONCE: a Y plane with one byte per output pixel and two chroma planes with one
 * byte per chroma SAMPLE POINT.  4:2:0 at factor 1: 1.5 bytes per pixel instead of 4.
 *
 * Definition, on the output stream o[j], j = 0 .. n-1 (n = out_width * out_height, row-major), with the chroma stage's
 * counters as the output sees them -- c = j mod module_width, r = j div module_width:
 *     position j is a sample point  <=>  c % hold_h == 0  and  r % hold_v == 0
 *     sample index  k(j) = (r / hold_v) * chroma_width + c / hold_h,     chroma_width = ceil(module_width / hold_h)
 *     Y[j] = o[j].Y for every j;     Cb[k(j)] = o[j].Cb,  Cr[k(j)] = o[j].Cr  for every sample point j
 *   (module_width, hold_h, hold_v) follow from where the chroma stage sits:
 *     chroma before spatial, factor 1 : (W,  h, v)               -- the image's own 4:a:b grid
 *     chroma before spatial, factor f : (Wo, max(1, h / f), 1)   -- decimation keeps every f-th column of the held stream
 *     spatial before chroma           : (W,  h, v) over the DECIMATED stream: the chroma counters wrap at the FULL width
 *                                       (ImageCompressorTop.scala:52-58), so one chroma row spans f decimated rows and the
 *                                       last one may be partial (chroma_samples < chroma_width * chroma_height)
 *     CSIC_SAMPLING_AVG               : (Wo, max(1, h / f), max(1, v / f)), replay_last = 0
 * Values are what the packed YCbCr output holds at those positions (after the quantiser, in either rounding).
 *
 * csic_reconstruct_device is the inverse: planar -> packed ARGB (through YCbCrUtils.ycbcr2rgb, as the reference's harness
 * does per pixel, ImageCompressorTopApp.scala:118) or packed YCbCr.  Position j takes Y[j] and the chroma sample
 *     k(j)                                                      on rows r % hold_v == 0 (c / hold_h floors),
 *     ((r - 1) / hold_v) * chroma_width + chroma_width - 1      on the other rows when replay_last = 1: the reference's
 *                                                               4:x:0 hold replays the LAST sample of the row above for a
 *                                                               whole row (ChromaSubsampler.scala:52-65),
 *     (r / hold_v) * chroma_width + c / hold_h                  on the other rows when replay_last = 0 (AVG: plain box).
 * For every parameter set  reconstruct(planar(x)) == the packed output of the same parameters, bit for bit: under
 * HOLD_DECIMATE that pins the planar path to the reference exactly as far as the packed path is pinned; under AVG to
 * oracle/csic_oracle.c:orc_process_avg -- no reference parity by construction.
 *
 * Buffer: ONE allocation per frame, planes at 256-byte aligned offsets; frame k of a batch at k * frame_bytes.  Planes are
 * tightly packed (no row padding).  Bytes of a chroma plane beyond chroma_samples are never written. */
typedef struct csic_planar_layout {
    int32_t y_width, y_height;            /* = csic_out_dims                                                        */
    int32_t chroma_width, chroma_height;  /* samples per chroma row, chroma rows                                    */
    int32_t module_width;                 /* row length of the chroma counters over the output stream               */
    int32_t hold_h, hold_v;               /* one sample per hold_h positions, on every hold_v-th chroma row          */
    int32_t replay_last;                  /* 1: rows without samples replay the last sample of the row above (HOLD)  */
    int64_t chroma_samples;               /* samples per chroma plane that carry data                               */
    int64_t y_offset, cb_offset, cr_offset; /* byte offsets of the planes inside a frame's buffer                   */
    int64_t frame_bytes;                  /* bytes per frame buffer (multiple of 256)                               */
    int64_t payload_bytes;                /* y_width * y_height + 2 * chroma_samples: what the format really stores */
} csic_planar_layout;
/* usable without a GPU; p->out_format need not be CSIC_FMT_PLANAR (the layout of "these parameters, planar") */
int  csic_planar_layout_of(const csic_params *p, csic_planar_layout *layout);

/* ---- bit-packed planar output (out_format = CSIC_FMT_PLANAR_BITS) -------------------------------------------------------
 * CSIC_FMT_PLANAR stores 8 bits per sample although the quantiser keeps only the top y_bits / cb_bits / cr_bits of each channel
 * (ColorQuantizer.scala:40-44): 3 to 6 of those bits are always zero for the reference's Q16bit (6/5/5) and Q8bit (3/3/2).  This
 * format stores each sample at its quantised width.  Sample geometry is exactly csic_planar_layout_of's (module_width, hold_h,
 * hold_v, k(j), replay_last, chroma_samples); only the storage of each plane changes.  Valid as out_format only, and only with
 * in_format = CSIC_FMT_ARGB8888 (csic_validate: CSIC_EINVAL_FORMAT otherwise).
 *
 * A plane with q bits per sample (q = y_bits, cb_bits or cr_bits): sample i of value v stores its code c = v >> (8 - q) at bit
 * positions [i*q, i*q + q) of the plane; bit position b is bit b % 8 of byte b / 8 (LSB first, little endian: a dword read at byte
 * 4m holds bits [32m, 32m + 32) in their natural order, and 32 samples fill exactly q dwords).  The unused high bits of a plane's
 * last byte are 0.  Reconstruct expands c << (8 - q).  Worked vectors:
 *     q = 3, codes 1,2,3,4,5,6,7,0  -> bytes d1 58 1f          q = 5, codes 0x1f, 0, 0x15 -> bytes 1f 54
 * Lossless with respect to the packed output for every valid parameter set: under HOLD_DECIMATE every stage after the quantiser
 * only copies values, and AVG is defined for the order chroma, spatial, quant only, so the quantiser runs last.
 *
 * Layout, with up(x) = x rounded up to 256 and B(s, q) = ceil(s * q / 8), n = y_width * y_height:
 *     y_offset = 0,  cb_offset = up(B(n, y_bits)),  cr_offset = cb_offset + up(B(chroma_width * chroma_height, cb_bits)),
 *     frame_bytes = cr_offset + up(B(chroma_width * chroma_height, cr_bits)),
 *     payload_bytes = B(n, y_bits) + B(chroma_samples, cb_bits) + B(chroma_samples, cr_bits)
 * (y_bytes, cb_bytes, cr_bytes = the three B terms of payload_bytes).  At 8/8/8 every offset, frame_bytes and payload_bytes equal
 * csic_planar_layout's and the frame is byte-identical to a CSIC_FMT_PLANAR frame.  Bytes between a plane's last byte and the next
 * offset are never written.
 *
 * csic_process_device / csic_process_batch_device / csic_process_host and csic_pipeline_* take such a plan: d_out is a 256-byte
 * aligned buffer of frame_bytes per frame.  Row pitches, every frame-graph backend (FUSED included), the file pools, csic_multi_*
 * and csic_stream_create refuse it with CSIC_EINVAL_FORMAT.  csic_reconstruct_bits_device is csic_reconstruct_device for these
 * frames: `nframes` bit-packed frames of `plan`'s parameters (any out_format) -> packed ARGB8888 or YCBCR888X, the same replay
 * rule, asynchronous, no allocation, capturable. */
typedef struct csic_planar_bits_layout {
    csic_planar_layout geometry;          /* csic_planar_layout_of of the same parameters (its offsets / sizes are PLANAR's)     */
    int32_t y_bits, cb_bits, cr_bits, reserved;
    int64_t y_bytes, cb_bytes, cr_bytes;  /* bytes each plane's samples occupy: B(n, y_bits), B(chroma_samples, cb / cr_bits)  */
    int64_t y_offset, cb_offset, cr_offset; /* byte offsets of the planes inside a frame's buffer                               */
    int64_t frame_bytes;                  /* bytes per frame buffer (multiple of 256)                                           */
    int64_t payload_bytes;                /* y_bytes + cb_bytes + cr_bytes                                                      */
} csic_planar_bits_layout;
/* usable without a GPU; p->out_format need not be CSIC_FMT_PLANAR_BITS */
int  csic_planar_bits_layout_of(const csic_params *p, csic_planar_bits_layout *layout);

/* ---- distortion: what a parameter set costs in image quality -------------------------------------------------------------
 * For a plan with parameters p and one input frame x (width x height pixels in p.in_format, frames back to back as for
 * csic_process_batch_device):
 *   o_rgb = the packed output of p with out_format = CSIC_FMT_ARGB8888, o_ycc = the packed output with CSIC_FMT_YCBCR888X
 *   (out_width x out_height each).  The plan's own out_format does not matter: PLANAR and PLANAR_BITS are lossless with respect
 *   to the packed output.
 *   Input pixel (r, c) is paired with output pixel (r / f, c / f) (integer division, the plan's factor f): replication
 *   upsampling.  Every input pixel is counted exactly once, ragged edges included, for every order class and for AVG.
 *   RGB reference of an input pixel: its R, G, B bytes (ARGB input; alpha ignored), or YCbCrUtils.ycbcr2rgb of its Y, Cb, Cr
 *   (YCbCr input; the inverse the packed ARGB output uses).
 *   YCbCr reference: the forward transform under the plan's rounding (ARGB input), or its own Y, Cb, Cr bytes (YCbCr input).
 *   Six sums per frame, uint64, in the order R, G, B, Y, Cb, Cr: sse_k = sum over the width * height input pixels of
 *   (reference_k - output_k)^2, against o_rgb for R, G, B and o_ycc for Y, Cb, Cr.  Integer sums: exact and bit-reproducible.
 *   PSNR (host layers): 10 log10(255^2 * W * H / sse_k), +inf when sse_k = 0; combined RGB: 10 log10(255^2 * 3 W H / (sse_R +
 *   sse_G + sse_B)).
 *
 * csic_distortion_workspace_bytes : the workspace csic_distortion_device needs for `nframes` (1..65535) frames of this plan (one
 *                                   48-byte partial per block; the answer depends on the kernel the plan selects, so query it
 *                                   again after csic_plan_tune).  Needs no device.
 * csic_distortion_device          : d_in -> d_sse[nframes * 6] (8-byte aligned), through d_workspace (8-byte aligned, at least the
 *                                   queried size, else CSIC_EINVAL_SIZE).  Asynchronous on `hip_stream`, no allocation, no
 *                                   synchronisation, hipGraph-capturable; NULL arguments fail with CSIC_EINVAL_NULL before any
 *                                   device is touched.  16-byte loads when d_in is 16-byte aligned, 4-byte loads otherwise
 *                                   (and under CSIC_TUNE_NO_VECTOR).
 * csic_distortion_host            : the same from host memory (in_px = nframes * width * height) into sse[nframes * 6];
 *                                   synchronous, allocates its staging.
 * csic_distortion_kernel_name     : the kernel csic_distortion_device takes for a 16-byte aligned d_in (static string). */
#define CSIC_DIST_CHANNELS 6   /* R, G, B, Y, Cb, Cr */
int  csic_distortion_workspace_bytes(const csic_plan *plan, int32_t nframes, size_t *bytes);
int  csic_distortion_device(csic_plan *plan, const void *d_in, int32_t nframes, uint64_t *d_sse,
                            void *d_workspace, size_t workspace_bytes, void *hip_stream);
int  csic_distortion_host(csic_plan *plan, const uint32_t *in, size_t in_px, int32_t nframes, uint64_t *sse);
const char *csic_distortion_kernel_name(const csic_plan *plan);

/* ---- structural similarity: 8 x 8 block SSIM, in integers ---------------------------------------------------------------------
 * Channels and pairing are exactly those of csic_distortion_*: the reference value of an input pixel in R, G, B, Y, Cb, Cr against
 * the paired output pixel (r / f, c / f) of o_rgb (R, G, B) and of o_ycc (Y, Cb, Cr); any in_format, every order, HOLD_DECIMATE
 * and AVG; the plan's own out_format does not matter.
 *
 * Windows: non-overlapping 8 x 8 blocks of input pixels with their top-left corner at (8 wy, 8 wx), wy < height / 8, wx < width / 8
 * (integer division).  Pixels beyond the last whole window are not measured; a frame with width < 8 or height < 8 has no window and
 * is refused with CSIC_EINVAL_DIMS.  f divides 8, so a window covers whole f x f replication cells.
 *
 * Per window and channel, with x the 64 reference values and y the 64 paired output values:
 *     s1 = sum x    s2 = sum y    ss = sum x^2 + sum y^2    s12 = sum xy
 *     vars  = 64 ss  - s1^2 - s2^2
 *     covar = 64 s12 - s1 s2
 *     c1 = 416      (= floor(0.01^2 255^2 64 + 0.5))
 *     c2 = 235963   (= floor(0.03^2 255^2 64 63 + 0.5))
 *     N = (2 s1 s2 + c1) (2 covar + c2)          signed 64-bit; |N| <= 7.2e16
 *     D = (s1^2 + s2^2 + c1) (vars + c2)         98 160 608 <= D <= 7.2e16
 *     q = sign(N) floor(64 |N| / floor(D / 1024))      SSIM in 16.16 fixed point, rounded toward zero
 * The constants and the 64 sum - s^2 form are the customary integer 8 x 8 SSIM; only the final quotient is pinned to integers here,
 * so that the GPU, numpy and any other host agree bit for bit.  Properties: 64 |N| < 2^63; |N| <= D, hence |q| <= 65536; q = 65536
 * exactly when x = y; |q / 65536 - N / D| < 2.6e-5 (1 / 65536 from the floor plus at most 1.05e-5 relative from truncating D, since
 * floor(D / 1024) >= 95 859).
 *
 * Outputs: d_ssim[nframes * 6], int64, the sum of q over the frame's windows in the order R, G, B, Y, Cb, Cr.  The mean SSIM of a
 * channel is sum / (65536 (width / 8) (height / 8)) and the combined RGB figure the mean of the three channel means (host layers).
 * d_map, which may be NULL: int32 [frame][channel][height / 8][width / 8], each entry that window's q -- where the loss is.
 *
 * csic_ssim_workspace_bytes : the workspace csic_ssim_device needs for `nframes` (1..65535) frames of this plan (one 48-byte partial
 *                             per block of 32 windows).  Needs no device.  CSIC_EINVAL_DIMS for a frame without a window.
 * csic_ssim_device          : d_in -> d_ssim[nframes * 6] (8-byte aligned) and, unless NULL, d_map (4-byte aligned), through
 *                             d_workspace (8-byte aligned, at least the queried size); a short workspace, a misaligned pointer or
 *                             nframes outside 1..65535 fail with CSIC_EINVAL_SIZE.  Asynchronous on `hip_stream`, no allocation, no
 *                             synchronisation, hipGraph-capturable; NULL plan, d_in, d_ssim or workspace fail with CSIC_EINVAL_NULL
 *                             before any device is touched.  16-byte loads when d_in is 16-byte aligned, 4-byte loads otherwise.
 * csic_ssim_host            : the same from host memory (in_px = nframes * width * height) into ssim[nframes * 6] and, unless NULL,
 *                             map; synchronous, allocates its staging.
 * csic_ssim_kernel_name     : the kernel csic_ssim_device takes (static string): k_ssim_fast<f1> / <f2> for the plans
 *                             k_dist_fast serves whose width and height are multiples of 8, k_ssim_gen<hold> / <avg> otherwise,
 *                             with ",ycc-in" for a YCbCr input.
 * CSIC_TUNE_FORCE_GENERIC selects k_ssim_gen, CSIC_TUNE_NONTEMPORAL = 0 cached loads and CSIC_TUNE_NO_VECTOR the 4-byte loads of
 * k_ssim_fast. */
#define CSIC_SSIM_WINDOW 8
#define CSIC_SSIM_ONE    65536
int  csic_ssim_workspace_bytes(const csic_plan *plan, int32_t nframes, size_t *bytes);
int  csic_ssim_device(csic_plan *plan, const void *d_in, int32_t nframes, int64_t *d_ssim, int32_t *d_map,
                      void *d_workspace, size_t workspace_bytes, void *hip_stream);
int  csic_ssim_host(csic_plan *plan, const uint32_t *in, size_t in_px, int32_t nframes, int64_t *ssim, int32_t *map);
const char *csic_ssim_kernel_name(const csic_plan *plan);

/* ---- code statistics: what the samples of a compressed frame really carry --------------------------------------------------------
 * csic_distortion_* and csic_ssim_* measure what a parameter set costs in quality; this is the rate side.  The raw size of the
 * bit-packed planes depends on the parameters alone.  These entry points return exact histograms of the sample codes of a compressed
 * frame and of their left-predicted residuals, from which the host layers compute zero-order entropies and the size an entropy coder
 * could reach.  The coder the library has is csic_pack_* below; these counts are what sizes it, and any better one.
 *
 * Source: a compressed frame of the plan's parameters, as for csic_decode_device.  src_format is CSIC_FMT_PLANAR or
 * CSIC_FMT_PLANAR_BITS (anything else: CSIC_EINVAL_FORMAT); frames lie frame_bytes apart (csic_planar_layout_of /
 * csic_planar_bits_layout_of) and are 256-byte aligned; every parameter set csic_decode_device accepts for that format is accepted.
 *
 * Planes p = 0, 1, 2 are Y, Cb, Cr with q_p = y_bits, cb_bits, cr_bits.  Plane 0 has n_0 = y_width * y_height samples, planes 1 and
 * 2 chroma_samples each.  Bytes or bits of a plane beyond its samples are never read into a count, the unwritten tail of a partial
 * last chroma row included.  The code c_i of sample i:
 *     PLANAR      : byte i of the plane >> (8 - q)    (the low bits are ignored, not checked)
 *     PLANAR_BITS : the q bits at [i q, i q + q), LSB first, as stated above for csic_planar_bits_layout
 * Two histograms per plane, over the plane's samples in storage order:
 *     kind 0, codes     : h0[c_i] += 1
 *     kind 1, residuals : e_0 = c_0,  e_i = (c_i - c_(i-1)) mod 2^q for i >= 1,  h1[e_i] += 1
 * Storage order is the order a coder walking the plane meets the samples: the predecessor of a row's first sample is the previous
 * row's last, with no special case per row.  Worked vectors (the ones of the bit layout above):
 *     q = 3, codes 1,2,3,4,5,6,7,0 -> h1[1] = 8          q = 5, codes 0x1f, 0, 0x15 -> h1[0x1f] = h1[1] = h1[0x15] = 1
 *
 * Result per frame: uint64_t [CSIC_STATS_KINDS][CSIC_STATS_PLANES][CSIC_STATS_BINS], 12 288 bytes, frames back to back.  Bins >= 2^q
 * are 0; a plane without samples gives all zeros.  Every count is exact, so the result does not depend on scheduling.
 *
 * Derived figures (host layers only, double precision, from the counts; N = a histogram's total, n_i its bins):
 *     H_k,p = -sum (n_i / N) log2(n_i / N)   bits per sample; 0 for an empty or single-valued plane
 *     bits_per_pixel(k) = sum_p N_p H_k,p / (width * height)          ideal_bytes(k) = ceil(sum_p N_p H_k,p / 8)
 *     "best" takes, per plane, min(q_p, H_0,p, H_1,p): raw, order-0 or left-predicted, whichever a coder would choose
 *
 * csic_code_stats_device : d_src -> d_hist[nframes * 2 * 3 * 256] (8-byte aligned).  Asynchronous on `hip_stream`, no allocation, no
 *             workspace, no synchronisation, hipGraph-capturable: d_hist is cleared by a memset on the stream, blocks count in LDS and
 *             add their non-zero bins with 64-bit atomics.  NULL plan, d_src or d_hist fail with CSIC_EINVAL_NULL, a bad src_format
 *             with CSIC_EINVAL_FORMAT, nframes outside 1..65535, a d_src that is not 256-byte aligned or a d_hist that is not 8-byte
 *             aligned with CSIC_EINVAL_SIZE -- all before any device is touched.
 * csic_code_stats_host   : the same from and to host memory, synchronous, allocates its staging; src_bytes = nframes * frame_bytes
 *             (CSIC_EINVAL_SIZE otherwise).
 * csic_code_stats_kernel_name : the kernel(s) csic_code_stats_device takes: k_cstat_bytes<nt> for PLANAR, k_cstat_bits<q6,5,5,nt> for
 *             PLANAR_BITS (one instantiation per bit width: the widths of Y, Cb, Cr), k_cstat_gen<planar> / <bits> under
 *             CSIC_TUNE_FORCE_GENERIC or CSIC_TUNE_VARIANT 9 (and, for PLANAR, CSIC_TUNE_NO_VECTOR); "" for a NULL plan or another
 *             format.  The string belongs to the calling thread and is valid until its next call of this function.
 * csic_code_stats_block_samples : consecutive samples of a plane that one block counts (the predecessor crosses lanes, waves and
 *             blocks: tests build frames around this number).  Needs no device. */
#define CSIC_STATS_KINDS  2    /* 0 = codes, 1 = residuals of the left predictor */
#define CSIC_STATS_PLANES 3    /* Y, Cb, Cr */
#define CSIC_STATS_BINS   256
int  csic_code_stats_device(csic_plan *plan, const void *d_src, int32_t src_format, int32_t nframes, uint64_t *d_hist, void *hip_stream);
int  csic_code_stats_host(csic_plan *plan, const void *src, size_t src_bytes, int32_t src_format, int32_t nframes, uint64_t *hist);
const char *csic_code_stats_kernel_name(const csic_plan *plan, int32_t src_format);
int  csic_code_stats_block_samples(const csic_plan *plan, int32_t src_format, int64_t *samples);   /* samples one block covers; needs no device */

/* ---- quantiser sweep: rate and distortion of all 512 bit sets of a plan in one pass ---------------------------------------------
 * The quantiser is three AND masks and commutes with every other stage (AVG applies it last), and the three YCbCr channels are
 * independent: the Y error depends on y_bits alone, and so on.  So 8 widths x 3 planes = 24 sums and 24 histograms describe every
 * (y_bits, cb_bits, cr_bits) of a plan.  Per frame, frames back to back:
 *     sse[p][q-1]  = element 3 + p of csic_distortion_* for the same plan with plane p's bit width set to q (p = 0, 1, 2: Y, Cb, Cr;
 *                    the other two widths do not matter): pairing, reference channels, ragged edges, orders and AVG as defined there.
 *     hist[p][q-1] = kind 1 (residuals), plane p of csic_code_stats_* on the CSIC_FMT_PLANAR output of the same plan with that
 *                    width: storage order, e_0 = c_0, no special case per row; bins >= 2^q are 0.
 * The plan's own three bit widths and its out_format are ignored.  ARGB input only (CSIC_EINVAL_FORMAT otherwise), the scope of
 * CSIC_FMT_PLANAR_BITS.  Every figure is an exact integer and does not depend on scheduling.
 *
 * csic_qsweep_workspace_bytes : the workspace csic_qsweep_device needs for `nframes` (1..65535) frames: one 192-byte partial per
 *                               block of the SSE kernel, rounded up to 256 bytes, then nframes 8/8/8 CSIC_FMT_PLANAR frames.  Needs
 *                               no device; query again after csic_plan_tune.
 * csic_qsweep_device      : d_in -> d_result[nframes] (8-byte aligned) through d_workspace (256-byte aligned, at least the queried
 *                           size).  Asynchronous on `hip_stream`, no allocation, no synchronisation, hipGraph-capturable: `hist` is
 *                           cleared by a kernel, blocks count in LDS and add their non-zero bins with 64-bit atomics.  One pass over
 *                           the input for the sums (k_qsweep_sse_fast for the plans k_dist_fast serves, k_qsweep_sse_gen otherwise),
 *                           the plan's planar kernel at 8/8/8 into the workspace, and one pass over those planes (k_qsweep_hist).
 *                           NULL arguments fail with CSIC_EINVAL_NULL; nframes outside 1..65535, a d_in that is not 4-byte, a d_result
 *                           that is not 8-byte or a workspace that is not 256-byte aligned with CSIC_EINVAL_SIZE; a YCbCr input with
 *                           CSIC_EINVAL_FORMAT -- all before any device is touched; then CSIC_ENODEVICE on a machine without a
 *                           device, and CSIC_EINVAL_SIZE for a workspace smaller than the queried size.
 * csic_qsweep_hist_device : the rate half alone, on given CSIC_FMT_PLANAR frames (256-byte aligned, frame_bytes apart, the low bits
 *                           of a byte are cut per width, so the frame is an 8/8/8 one or carries junk there): writes `hist` of
 *                           d_result[nframes] and leaves `sse` untouched.  Same refusals.
 * csic_qsweep_host        : csic_qsweep_device from host memory (in_px = nframes * width * height); synchronous, allocates its staging.
 * csic_qsweep_kernel_name : the SSE kernel csic_qsweep_device takes (static string; "" for a NULL plan).
 * csic_qsweep_block_samples : consecutive samples of a plane that one block of k_qsweep_hist counts.  Needs no device.
 *
 * csic_qsweep_rank (host arithmetic, no device): sums the results of `nframes` frames and lists every (y, cb, cr) with
 * 1 <= q_p <= max_bits[p] (max_bits NULL: 8, 8, 8; a value outside 1..8: CSIC_EINVAL_BITS), in ascending order of
 * (distortion, est_bytes, y_bits, cb_bits, cr_bits).  On entry *n is the capacity of `out` (CSIC_EINVAL_SIZE when it is less than
 * max_bits[0] * max_bits[1] * max_bits[2]), on return the number of candidates written.
 *     distortion = w_0 sse_Y + w_1 sse_Cb + w_2 sse_Cr, exact uint64; weights 1..255 (NULL: 1, 1, 1; 0: CSIC_EINVAL_SIZE); a sum
 *                  that leaves 64 bits and a frame of more than 2^30 pixels are refused with CSIC_EINVAL_SIZE.
 *     est_bytes, coding = CSIC_CODING_GROUPS, CSIC_CODING_RICE or CSIC_CODING_RANS: with N_p the total of hist[p][q_p-1] (the
 *                  plane's samples over all frames) and H its zero-order entropy (double precision, as in the derived figures of
 *                  csic_code_stats_*), bits_p = min(N_p q_p, N_p H) and est_bytes = 80 + sum_p ceil(bits_p / 8).
 *     est_bytes, coding = CSIC_CODING_RAW: the exact size of the file, 80 + nframes * payload_bytes of csic_planar_bits_layout_of
 *                  for those widths.  Another coding: CSIC_EINVAL_FORMAT.
 * p->y_bits, cb_bits, cr_bits and out_format are ignored; p->in_format must be ARGB (CSIC_EINVAL_FORMAT). */
#define CSIC_QSWEEP_WIDTHS         8
#define CSIC_QSWEEP_MAX_CANDIDATES 512
#define CSIC_QSWEEP_MAX_TRIES      4     /* encodes the host layers' size-targeted compression makes at most */
typedef struct csic_qsweep_result {
    uint64_t sse[CSIC_STATS_PLANES][CSIC_QSWEEP_WIDTHS];                     /* plane p = Y, Cb, Cr; index q - 1 for width q = 1..8 */
    uint64_t hist[CSIC_STATS_PLANES][CSIC_QSWEEP_WIDTHS][CSIC_STATS_BINS];   /* residual histogram of plane p at width q          */
} csic_qsweep_result;
typedef struct csic_qsweep_candidate {
    uint64_t distortion;
    uint64_t est_bytes;
    int32_t y_bits, cb_bits, cr_bits;
    int32_t reserved;                     /* 0 */
} csic_qsweep_candidate;
int  csic_qsweep_workspace_bytes(const csic_plan *plan, int32_t nframes, size_t *bytes);
int  csic_qsweep_device(csic_plan *plan, const void *d_in, int32_t nframes, csic_qsweep_result *d_result,
                        void *d_workspace, size_t workspace_bytes, void *hip_stream);
int  csic_qsweep_hist_device(csic_plan *plan, const void *d_planar, int32_t nframes, csic_qsweep_result *d_result, void *hip_stream);
int  csic_qsweep_host(csic_plan *plan, const uint32_t *in, size_t in_px, int32_t nframes, csic_qsweep_result *result);
const char *csic_qsweep_kernel_name(const csic_plan *plan);
int  csic_qsweep_block_samples(const csic_plan *plan, int64_t *samples);
int  csic_qsweep_rank(const csic_params *p, const csic_qsweep_result *r, int32_t nframes, int32_t coding, const uint8_t weights[3],
                      const uint8_t max_bits[3], csic_qsweep_candidate *out, int32_t *n);

const char *csic_strerror(int status);
const char *csic_last_error(void);       /* thread-local; "" when the last call succeeded */

/* ---- device path --------------------------------------------------------------------------------*/
int  csic_device_count(void);            /* >= 0, or CSIC_ENODEVICE / CSIC_EHIP */

/* Validates, selects and specialises the fused kernel for `p` on HIP device `device`.  Stands in for
 * `new ImageCompressorTop(...)` (ImageCompressorTopApp.scala:53-66) / `new ImageProcessor(params)`
 * (SpatialDownsamplerSpec.scala:180): parameters are generate-time constants there and plan-time
 * constants here.  There is no CPU backend: device must be >= 0. */
int  csic_plan_create(const csic_params *p, int device, csic_plan **out);
int  csic_plan_destroy(csic_plan *plan);

/* Name of the kernel variant the plan dispatches to (static string owned by the plan), for logs,
 * tests and matching rocprofv3 kernel names. */
const char *csic_plan_kernel_name(const csic_plan *plan);

/* Tuning knobs for A/B measurements; a knob the selected kernel does not have is ignored.
 *   CSIC_TUNE_VARIANT : kernel-family specific variant index (0 = default; 1, 2 = the 16-byte f = 2 kernels, 4 = k_dec for
 *                       f = 1, 5 = k_dec instead of k_decflat on rows that do not tile into whole blocks / waves, 6 = k_decflat wherever it applies, 7 = the one-pixel-per-lane k_generic instead of k_flatgen,
 *                       8 = AVG: the tile kernel only for frames of whole tiles, as in rounds 1-3, 9 = planar (and planar bits): the general kernels instead of the fast paths,
 *                       10 = planar, factor >= 2: 4 consecutive positions per lane (k_planar_flat) instead of the transposing k_planar_strided,
 *                       11 = factor 1: k_f1x4 (rounds 1-3's kernel) instead of k_f1flat,
 *                       12 = planar AVG at factor 1 on frames of whole tiles: k_avg's body with the planar sink instead of k_planar_avg_f1)
 *   CSIC_TUNE_FORCE_GENERIC : 1 = always use the one-thread-per-pixel generic kernel
 *                             (csic_distortion_device: its general kernel k_dist_gen; csic_ssim_device: its general kernel
 *                             k_ssim_gen; csic_code_stats_device: its general kernel k_cstat_gen; nothing else changes for the
 *                             other entry points)
 *   CSIC_TUNE_NONTEMPORAL   : 1 (default) = non-temporal loads/stores for the frame stream, 0 = cached
 *   CSIC_TUNE_NO_VECTOR     : 1 = never use the 16-byte-per-lane kernels (csic_decode_device: its general kernel;
 *                             csic_distortion_device and csic_ssim_device: the 4-byte loads of their fast kernels, same sums;
 *                             csic_code_stats_device on a PLANAR source: its general kernel)
 *   CSIC_TUNE_BLOCK_THREADS : threads per block, 64 / 128 / 256 (0 = the library's choice) */
#define CSIC_TUNE_VARIANT        1
#define CSIC_TUNE_FORCE_GENERIC  2
#define CSIC_TUNE_NONTEMPORAL    3
#define CSIC_TUNE_NO_VECTOR      4   /* 1 = 4-byte accesses only (what unaligned pointers get automatically) */
#define CSIC_TUNE_BLOCK_THREADS  5   /* 0 (default) = the library's choice (256; 128 for a large single frame); 64 / 128 / 256 = forced */
int  csic_plan_tune(csic_plan *plan, int32_t knob, int32_t value);

/* One frame, device-resident: d_in holds width*height input pixels, d_out receives
 * out_width*out_height pixels.  Asynchronous on `hip_stream` (a hipStream_t, NULL = default stream);
 * no allocation, no synchronisation, hipGraph-capturable.  Replaces the per-pixel poke/peek loops
 * around the simulated RTL plus the host inverse transform
 * (ImageCompressorTopApp.scala:76-124, :118). */
int  csic_process_device(csic_plan *plan, const void *d_in, void *d_out, void *hip_stream);

/* `nframes` frames laid out back to back (frame k at d_in + k*W*H*4, d_out + k*Wo*Ho*4) in ONE launch
 * (frame index on the grid's z axis); same stream semantics as csic_process_device. */
int  csic_process_batch_device(csic_plan *plan, const void *d_in, void *d_out, int32_t nframes,
                               void *hip_stream);

/* The same for frames whose rows are NOT tightly packed: row r of frame k starts at
 * d_in + (k * height + r) * in_pitch_px pixels (resp. out_height / out_pitch_px for the output), with
 * in_pitch_px >= width and out_pitch_px >= out_width.  Padded decoder surfaces and regions of interest inside a
 * larger frame go through without a repacking copy (the reference streams pixels and has no pitch notion: the
 * semantic width -- chroma counters, ImageCompressorTop.scala:52-58 -- stays `width`; only addressing changes).
 * The 16-byte kernels need pitches that are multiples of 4 pixels, otherwise the 4-byte kernels are used. */
int  csic_process_pitched_device(csic_plan *plan, const void *d_in, int32_t in_pitch_px, void *d_out,
                                 int32_t out_pitch_px, int32_t nframes, void *hip_stream);

/* With out_format = CSIC_FMT_PLANAR, d_out of csic_process_device / csic_process_batch_device is a planar frame buffer of
 * csic_planar_layout.frame_bytes bytes per frame (256-byte aligned); csic_process_host and csic_pipeline_* hand the same
 * buffer to the host, and a frame graph of a planar plan (CSIC_FRAME_GRAPH_AUTO / _FUSED: one launch over the frames'
 * buffers) takes d_out[k] = frame k's planar buffer.  Row pitches, the per-frame-launch graph backends (_HIP, _DIRECT), the
 * file pools and csic_multi_* take packed formats only (CSIC_EINVAL_FORMAT otherwise).
 *
 * csic_reconstruct_device: `nframes` planar frames of `plan`'s parameters (the plan may have any out_format: only its
 * parameters matter) -> packed pixels, out_format = CSIC_FMT_ARGB8888 or CSIC_FMT_YCBCR888X, out_width * out_height per
 * frame back to back; asynchronous on `hip_stream`, no allocation, capturable. */
int  csic_reconstruct_device(csic_plan *plan, const void *d_planar, void *d_out, int32_t nframes, int32_t out_format,
                             void *hip_stream);
/* The same for CSIC_FMT_PLANAR_BITS frames (frame_bytes of csic_planar_bits_layout_of apart, 256-byte aligned). */
int  csic_reconstruct_bits_device(csic_plan *plan, const void *d_bits, void *d_out, int32_t nframes, int32_t out_format,
                                  void *hip_stream);

/* ---- full-resolution decode: a compressed frame back to width x height pixels ----------------------------------------------
 * csic_reconstruct*_device and csic_process_device stop at the decimated frame, out_width x out_height.  csic_decode_* produce the
 * frame a viewer looks at, and the one csic_distortion_* measures.
 *
 * Definition.  Let o be the packed output of the plan's parameters in `out_format`, out_width x out_height (what
 * csic_reconstruct*_device yields from a planar source and csic_process_device yields directly).  Then
 *     decode(r, c) = o(r / f, c / f)        0 <= r < height, 0 <= c < width, integer division by the plan's factor f
 * -- replication upsampling; ragged edges follow the same rule because out_width = ceil(width / f).  At f = 1 the decode equals the
 * reconstruct output bit for bit.  Only the plan's parameters matter, as for reconstruct: any in_format, any out_format of the plan,
 * HOLD_DECIMATE or AVG, all six orders.  It is the pairing of csic_distortion_*: the sums of squared differences between an input
 * frame and decode(compress(input)) ARE that frame's distortion, channel by channel.
 *
 * src_format: CSIC_FMT_PLANAR_BITS / CSIC_FMT_PLANAR -- frames frame_bytes apart (csic_planar_bits_layout_of / csic_planar_layout_of),
 *             256-byte aligned (CSIC_EINVAL_SIZE otherwise), the chroma replay rule of csic_reconstruct_device, replay_last rows included;
 *             CSIC_FMT_YCBCR888X / CSIC_FMT_ARGB8888 -- out_width * out_height packed pixels per frame, back to back.
 * out_format: CSIC_FMT_ARGB8888 (through YCbCrUtils.ycbcr2rgb, as every packed ARGB output) or CSIC_FMT_YCBCR888X; width * height
 *             pixels per frame, back to back.  An ARGB source is replicated as it is; an ARGB source with a YCbCr output is refused
 *             (CSIC_EINVAL_FORMAT: the inverse transform has no inverse).
 * csic_decode_device : asynchronous on `hip_stream`, no allocation, no synchronisation, hipGraph-capturable; NULL arguments fail with
 *             CSIC_EINVAL_NULL and nframes <= 0 with CSIC_EINVAL_SIZE before any device is touched.  A packed source or an output that
 *             is only 4-byte aligned works (4-byte accesses).  More than 65535 frames go out as several launches.
 * csic_decode_host   : the same from and to host memory, synchronous, allocates its staging; src_bytes = nframes * frame_bytes (planar
 *             sources) or nframes * out_width * out_height * 4, out_px = nframes * width * height (CSIC_EINVAL_SIZE otherwise).
 * csic_decode_kernel_name : the kernel csic_decode_device takes for one frame in 16-byte aligned buffers ("" for a refused format pair).  At f = 1 a
 *             planar source is a reconstruct and the name is that kernel's (k_rbits / k_recon).  The string belongs to the calling
 *             thread and is valid until its next call of this function.
 * CSIC_TUNE_VARIANT 9, CSIC_TUNE_NO_VECTOR and CSIC_TUNE_FORCE_GENERIC select the general kernel (one output pixel per lane);
 * CSIC_TUNE_NONTEMPORAL and CSIC_TUNE_BLOCK_THREADS apply as in csic_reconstruct_bits_device. */
int  csic_decode_device(csic_plan *plan, const void *d_src, int32_t src_format, void *d_out, int32_t out_format, int32_t nframes,
                        void *hip_stream);
int  csic_decode_host(csic_plan *plan, const void *src, size_t src_bytes, int32_t src_format, uint32_t *out, size_t out_px,
                      int32_t out_format, int32_t nframes);
const char *csic_decode_kernel_name(const csic_plan *plan, int32_t src_format, int32_t out_format);

/* ---- view decode: a cropped, box-reduced window of a compressed frame ---------------------------------------------------------
 * csic_decode_* produce the whole frame.  csic_decode_view_* produce a window of it, reduced by an s x s box, without writing the
 * frame: a thumbnail of all of it, or full detail of a part of it.
 *
 * Definition.  Let `decode` be csic_decode_*'s frame for the same plan, source format and output format, and s = view->scale, one
 * of 1, 2, 4, 8, 16.  For 0 <= r < view->height, 0 <= c < view->width and each of the four bytes b of a packed pixel
 *     view(r, c).b = ( SUM over i < s, j < s of decode(y0 + r s + i, x0 + c s + j).b  +  (s s >> 1) ) >> (2 log2 s)
 * -- the average is taken over the decoded BYTES, after the inverse transform and its clamps, not over the samples (for an ARGB
 * output that is a different number from transforming an average); the fourth byte is treated like the others (it is constant in
 * `decode`, so it comes through unchanged); s = 1 is a crop of `decode`, bit for bit.  There is no partial box and no division.
 * Worked vector, s = 2, the four decoded pixels of one box -> the view's pixel:
 *     FF102030 FF112131 FF122232 FF142434 -> FF122232      (B: 30 + 31 + 32 + 34 = C7 hex, + 2, >> 2 = 32 hex)
 *     FF000000 FF000001 FF0000FF FF000100 -> FF000040      (B: 0 + 1 + FF + 0 = 100 hex -> 40; G: 0 + 0 + 0 + 1 -> (1 + 2) >> 2 = 0)
 * view->width and view->height count OUTPUT pixels; the source rectangle must lie inside the frame: x0, y0 >= 0, width, height >= 1,
 * x0 + width s <= the plan's width and y0 + height s <= the plan's height, evaluated in 64 bits.  A rectangle that does not, and a
 * scale outside the set, are refused with CSIC_EINVAL_SIZE.  Source and output formats, the refused ARGB -> YCbCr pair, the alignment
 * rules (256-byte aligned planar frames; a packed source or an output that is only 4-byte aligned works), HOLD_DECIMATE and AVG and
 * all six orders are as for csic_decode_*.  Output: view->width * view->height pixels per frame, back to back; the one view applies
 * to all `nframes` frames.
 * csic_decode_view_device : asynchronous on `hip_stream`, no allocation, no synchronisation, hipGraph-capturable; NULL arguments fail
 *             with CSIC_EINVAL_NULL and nframes <= 0, a bad view or a bad format with their codes before any device is touched.  More
 *             than 65535 frames go out as several launches.
 * csic_decode_view_host   : the same from and to host memory, synchronous, allocates its staging; src_bytes as for csic_decode_host,
 *             out_px = nframes * view->width * view->height (CSIC_EINVAL_SIZE otherwise).
 * csic_decode_view_kernel_name : the kernel csic_decode_view_device takes for one frame in 16-byte aligned buffers ("" for a refused
 *             format pair or view): k_view<...>, a lane per 4 output pixels and 16-byte stores, when view->width % 4 == 0, else
 *             k_view_gen<...>, a lane per output pixel.  The string belongs to the calling thread until its next call of this function.
 * CSIC_TUNE_VARIANT 9, CSIC_TUNE_NO_VECTOR and CSIC_TUNE_FORCE_GENERIC select the general kernel; CSIC_TUNE_NONTEMPORAL and
 * CSIC_TUNE_BLOCK_THREADS apply as in csic_decode_device. */
typedef struct csic_view { int32_t x0, y0, width, height, scale; } csic_view;   /* width, height: OUTPUT pixels */
int  csic_decode_view_device(csic_plan *plan, const void *d_src, int32_t src_format, const csic_view *view, void *d_out,
                             int32_t out_format, int32_t nframes, void *hip_stream);
int  csic_decode_view_host(csic_plan *plan, const void *src, size_t src_bytes, int32_t src_format, const csic_view *view, uint32_t *out,
                           size_t out_px, int32_t out_format, int32_t nframes);
const char *csic_decode_view_kernel_name(const csic_plan *plan, int32_t src_format, int32_t out_format, const csic_view *view);

/* Row pitches, in pixels, at which frames of this plan stream fastest when the CALLER lays them out
 * (csic_process_pitched_device).  Measured on 2048- to 16384-pixel rows x every factor x 13 (input pad, output pad) pairs
 * (tools/probe_pitch2.py, profiles/r04_probe_pitch.jsonl, r04_probe_pitch_f1flat.jsonl): on the round-4 kernels packed rows are
 * as fast as any padded layout -- the gains rounds 2 and 3 saw from 1 KiB of padding (8192-pixel rows: +2-4 points at factor
 * 2 / 8 with k_dec, +2-5 points at factor 1 with k_f1x4) were properties of those kernels' block-to-address mappings and went
 * away with the flat mappings of k_decflat and k_f1flat; pads of 16-64 pixels lose up to 10 points.  So this returns the
 * widths themselves today.  It exists so that a caller that owns its surfaces asks instead of guessing. */
int  csic_plan_preferred_pitch(const csic_plan *plan, int32_t *in_pitch_px, int32_t *out_pitch_px);

/* ---- the range-checking build (diagnostics) ----------------------------------------------------------------------
 * `make -C chroma-subsampling-image-compressor_amd/csrc debug` builds libcsic_hip_debug.so from the same sources with
 * -DCSIC_DEBUG: every global access of the pixel kernels is checked against the frame's extent -- (H - 1) * pitch + W
 * pixels of input, (Ho - 1) * pitch + Wo of output, the planar frame's frame_bytes -- and a violation executes s_trap: the
 * queue reports a hardware exception and the process aborts instead of reading or writing a neighbour's memory silently.
 * It is the GPU-side stand-in for a sanitizer (GPU AddressSanitizer is not available on the pool); load it with
 * CSIC_LIB=<path> (Python host) or link it instead of libcsic_hip.so.  csic_debug_build() tells which build is loaded;
 * csic_debug_probe_device performs ONE checked read at pixel offset `offset_px` of a width x height frame (into *d_sink):
 * in the debug build an offset outside the frame traps, in the product build it is the caller's out-of-bounds read --
 * tests use it (in a child process) to show that the checks are live. */
int  csic_debug_build(void);
int  csic_debug_probe_device(const void *d_frame, int32_t width, int32_t height, int64_t offset_px, void *d_sink, void *hip_stream);

/* Convenience synchronous host path: H2D + kernel + D2H through plan-owned staging buffers.
 * in_px must equal width*height and out_px out_width*out_height (planar: frame_bytes / 4). */
int  csic_process_host(csic_plan *plan, const uint32_t *in, size_t in_px, uint32_t *out, size_t out_px);

/* Synthetic frame generator of SURVEY.md 8(d), on the device:
 *   dst[i] = 0xFF000000 | (fmix32((uint32)(first_index + i) + seed * 0x9E3779B9) & 0xFFFFFF)
 * Used by bench.py and the full-size property tests so that frames never cross PCIe. */
int  csic_synth_frame_device(void *d_dst, int64_t npix, int64_t first_index, uint32_t seed,
                             void *hip_stream);

/* Plain device-to-device copy of npix pixels with 16-byte-per-lane non-temporal accesses: the measured
 * streaming ceiling that bench.py reports next to the spec-peak roofline.  npix % 4 == 0,
 * 16-byte aligned pointers; asynchronous on `hip_stream`. */
int  csic_copy_device(void *d_dst, const void *d_src, int64_t npix, void *hip_stream);

/* 64-bit order-sensitive checksum of npix pixels in device memory (sum of fmix32-mixed
 * (pixel, index) pairs), for the full-size parity properties; synchronous. */
int  csic_checksum_device(const void *d_src, int64_t npix, uint64_t *sum, void *hip_stream);

/* ---- pre-recorded per-frame launches (BASELINE.json configs[4], "hipGraph-captured per-frame launch") ------
 * A stream of frames that live in SEPARATE device buffers (a decoder's surface pool) cannot use the one
 * contiguous batched launch of csic_process_batch_device, and a frame of 10-25 MB is only 1.3-3 us of HBM time
 * behind the ~1.7 us dependent-kernel boundary that every launch on a HIP stream -- eager or replayed from a
 * hipGraph chain -- pays.  A frame graph records one launch per frame once (frame k: d_in[k] -> d_out[k]; same
 * preconditions as csic_process_device) and replays them so that independent frames overlap.  The reference
 * processes images strictly one after the other (ImageCompressorTopApp.scala:23-145, a fresh DUT per image);
 * frames are independent, so no ordering between them has to be kept.  Three backends:
 *
 *   CSIC_FRAME_GRAPH_HIP     `branches` hipGraph chains (kernel nodes identical to the eager launch), chain 0
 *                            replayed on the caller's stream, the others on internal streams forked from and
 *                            joined to it by events: csic_frame_graph_launch is asynchronous and fully ordered
 *                            with `hip_stream`.  branches = 1 is the strictly serial graph that capturing a loop
 *                            of csic_process_device calls gives.  (ONE hipGraph with parallel branches is not
 *                            used: ROCm 7.2 replays such a graph node by node from the host, slower than a chain.)
 *   CSIC_FRAME_GRAPH_DIRECT  the same launches as pre-built AQL kernel-dispatch packets on `branches` (= queues,
 *                            default up to 3, max 8) user-mode HSA queues owned by the library, frame k on queue
 *                            k % queues, WITHOUT the barrier bit HIP sets on every packet: consecutive frames
 *                            overlap like the workgroups of one big launch (cfg 5 frame: 3.65 us in a hipGraph
 *                            chain, 1.76 us here, 1.75 us in one batched launch).  These queues are NOT HIP
 *                            streams: csic_frame_graph_submit starts the work immediately -- the caller makes
 *                            the inputs ready first (e.g. by synchronising the producing stream) -- and returns
 *                            a ticket; csic_frame_graph_wait blocks the host until that submission (and all
 *                            earlier ones of this graph) has finished, outputs visible to host and device.
 *                            csic_frame_graph_launch(graph, hip_stream) orders the same work with a HIP stream on
 *                            the device, asynchronously: the graph's signals are HIP "signal memory"
 *                            (hipExtMallocWithFlags(.., hipMallocSignalMemory) -- the value word of an HSA signal,
 *                            usable as hsa_signal_t in AQL barrier packets and readable / writable by kernels).
 *                            Every queue starts with a one-wave gate kernel that spins on the gate word; ONE one-wave
 *                            hand-off kernel on `hip_stream` opens the gate when the stream reaches it and then spins
 *                            until every queue's closing packet has zeroed its done word; work enqueued on
 *                            `hip_stream` afterwards sees the outputs.  (A dependency resolved by the command
 *                            processor polling a signal -- AQL barrier packets, hipStreamWaitValue64 -- costs about
 *                            10 us per hop on this part; a polling wave reacts within a microsecond.  Both spins are
 *                            bounded: after CSIC_DIRECT_TIMEOUT_MS (environment, default 30000) the kernel flags the
 *                            graph and returns, and the next launch / wait of that graph reports CSIC_EHIP.
 *                            CSIC_DIRECT_HANDOFF=cp in the environment keeps the command-processor form -- gate
 *                            barrier packets opened by hipStreamWriteValue64, hipStreamWaitValue64 on the closing
 *                            signal -- for comparison.)
 *                            csic_frame_graph_stream_ordered() tells whether the runtime offered this (else launch
 *                            degrades to hipStreamSynchronize + submit + wait).  A gate blocks its queues until the
 *                            stream reaches it, so do not make that stream's earlier work depend on a LATER direct
 *                            submission.  Up to 16 submissions/launches may be outstanding per graph (a 17th waits
 *                            for the oldest); host-ordered submissions are not ordered among themselves.
 *                            Queue count: the device runs 4 queues at once.  Host-ordered submissions are fastest
 *                            on 4 (cfg 5 frame 1.71 us, 3 queues 1.78 us).  A stream-ordered launch also keeps the
 *                            launch stream's own queue busy (its hand-off kernel runs as long as the frames do), and with
 *                            4 + 1 active queues the hardware scheduler time-slices them (64 frames: 250 us instead of
 *                            126 us) -- so csic_frame_graph_launch NEVER uses more than 3 queues: a graph created with
 *                            more keeps a second dealing of its frames over 3 queues for launches and uses all of them
 *                            for csic_frame_graph_submit.  A stream-ordered launch costs about 8 us of hand-off on top
 *                            of the host-ordered time (17-40 us in the command-processor form): record several frames
 *                            per graph.
 *                            Limits a caller must know:
 *                            - NOT capturable.  csic_frame_graph_launch on a capturing stream returns CSIC_ECAPTURE (the
 *                              packets would go out at capture time and a replay would find nothing behind its hand-off).
 *                            - The gate waves are dispatched when the host calls launch, not when the stream gets there:
 *                              stream work in front of a launch that runs LONGER than CSIC_DIRECT_TIMEOUT_MS makes the
 *                              gate give up -- the frames then run on inputs that may not be ready, the graph's error
 *                              word is set, and the next launch / wait / destroy of that graph reports CSIC_EHIP.  Raise
 *                              the timeout for such hosts; it bounds how long a wave may spin, nothing else.
 *                            - Waiting for ring space is bounded too (CSIC_DIRECT_SUBMIT_TIMEOUT_MS, default twice the
 *                              device bound + 5 s).  Room is checked on every queue BEFORE anything is written, so a
 *                              submission that cannot start fails cleanly (nothing queued, the engine stays usable).
 *                              Only a graph larger than the rings (> 4096 packets per queue, host-ordered) can fail between
 *                              two chunks; that marks the device's engine failed: every later DIRECT call on the device
 *                              returns CSIC_EHIP with the first failure's message, and what the stuck packets refer to
 *                              is leaked instead of freed.
 *
 *   CSIC_FRAME_GRAPH_FUSED   not per-frame launches at all: ONE kernel launch covers every frame (frame index on the
 *                            grid's z axis, the frame bases read from a device-resident pointer table the graph owns), so
 *                            frames in separate buffers run exactly like csic_process_batch_device's contiguous batch.
 *                            csic_frame_graph_launch is an ordinary asynchronous launch on `hip_stream`: fully ordered,
 *                            hipGraph-capturable, no internal streams or queues (`branches` is ignored).
 *
 * A graph, like a plan, is not thread-safe (one thread at a time per graph, including its ticket bookkeeping; different
 * graphs may be used from different threads, the library serialises their access to its queues).
 * csic_frame_graph_destroy waits for the graph's DIRECT submissions and for the HIP backend's internal streams; work that
 * csic_frame_graph_launch put on the CALLER's stream (chain 0 of the HIP backend, the fused launch) is the caller's to
 * synchronise before destroying the graph, as with any resource a stream still uses.
 * branches <= 0 selects the backend's default for the frame size (more overlap for smaller frames; measured table
 * in profiles/r02_small_launch.md).  The pointer arrays are read at creation only; the buffers they
 * name must stay valid for as long as the graph is launched.  csic_frame_graph_create == _create_ex with
 * CSIC_FRAME_GRAPH_AUTO, which today always resolves to FUSED: the plain entry point gives the fastest stream-ordered
 * path (cfg 5: 76 % of the HBM roofline against 42 % for hipGraph chains); per-frame launches are there for callers who
 * name them. */
#define CSIC_FRAME_GRAPH_HIP    0
#define CSIC_FRAME_GRAPH_DIRECT 1
#define CSIC_FRAME_GRAPH_FUSED  2
#define CSIC_FRAME_GRAPH_AUTO   3   /* the library's choice: FUSED (all frames of a graph share one plan, so it always applies) */
#define CSIC_FRAME_GRAPH_DEFAULT_BRANCHES 4   /* HIP backend, small frames (2 chains when a frame is >= 5 us of HBM time)          */
#define CSIC_FRAME_GRAPH_DEFAULT_QUEUES   3   /* DIRECT backend, small frames (2 queues from 2.5 us, 1 queue from 10 us per frame); see below */
typedef struct csic_frame_graph csic_frame_graph;
int  csic_frame_graph_create(csic_plan *plan, const void *const *d_in, void *const *d_out, int32_t nframes,
                             int32_t branches, csic_frame_graph **out);
int  csic_frame_graph_create_ex(csic_plan *plan, const void *const *d_in, void *const *d_out, int32_t nframes,
                                int32_t branches, int32_t backend, csic_frame_graph **out);
int  csic_frame_graph_launch(csic_frame_graph *graph, void *hip_stream);
int  csic_frame_graph_submit(csic_frame_graph *graph, int64_t *ticket);            /* DIRECT only */
int  csic_frame_graph_wait(csic_frame_graph *graph, int64_t ticket);               /* DIRECT only; ticket < 0 = all */
int  csic_frame_graph_count(const csic_frame_graph *graph, int32_t *nframes, int32_t *branches);
int  csic_frame_graph_backend(const csic_frame_graph *graph);                      /* the RESOLVED backend (never AUTO), or < 0 */
int  csic_frame_graph_launch_branches(const csic_frame_graph *graph);              /* chains / queues csic_frame_graph_launch uses: DIRECT min(branches, 3), FUSED 1 */
int  csic_frame_graph_stream_ordered(const csic_frame_graph *graph);               /* 1: launch() is asynchronous and ordered with its stream */
int  csic_frame_graph_destroy(csic_frame_graph *graph);

/* ---- PNG files (host only; reading: the library's own inflate, writing: zlib) ------------------------
 * The codec either side of the path: stands in for scrimage's loader / PngWriter behind
 * ImageProcessorModel.readImage / writeImage (ImageProcessorModel.scala:14-22).  Decoding yields straight
 * 8-bit samples as ARGB ints with alpha = 255 (input alpha dropped, gAMA/cHRM not applied -- the behaviour
 * the reference's golden images pin) and writes directly into `dst`, which may be a pinned
 * buffer from csic_pipeline_acquire_input.  Non-interlaced PNGs of every colour type / bit depth are read;
 * 8-bit RGB is written (`level` = zlib level 0..9; at level 1 a frame encodes about four times faster than at 6),
 * images of more than 1 MiB of filtered data on up to 16 threads (CSIC_PNG_THREADS=n sets the number; the bytes
 * written do not depend on it: the deflate stream is cut into pieces by the data alone).
 * The reader accepts and rejects exactly what zlib's inflate does (csrc/csic_inflate.cpp); environment variable
 * CSIC_NO_SIMD=1 keeps it off the PCLMULQDQ / SSSE3 paths it otherwise takes where the CPU has them. */
int  csic_png_info(const char *path, int32_t *width, int32_t *height);
int  csic_png_read_argb(const char *path, uint32_t *dst, size_t dst_px);
int  csic_png_write_argb(const char *path, const uint32_t *src, int32_t width, int32_t height, int32_t level);

/* ---- lossless group coding of the bit planes (csic_pack_*) ----------------------------------------------------------------------
 * csic_code_stats_* say what an entropy coder could reach; this is the library's first coder, chosen so that encode and decode are
 * data-parallel per group of 32 samples and need no serial bit stream.  It is lossless: unpack(pack(x)) gives back the three payload
 * ranges of x.  (The per-sample variable-length coder that comes closer to the entropy bound is csic_rice_* below.)
 *
 * Input: one CSIC_FMT_PLANAR_BITS frame of the parameters.  Planes p = 0, 1, 2 are Y, Cb, Cr with q_p = y_bits, cb_bits, cr_bits bits
 * per code and n_0 = y_width * y_height, n_1 = n_2 = chroma_samples samples (as for csic_code_stats_*); c_i is the code of sample i in
 * storage order.
 *
 * Groups.  A plane is cut into G_p = ceil(n_p / 32) groups of 32 consecutive samples: one group is exactly q dwords of the source, no
 * sample straddles a group.  The last group is completed by repeating the plane's last real code.  Source bits and bytes beyond sample
 * n_p - 1 are never read into a value (they are undefined in a PLANAR_BITS buffer).  Per group g, with slots j = 0 .. 31:
 *     anchor_g = c_(32 g)                                        the group's first code
 *     e_0 = 0,   e_j = (c_(32 g + j) - c_(32 g + j - 1)) mod 2^q    for j >= 1
 *     s_j = e_j if e_j < 2^(q - 1), else e_j - 2^q               the centred residual
 *     u_j = 2 s_j if s_j >= 0, else -2 s_j - 1                   folded: 0 <= u_j < 2^q
 *     w_g = the number of significant bits of max_j u_j          0 when every u_j is 0; 0 <= w_g <= q
 * Groups do not depend on each other: the predictor restarts at every group, so decode needs no scan over samples.
 *
 * The coded frame (CSIC_CODING_GROUPS) is a byte string.  Every section starts at a multiple of 4, every padding bit is 0 (the string
 * is deterministic), bit order is LSB first as in PLANAR_BITS.  Sections, in this order:
 *     1. widths of Y, Cb, Cr   nibble g at bits [4 g, 4 g + 4) holds w_g; each section 4 * ceil(G_p / 8) bytes
 *     2. anchors of Y, Cb, Cr  a PLANAR_BITS-style plane of G_p codes at q_p bits; each section 4 * ceil(G_p q_p / 32) bytes
 *     3. payload               all groups of Y, then of Cb, then of Cr: group g occupies w_g dwords, slot j's u_j at bits
 *                              [j w_g, j w_g + w_g) of those dwords; a group with w_g = 0 occupies nothing
 *     fixed_bytes = the sum of sections 1 and 2         coded_bytes = fixed_bytes + 4 * sum of w_g over all groups
 *     bound_bytes = the next multiple of 256 at or above fixed_bytes + 4 * sum_p G_p q_p          (no frame codes to more)
 * Worked vectors, one plane alone (the ones of the bit layout):
 *     q = 3, codes 1,2,3,4,5,6,7,0 -> w = 2, widths 02 00 00 00, anchors 01 00 00 00, payload a8 aa 00 00 00 00 00 00
 *     q = 5, codes 0x1f, 0, 0x15   -> anchor 0x1f, u = 0, 2, 21, 0, ..., w = 5
 * Decode: c_(32 g) = anchor_g, c_(32 g + j) = (c_(32 g + j - 1) + e_j) mod 2^q with e_j unfolded from u_j.  It writes exactly the
 * y_bytes / cb_bytes / cr_bytes of the PLANAR_BITS frame (the unused high bits of a plane's last byte 0) and nothing outside them.
 *
 * Host codec (no GPU; the parameters are those csic_container_write accepts, with its statuses; p->out_format is ignored):
 *   csic_pack_layout_of : groups, section offsets and sizes of a coded frame of these parameters.
 *   csic_pack_host      : one frame (frame_bytes of csic_planar_bits_layout_of) -> coded[0, *coded_bytes).  A `capacity` below the
 *                         frame's coded size fails with CSIC_EINVAL_SIZE (bound_bytes always suffices); *coded_bytes then holds the
 *                         size that was needed.
 *   csic_unpack_host    : coded[0, coded_bytes) -> the three payload ranges of one frame buffer; the rest of the buffer is not touched.
 *                         The input is untrusted: a nibble greater than q_p, a padding bit that is not 0 (widths or anchors) or a
 *                         coded_bytes other than what the widths imply give CSIC_EFORMAT and write nothing; whatever the bytes, nothing
 *                         outside coded[0, coded_bytes) is read and nothing outside the payload ranges written.
 *
 * Device codec (gfx950), asynchronous on `hip_stream`, no allocation, no synchronisation, hipGraph-capturable; three launches per
 * direction in stream order (widths / sums, a scan of the blocks' totals, emit), no block ever waits for another:
 *   csic_pack_workspace_bytes : the workspace both directions need for `nframes` (1..65535) frames: one uint32 per block of 256
 *                         groups and frame.  Needs no device.
 *   csic_pack_device    : d_bits (frames frame_bytes apart, 256-byte aligned) -> d_coded (frames bound_bytes apart, 256-byte aligned)
 *                         and d_sizes[k] (8-byte aligned) = frame k's coded_bytes.  Bytes of a coded frame beyond its coded_bytes are
 *                         not written.
 *   csic_unpack_device  : the inverse.  Bytes of a PLANAR_BITS frame outside the three payload ranges are not written.  It does NOT
 *                         validate: a nibble takes part as min(nibble, q_p), so that no access can leave a frame's bound_bytes, and
 *                         a coded frame csic_unpack_host would refuse decodes to some valid codes.  Validate untrusted input on the host.
 *   csic_pack_kernel_name : the kernels of both directions, "k_pack<q6,5,5,nt>" (one instantiation per bit width, as k_cstat_bits);
 *                         "" for a NULL plan.  The string belongs to the calling thread until its next call of this function.
 * NULL plan / buffers fail with CSIC_EINVAL_NULL; nframes outside 1..65535, a misaligned pointer (d_workspace: 8 bytes) or a short
 * workspace with CSIC_EINVAL_SIZE -- all before any device is touched.  CSIC_TUNE_NONTEMPORAL applies to the accesses of the
 * PLANAR_BITS frames; CSIC_TUNE_BLOCK_THREADS is ignored (a block is 256 lanes = 256 groups: the workspace is laid out by it), and so
 * are the other knobs. */
#define CSIC_CODING_RAW    0   /* the planes' payload bytes as they are (.csic version 1) */
#define CSIC_CODING_GROUPS 1   /* the group coding above (.csic version 3)                */
typedef struct csic_pack_layout {
    int64_t groups[3];             /* G_p                                                              */
    int64_t widths_offset[3];      /* byte offsets of the sections inside a coded frame               */
    int64_t anchors_offset[3];
    int64_t payload_offset;        /* = fixed_bytes                                                    */
    int64_t fixed_bytes;
    int64_t bound_bytes;           /* multiple of 256: the distance of coded frames in device memory   */
} csic_pack_layout;
int  csic_pack_layout_of(const csic_params *p, csic_pack_layout *layout);
int  csic_pack_host(const csic_params *p, const void *bits_frame, void *coded, size_t capacity, uint64_t *coded_bytes);
int  csic_unpack_host(const csic_params *p, const void *coded, size_t coded_bytes, void *bits_frame);
int  csic_pack_workspace_bytes(const csic_plan *plan, int32_t nframes, size_t *bytes);
int  csic_pack_device(csic_plan *plan, const void *d_bits, int32_t nframes, void *d_coded, uint64_t *d_sizes,
                      void *d_workspace, size_t workspace_bytes, void *hip_stream);
int  csic_unpack_device(csic_plan *plan, const void *d_coded, int32_t nframes, void *d_bits,
                        void *d_workspace, size_t workspace_bytes, void *hip_stream);
const char *csic_pack_kernel_name(const csic_plan *plan);

/* ---- lossless Rice coding of the bit planes (csic_rice_*) -------------------------------------------------------------------------
 * The group coding stores every group at the width of its largest residual: one edge pixel sets the cost of its 31 neighbours.  This
 * coding (CSIC_CODING_RICE) gives each sample a Golomb-Rice code with a parameter chosen per group, and stays as data-parallel: one
 * lane per group, no serial bit stream across groups, no stored lengths.  Coding id 2 was never written and stays refused.
 *
 * Carried over from the group coding, word for word: the input is one CSIC_FMT_PLANAR_BITS frame; planes, q_p, n_p, the groups of 32
 * (G_p of them), anchor_g, e_j, s_j and the folded u_j (slots j = 1 .. 31) are as above; the last group is completed with the plane's
 * last real code; bits beyond sample n_p - 1 are never read into a value; bit order is LSB first, every section starts at a multiple
 * of 4 and every padding bit is 0.
 *
 * Mode of a group, a nibble m_g:
 *     m = 15        zero: every u_j is 0, the group stores nothing
 *     m = k < q     Rice (a "unary group"): slot j stores the k low bits of u_j and (u_j >> k) in unary; 31 k + sum_j ((u_j >> k) + 1) bits
 *     m = q         raw: 31 q bits; k = q with the unary part omitted
 * The encoder takes zero mode when it applies, otherwise the cheapest of k = 0 .. q and on a tie the smallest k: no group costs more
 * than 31 q bits.
 *
 * Blocks.  Plane p has B_p = ceil(G_p / 256) blocks of 256 consecutive groups; a frame's blocks are numbered Y, then Cb, then Cr;
 * NB = sum_p B_p.
 *
 * Sections, in this order:
 *     1. modes of Y, Cb, Cr     nibble g at bits [4 g, 4 g + 4); each section 4 * ceil(G_p / 8) bytes, padding nibbles 0
 *     2. anchors of Y, Cb, Cr   exactly as in the group coding
 *     3. directory              NB + 1 uint32: dir[i] = the dword offset of block i's chunk from payload_offset, dir[0] = 0,
 *                               dir[NB] = the number of payload dwords
 *     4. payload                one chunk per block, back to back; a chunk is R then U:
 *          R   for each group of the block in order 31 k_g bits, slot j's u_j & (2^k - 1) at bits [(j - 1) k, j k) of the group's run
 *              (zero groups and k = 0 groups contribute nothing); runs bit-contiguous, R zero-padded to a dword
 *          U   for each unary group in order and j = 1 .. 31: (u_j >> k) zero bits, then a one bit (the terminator);
 *              bit-contiguous, zero-padded to a dword
 *     fixed_bytes = the sum of sections 1 to 3              coded_bytes = fixed_bytes + 4 * dir[NB]
 *     a chunk is at most 248 q_p + 1 dwords (R + U <= 256 * 31 q bits); a longer one is not a coded frame
 *     bound_bytes = the next multiple of 256 at or above fixed_bytes + 4 * sum_p B_p (248 q_p + 1)
 * Decode of group g in block b: R starts at dir[b]; the group's run in R starts at sum 31 k over the earlier groups of the block; U
 * starts ceil(R bits / 32) dwords behind R's start; the group's unary run starts right behind terminator number 31 z of U, z = the
 * unary groups before g in the block (z = 0: bit 0 of U).  u_j = (zeros << k) | remainder, then unfold and prefix-sum as above.
 * Worked vector, one plane alone: q = 3, codes 1,2,3,4,5,6,7,0 -> u_1 .. u_7 = 2, the rest 0; k = 0 costs 45 bits;
 *     modes 00 00 00 00, anchors 01 00 00 00, directory 00 00 00 00 02 00 00 00, payload 24 49 f2 ff ff 1f 00 00
 *
 * Host codec (no GPU; parameters and statuses as for csic_pack_*):
 *   csic_rice_layout_of   : groups, blocks, section offsets and sizes of a coded frame of these parameters.
 *   csic_rice_pack_host   : as csic_pack_host, capacity rule included.
 *   csic_rice_unpack_host : as csic_unpack_host.  The input is untrusted; CSIC_EFORMAT, nothing written, for: a nibble outside
 *                         {0 .. q_p, 15}; a padding nibble, anchor padding bit or R / U padding bit that is not 0; dir[0] != 0 or a chunk
 *                         that is not ceil(R / 32) + ceil(U / 32) dwords (or longer than 248 q_p + 1); coded_bytes != fixed_bytes +
 *                         4 dir[NB]; a U that does not hold exactly 31 terminators per unary group; a decoded u_j >= 2^q.  Whether the
 *                         encoder's k was the cheapest is not checked.
 * Device codec (gfx950), with the argument lists, alignment rules, refusals before any device is touched, asynchrony and
 * capturability of csic_pack_*:
 *   csic_rice_workspace_bytes : what csic_rice_pack_device needs: one uint32 per block and frame.
 *   csic_rice_pack_device : three launches per run of planes of one width (modes and sums; the scan of the group coding; emit, which
 *                         assembles each chunk in LDS and stores it and its directory entry as whole dwords).
 *   csic_rice_unpack_device : ONE pass, no workspace: a block reads its directory entry, takes its chunk into LDS, counts terminators
 *                         per dword and selects each group's start.  It does NOT validate: a nibble takes part as min(m, q_p) (15:
 *                         zero mode), chunk extents are clamped to bound_bytes and to 248 q_p + 1 dwords, a unary run ends with its
 *                         chunk at the latest, u is masked to q bits.  Whatever the bytes, nothing outside a frame's bound_bytes is
 *                         read and nothing outside the three payload ranges written.  Validate untrusted input on the host.
 *   csic_rice_kernel_name : "k_rice<q6,5,5,nt>". */
#define CSIC_CODING_RICE   3   /* the Rice coding above (.csic version 4)                 */
typedef struct csic_rice_layout {
    int64_t groups[3];             /* G_p                                                              */
    int64_t blocks[3];             /* B_p                                                              */
    int64_t modes_offset[3];       /* byte offsets of the sections inside a coded frame               */
    int64_t anchors_offset[3];
    int64_t directory_offset;      /* sum_p B_p + 1 uint32                                             */
    int64_t payload_offset;        /* = fixed_bytes                                                    */
    int64_t fixed_bytes;
    int64_t bound_bytes;           /* multiple of 256: the distance of coded frames in device memory   */
} csic_rice_layout;
int  csic_rice_layout_of(const csic_params *p, csic_rice_layout *layout);
int  csic_rice_pack_host(const csic_params *p, const void *bits_frame, void *coded, size_t capacity, uint64_t *coded_bytes);
int  csic_rice_unpack_host(const csic_params *p, const void *coded, size_t coded_bytes, void *bits_frame);
int  csic_rice_workspace_bytes(const csic_plan *plan, int32_t nframes, size_t *bytes);
int  csic_rice_pack_device(csic_plan *plan, const void *d_bits, int32_t nframes, void *d_coded, uint64_t *d_sizes,
                           void *d_workspace, size_t workspace_bytes, void *hip_stream);
int  csic_rice_unpack_device(csic_plan *plan, const void *d_coded, int32_t nframes, void *d_bits, void *hip_stream);
const char *csic_rice_kernel_name(const csic_plan *plan);

/* ---- lossless rANS coding of the bit planes (csic_rans_*) -------------------------------------------------------------------------
 * A Golomb-Rice code spends at least one bit on every sample of a group that is not all zero; where the entropy of the residuals is
 * below one bit per sample the Rice coding cannot follow it.  This coding (CSIC_CODING_RANS) is a table-driven range coder (rANS) with
 * one static frequency table per plane and frame: it reaches the `ideal` figure of csic_code_stats_* up to its tables and stream
 * flushes.  It is interleaved over the 64 lanes of a wave and cut into independent blocks behind a directory, so there is still no
 * serial bit stream across the frame.  Coding ids 2 and 4 were never written and stay refused.
 *
 * Carried over from the group coding, word for word: the input is one CSIC_FMT_PLANAR_BITS frame; planes, q_p, n_p, the groups of 32
 * (G_p of them), anchor_g, e_j, s_j and the folded u_j (slots j = 1 .. 31) are as above; the last group is completed with the plane's
 * last real code (so its slots behind the last sample hold u_j = 0, and are coded); bits beyond sample n_p - 1 are never read into a
 * value; bit order is LSB first, every section starts at a multiple of 4 and every padding bit is 0.
 *
 * Model, per plane and frame.  M = 4096.  N = 31 G_p coded slots; c_s = how many of them hold the value s, s = 0 .. 2^q - 1.  The
 * frequencies f_s, with sum_s f_s = M exactly, f_s >= 1 where c_s > 0 and f_s = 0 where c_s = 0, come from the scaling rule:
 *     1. f_s = 0 if c_s = 0, else max(1, floor(c_s M / N)).
 *     2. d = M - sum_s f_s.  If d > 0, d is added to f_t, t = the s with the largest c_s (the smallest such s on a tie).
 *     3. If d < 0, -d times: 1 is taken off f_t, t = the s with the currently largest f_s (the smallest such s on a tie).  (That f_t is
 *        above M / 2^q >= 16: no frequency falls below 1.)
 * cum_s = sum of f_r over r < s.  The rule is the encoder's; decoding depends only on the stored table.
 *
 * State.  A stream's state x is 32 bits, L = 2^16 <= x < 2^32, renormalised in 16-bit words.
 *     decode a symbol   slot = x & (M - 1); s = the symbol with cum_s <= slot < cum_s + f_s; x = f_s (x >> 12) + slot - cum_s;
 *                       then, if x < L, x = (x << 16) | the stream's next word
 *     encode a symbol   (the exact inverse) if x >= f_s << 20: emit the word x & 0xffff, x = x >> 16;
 *                       then x = ((x / f_s) << 12) + (x mod f_s) + cum_s
 * At most one word moves per symbol.  A symbol with f_s = M codes in zero bits: x does not change.  The encoder starts every stream at
 * x = L and codes the stream's symbols in the reverse of the decode order; what it ends with is the stream's stored state.
 *
 * Blocks and interleave.  Plane p has B_p = ceil(G_p / 1024) blocks of 1024 consecutive groups; a frame's blocks are numbered Y, then
 * Cb, then Cr; NB = sum_p B_p.  A block has 64 streams; stream l owns those of the groups 1024 b + 64 i + l, i = 0 .. 15, that exist:
 * min(64, groups of the block) streams own a group.  Decode runs the steps t = 0 .. 495 with i = t / 31 and j = 1 + t mod 31: at step t
 * every stream whose group i exists decodes slot j of that group; the streams that renormalise at that step then take their words from
 * the block's word string, one each, in ascending stream order.  Every stream starts from its stored state and ends at exactly L.
 *
 * Sections, in this order:
 *     1. tables of Y, Cb, Cr    2^q_p uint16: f_0, f_1, ...
 *     2. anchors of Y, Cb, Cr   exactly as in the group coding
 *     3. directory              NB + 1 uint32: bits 0 .. 30 of dir[i] = the dword offset of block i's chunk from payload_offset, bit
 *                               31 set = the chunk is raw; dir[0] has offset 0; dir[NB] = the number of payload dwords, bit 31 clear
 *     4. payload                one chunk per block, back to back
 *          rANS chunk   the stored states of the streams that own a group, one uint32 each in stream order, then the word string
 *                       (uint16 each, word k in bytes [2 k, 2 k + 2) behind the states), zero-padded to a dword
 *          raw chunk    for each group of the block in order 31 q bits, u_j at bits [(j - 1) q, j q) of the group's run; runs
 *                       bit-contiguous, zero-padded to a dword: ceil(31 q groups / 32) dwords
 *     The encoder takes the raw chunk iff it is strictly smaller than the rANS chunk: no chunk is longer than its block's raw chunk.
 *     fixed_bytes = the sum of sections 1 to 3              coded_bytes = fixed_bytes + 4 * dir[NB]
 *     bound_bytes = the next multiple of 256 at or above fixed_bytes + the raw chunks of all blocks
 * Worked vector, one plane alone: q = 3, codes 1,2,3,4,5,6,7,0 -> u_1 .. u_7 = 2, the other 24 slots 0; f_0 = 3172, f_2 = 924; one
 * stream with the stored state 0x00e98cc8, which takes its one word 0x9dd4 at step t = 3; the raw chunk would be 3 dwords:
 *     table 64 0c 00 00 9c 03 00 00 00 00 00 00 00 00 00 00, anchors 01 00 00 00, directory 00 00 00 00 02 00 00 00,
 *     payload c8 8c e9 00 d4 9d 00 00
 *
 * Host codec (no GPU; parameters and statuses as for csic_pack_*):
 *   csic_rans_layout_of   : groups, blocks, section offsets and sizes of a coded frame of these parameters.
 *   csic_rans_pack_host   : as csic_pack_host, capacity rule included.
 *   csic_rans_unpack_host : as csic_unpack_host.  The input is untrusted; CSIC_EFORMAT, nothing written, for: a table that does not
 *                         sum to M; a padding bit that is not 0 (anchors, a raw chunk, the padding word of a word string); dir[0] with
 *                         an offset other than 0; offsets that decrease; a flag on dir[NB]; a raw chunk that is not exactly its size; a
 *                         rANS chunk shorter than its states or longer than the block's raw chunk; a stored state below L; a word
 *                         string that is not consumed exactly (one zero padding word allowed); a stream that does not end at L;
 *                         coded_bytes other than fixed_bytes + 4 dir[NB].  Whether the table is the scaling rule's, or the raw
 *                         decision the encoder's, is not checked.
 * Device codec (gfx950), with the argument lists, alignment rules, refusals before any device is touched, asynchrony and
 * capturability of csic_rice_*:
 *   csic_rans_workspace_bytes : what csic_rans_pack_device needs: per frame two uint32 per block and 256 uint32 per plane.
 *   csic_rans_pack_device : in stream order a kernel that clears the counts, a histogram pass (which stores the anchors), one
 *                         table launch, a sizing pass (one wave per block runs the encoder without
 *                         storing), the scan of the group coding over the blocks' sizes, and the emit pass (one wave per block
 *                         assembles its chunk in LDS, words placed from the end, and stores it and its directory entry).
 *   csic_rans_unpack_device : ONE pass, no workspace: one wave per block builds the slot table in LDS, takes its chunk and walks the
 *                         496 steps.  It does NOT validate: directory offsets are clamped to bound_bytes, a chunk to its block's raw
 *                         size, table entries so that no slot leaves the table, a word behind the chunk reads as 0.  Whatever the
 *                         bytes, nothing outside a frame's bound_bytes is read and nothing outside the three payload ranges written.
 *                         Validate untrusted input on the host.
 *   csic_rans_kernel_name : "k_rans<q6,5,5,nt>". */
#define CSIC_CODING_RANS   5   /* the rANS coding above; ids 2 and 4 are never written    */
typedef struct csic_rans_layout {
    int64_t groups[3];             /* G_p                                                              */
    int64_t blocks[3];             /* B_p, blocks of 1024 groups                                       */
    int64_t tables_offset[3];      /* byte offsets of the sections inside a coded frame               */
    int64_t anchors_offset[3];
    int64_t directory_offset;      /* sum_p B_p + 1 uint32                                             */
    int64_t payload_offset;        /* = fixed_bytes                                                    */
    int64_t fixed_bytes;
    int64_t bound_bytes;           /* multiple of 256: the distance of coded frames in device memory   */
} csic_rans_layout;
int  csic_rans_layout_of(const csic_params *p, csic_rans_layout *layout);
int  csic_rans_pack_host(const csic_params *p, const void *bits_frame, void *coded, size_t capacity, uint64_t *coded_bytes);
int  csic_rans_unpack_host(const csic_params *p, const void *coded, size_t coded_bytes, void *bits_frame);
int  csic_rans_workspace_bytes(const csic_plan *plan, int32_t nframes, size_t *bytes);
int  csic_rans_pack_device(csic_plan *plan, const void *d_bits, int32_t nframes, void *d_coded, uint64_t *d_sizes,
                           void *d_workspace, size_t workspace_bytes, void *hip_stream);
int  csic_rans_unpack_device(csic_plan *plan, const void *d_coded, int32_t nframes, void *d_bits, void *hip_stream);
const char *csic_rans_kernel_name(const csic_plan *plan);

/* ---- temporal delta coding of frame sequences (csic_delta_*) ------------------------------------------------------------------------
 * Both codings above code every frame on its own.  This layer sits in front of them: it turns a sequence of CSIC_FMT_PLANAR_BITS
 * frames into a sequence of DIFFERENCE frames of the same layout, which either coding then codes as it codes any frame, and one small
 * map per frame.  It is lossless.  Prediction across the groups of a frame would need a scan over a plane (csic_rows_*, below, predicts
 * from the row above inside bands of 16 steps instead); across frames the
 * dependency is per sample -- sample i of frame k depends on sample i of frame k - 1 only -- so encode and decode stay one lane per
 * group.  There is no motion compensation here: content that stays in place gains, a pan gains nothing and loses the map at most; the
 * layer for content that moves is csic_mc_*, below.
 *
 * Input: frames x_0 .. x_(n - 1) of one parameter set and gop >= 1.  Frame k is a KEY frame iff k % gop == 0; every other frame is a
 * DELTA frame against x_(k - 1), the source frame itself (the coding is lossless: the decoder has it exactly).  Planes, q_p, n_p and the
 * groups of 32 (G_p = ceil(n_p / 32)) are those of csic_pack_*.
 *
 * For group g of a delta frame, with c the frame's codes and r the previous frame's, slot by slot:
 *     d_i     = (c_i - r_i) mod 2^q
 *     cost(v) = the sum over the group's real slots j >= 1 of u_j, the folded, centred left residuals of csic_pack_* computed over the
 *               values v; slots behind the plane's last sample add nothing (a group of one sample costs 0 either way)
 *     t_g     = 1 (inter) iff cost(d) < cost(c); a tie is intra
 * The group of the difference frame D_k holds d where t_g = 1 and c where t_g = 0.  D_k is a PLANAR_BITS frame: the bits behind a
 * plane's last sample are 0, bytes outside the three payload ranges are not written.  For a key frame D_k = x_k.
 *
 * The map of a frame has three sections, Y, Cb, Cr, of 4 * ceil(G_p / 32) bytes each: bit g of a section (LSB first) is t_g, padding
 * bits are 0, the map of a key frame is all zeros.  map_bytes is the sum of the sections, map_stride the next multiple of 256: the
 * distance between the maps of consecutive frames in a buffer of maps, on the host and on the device.  A buffer of `nframes` maps
 * needs (nframes - 1) * map_stride + map_bytes bytes; bytes of a map behind its map_bytes are not touched.
 *
 * Inverse, frame after frame from each key frame: c_i = (d_i + r_i) mod 2^q where t_g = 1, c_i = d_i otherwise.
 *
 * Worked vectors, one plane alone, q = 3 (the bytes are the plane's payload in the bit layout):
 *     identical frames   c = r = 1,2,3,4,5,6,7,0: d = 0 x 8, cost(d) = 0 < cost(c) = 14 -> map 01 00 00 00, D = 00 00 00
 *     a tie              c = 0,1 and r = 1,1: d = 7,0, cost(d) = 2 = cost(c) -> intra, map 00 00 00 00, D = 08
 *     the wrap           c = 0,4,0 and r = 7,3,7 (2^q - 1 under a 0): d = 1,1,1, cost(d) = 0 < cost(c) = 14 -> map 01 00 00 00,
 *                        D = 49 00; back: (1 + 7) mod 8 = 0
 *     a ragged group     q = 2, n = 34: group 1 has the two samples 32, 33.  c = 3,0 and r = 2,3 there: d = 1,1, cost(d) = 0 <
 *                        cost(c) = 2 -> bit 1 of the map; the 30 slots behind sample 33 take no part and are stored as zero bits
 *
 * Host codec (no GPU; parameters and statuses as for csic_pack_*):
 *   csic_delta_layout_of : groups, the sections' offsets, map_bytes and map_stride of these parameters.
 *   csic_delta_host      : frames (frame_bytes apart) -> diff (frame_bytes apart) and maps (map_stride apart).
 *   csic_undelta_host    : the inverse.  The maps are untrusted: a padding bit that is set or a non-zero map of a key frame gives
 *                          CSIC_EFORMAT; a refused call writes nothing.  (The difference frames need no check: any codes are codes.)
 * Device codec (gfx950): asynchronous on `hip_stream`, no allocation, no synchronisation, no workspace, hipGraph-capturable; one launch
 * per run of planes of one width, grid z over the ceil(nframes / gop) runs of frames that begin with a key frame; a lane walks its
 * group through a run with the previous frame's group in registers, so every frame is read once and written once.
 *   csic_delta_device    : d_frames -> d_diff and d_maps; the source is only read.
 *   csic_undelta_device  : the inverse.  It does NOT validate and has nothing to clamp: any map bit decodes to valid codes; a key
 *                          frame's map is ignored.
 *   csic_delta_kernel_name : "k_delta<q6,5,5,nt>", as csic_pack_kernel_name.
 * For all four calls: diff == frames, exactly in place, is allowed; any other overlap of the frames, the difference frames and the
 * maps is CSIC_EINVAL_SIZE, as are nframes outside 1..65535, gop < 1 (a gop above nframes means one key frame) and, on the device, a
 * buffer that is not 256-byte aligned.  NULL arguments: CSIC_EINVAL_NULL; parameters the container does not take: csic_validate's
 * status -- all before any device is touched.  CSIC_TUNE_NONTEMPORAL applies to the accesses of the frames; the other knobs are ignored. */
typedef struct csic_delta_layout {
    int64_t groups[3];             /* G_p                                                              */
    int64_t map_offset[3];         /* byte offsets of the sections inside a map                        */
    int64_t map_bytes;             /* sum_p 4 * ceil(G_p / 32)                                         */
    int64_t map_stride;            /* multiple of 256: the distance of maps in a buffer of maps        */
} csic_delta_layout;
int  csic_delta_layout_of(const csic_params *p, csic_delta_layout *layout);
int  csic_delta_host(const csic_params *p, const void *frames, int32_t nframes, int32_t gop, void *diff, void *maps);
int  csic_undelta_host(const csic_params *p, const void *diff, const void *maps, int32_t nframes, int32_t gop, void *frames);
int  csic_delta_device(csic_plan *plan, const void *d_frames, int32_t nframes, int32_t gop, void *d_diff, void *d_maps, void *hip_stream);
int  csic_undelta_device(csic_plan *plan, const void *d_diff, const void *d_maps, int32_t nframes, int32_t gop, void *d_frames,
                         void *hip_stream);
const char *csic_delta_kernel_name(const csic_plan *plan);

/* ---- motion-compensated delta coding of frame sequences (csic_mc_*) -----------------------------------------------------------------
 * A second temporal layer beside csic_delta_*, for content that moves: the same inputs, the same kind of outputs -- a sequence of
 * DIFFERENCE frames of the CSIC_FMT_PLANAR_BITS layout, which either coding codes as it codes any frame, and one map per frame -- but
 * a group is predicted from the previous frame DISPLACED by one of up to 15 offsets that the frame's plane has chosen for itself.  It
 * is lossless.  The map costs 4 bits per group where csic_delta_*'s costs 1, so content that stays put is better off there: the layer
 * is opt-in.
 *
 * Planes, q_p, n_p, the groups of 32 (G_p), key and delta frames and gop are those of csic_delta_*.  Plane p has a row width w_p:
 * y_width for Y, chroma_width for Cb and Cr (csic_planar_layout).
 *
 * DISPLACEMENT.  A displacement is a flat signed sample offset s (int32).  With r the previous source frame's codes of the plane, the
 * reference of sample i is  ref_s(i) = r[clamp(i + s, 0, n_p - 1)],  i + s computed in 64 bits.  Rows wrap into their neighbours at
 * the plane's edges; that is accepted, because the coding is lossless whatever the predictor.
 *
 * CANDIDATES.  The range R is 0 .. 7.  The candidates are all (dy, dx) of [-R, R]^2, ranked by (|dx| + |dy|, dy, dx) ascending -- rank
 * 0 is the zero vector, then (-1, 0), (0, -1), (0, 1), (1, 0), (-2, 0), (-1, -1), ... --, each with s = dy * w_p + dx.
 *
 * COST AND VOTE.  cost_s(g) is cost() of csic_delta_* over d_i = (c_i - ref_s(i)) mod 2^q on the group's real slots.  Every group of
 * a delta frame votes for the lowest-ranked candidate that attains its minimal cost.
 *
 * TABLE.  Each plane of each delta frame has a table of 16 int32 words: word 0 is T, the number of entries; word 1 is 0, the zero
 * vector, always; words 2 .. T hold s of the non-zero candidates that got votes, ordered by votes descending, then rank ascending, at
 * most 14 of them (T = 1 + min(14, their number)); unused words are 0.
 *
 * CHOICE.  A group takes the lowest t of 1 .. T whose cost_(word t)(g) is minimal over the table.  It is INTER with nibble t iff that
 * cost is below cost(c), the cost of its own codes; a tie is intra, nibble 0, as in csic_delta_*.  The group of the difference frame
 * holds d (against word t) where it is inter and c where it is intra; the bits behind a plane's last sample are 0, bytes outside the
 * three payload ranges are not written.  For a key frame D_k = x_k.
 *
 * MAP.  Three tables of 64 bytes at byte offsets 0, 64 and 128 (Y, Cb, Cr; little endian), followed by three nibble sections of
 * 4 * ceil(G_p / 8) bytes each: group g is nibble g % 8 of dword g / 8, least significant first; padding nibbles are 0.  map_bytes is
 * 192 + the sections, map_stride map_bytes rounded up to a multiple of 256: the distance between the maps of consecutive frames in a
 * buffer of maps, which needs (nframes - 1) * map_stride + map_bytes bytes; bytes of a map behind its map_bytes are not touched.  The
 * map of a key frame is all zeros.
 *
 * INVERSE, frame after frame from each key frame: c_i = (d_i + r[clamp(i + word t)]) mod 2^q where the group's nibble is t >= 1,
 * c_i = d_i where it is 0; r is the decoded previous frame.
 *
 * Worked vectors, the Y plane of an 8 x 1 frame (w = 8, n = 8, one group), q = 3, r = 1,2,3,4,5,6,7,0 (bytes as for csic_delta_*):
 *     a pan, R = 1      c = 1,1,2,3,4,5,6,7 = r one sample to the right, the edge repeated.  Candidate (0, -1), s = -1, rank 2, gives
 *                       d = 0 x 8 at cost 0 and is the only one that does: it gets the vote.  Table 2, 0, -1, 0 x 13 (bytes 02 00 00 00
 *                       00 00 00 00 ff ff ff ff 00 ...).  Word 1: d = 0,7,7,7,7,7,7,7, cost 1; word 2: cost 0; cost(c) = 12: inter,
 *                       nibble 2, section 02 00 00 00, D = 00 00 00
 *     the same, R = 0   the zero vector alone: table 1, 0 x 15; cost 1 < 12: nibble 1, section 01 00 00 00, D = f8 ff ff
 *     clamping          c = 1 x 8, R = 1: (-1, 0), s = -8, rank 1, reads r[0] = 1 everywhere, d = 0 x 8, cost 0; so do (-1, -1) and
 *                       (-1, 1) at ranks 5 and 6: the lowest rank gets the vote.  Table 2, 0, -8, 0 x 13; cost(c) = 0: a tie, intra,
 *                       nibble 0, section 00 00 00 00, D = 49 92 24 (the codes)
 *     identical frames  c = r, R = 1: the zero vector gets the vote, table 1, 0 x 15, nibble 1, D = 00 00 00 -- what csic_delta_*
 *                       stores, with R = 0 always: at R = 0 the inter / intra choices are exactly csic_delta_*'s
 *
 * Host codec (no GPU; parameters and statuses as for csic_delta_*):
 *   csic_mc_layout_of    : groups, row widths, the tables' and the sections' offsets, map_bytes, map_stride and the device codec's
 *                          workspace bytes per frame of these parameters.
 *   csic_mc_delta_host   : frames (frame_bytes apart) -> diff (frame_bytes apart) and maps (map_stride apart), range R.
 *   csic_mc_undelta_host : the inverse.  The maps are untrusted: T > 15, a nibble above T, a non-zero unused table word, word 1 != 0
 *                          when T >= 1, a set padding nibble or a non-zero map of a key frame gives CSIC_EFORMAT; a refused call writes
 *                          nothing.  Any int32 displacement is valid, because it clamps.
 * Device codec (gfx950): asynchronous on `hip_stream`, no allocation, no synchronisation, hipGraph-capturable.
 *   csic_mc_delta_device   : d_frames -> d_diff and d_maps; the source is only read.  The reference is the SOURCE frame, so all frames
 *                            are independent: frames on grid z.  d_workspace: at least nframes * workspace_frame_bytes bytes, 256-byte
 *                            aligned, the vote counters; its contents before and after are of no interest.
 *   csic_mc_undelta_device : the inverse.  Frame k needs all of frame k - 1: one launch per step of a run, min(gop, nframes) launches
 *                            in a line, grid z over the runs; no workspace.  It does NOT validate: any nibble reads one of the 16
 *                            words, any word clamps; a key frame's map is ignored.
 *   csic_mc_kernel_name    : "k_mc_delta<q6,5,5,nt>", as csic_delta_kernel_name.
 * For all four calls: nframes outside 1..65535, gop < 1, ANY overlap of the frames, the difference frames and the maps -- in place is
 * NOT allowed: a group reads other groups of the previous frame -- and, on the device, a buffer that is not 256-byte aligned or a
 * workspace that is too small are CSIC_EINVAL_SIZE; so is a range outside 0..7.  NULL arguments: CSIC_EINVAL_NULL; parameters the
 * container does not take: csic_validate's status -- all before any device is touched.  CSIC_TUNE_NONTEMPORAL applies to the accesses
 * that stream -- a frame's own groups and the difference frames --; the reference windows are read several times and stay cached. */
typedef struct csic_mc_layout {
    int64_t groups[3];             /* G_p                                                              */
    int64_t width[3];              /* w_p                                                              */
    int64_t table_offset[3];       /* 0, 64, 128: byte offsets of the tables inside a map              */
    int64_t map_offset[3];         /* byte offsets of the nibble sections inside a map                 */
    int64_t map_bytes;             /* 192 + sum_p 4 * ceil(G_p / 8)                                    */
    int64_t map_stride;            /* multiple of 256: the distance of maps in a buffer of maps        */
    int64_t workspace_frame_bytes; /* csic_mc_delta_device's workspace, per frame                      */
} csic_mc_layout;
int  csic_mc_layout_of(const csic_params *p, csic_mc_layout *layout);
int  csic_mc_delta_host(const csic_params *p, const void *frames, int32_t nframes, int32_t gop, int32_t range, void *diff, void *maps);
int  csic_mc_undelta_host(const csic_params *p, const void *diff, const void *maps, int32_t nframes, int32_t gop, void *frames);
int  csic_mc_delta_device(csic_plan *plan, const void *d_frames, int32_t nframes, int32_t gop, int32_t range, void *d_diff, void *d_maps,
                          void *d_workspace, size_t workspace_bytes, void *hip_stream);
int  csic_mc_undelta_device(csic_plan *plan, const void *d_diff, const void *d_maps, int32_t nframes, int32_t gop, void *d_frames,
                            void *hip_stream);
const char *csic_mc_kernel_name(const csic_plan *plan);

/* ---- row prediction of the bit planes (csic_rows_*) ---------------------------------------------------------------------------------
 * Every coding above predicts a sample from its left neighbour inside a flat group of 32; none knows that a plane has rows.  This layer
 * sits in front of them as csic_delta_* does: it turns a CSIC_FMT_PLANAR_BITS frame x into a DIFFERENCE frame D of the same layout,
 * which any coding codes as it codes any frame, and one small map.  A group of D holds either the group's codes or -- where the row
 * above predicts the group better than the left neighbour -- values whose LEFT residuals are the differences against the row above.  It
 * is lossless.  A frame stands alone: there is no gop, and frames of a call are independent.
 *
 * Planes, q_p, n_p and the groups of 32 (G_p = ceil(n_p / 32)) are those of csic_pack_*; a plane's row width w is csic_mc_*'s w_p.
 * Per plane:  K = floor(w / 32)  and  S = 32 * K * CSIC_ROWS_BAND.  A plane with K = 0 takes no part: its map bits are 0 and its D is
 * x.  BANDS are the flat sample ranges [b S, (b + 1) S): they begin on group boundaries and, like csic_mc_*'s displacements, do not
 * care about row ends.
 *
 * REFERENCE.   ref(i) = x[i - w] if i - w >= S * floor(i / S), else 0: the first w samples of a band restart.
 *              u_i    = (x_i - ref(i)) mod 2^q
 * CHOICE, per group g, over its real slots (slots behind the plane's last sample add nothing, as in csic_delta_*):
 *     cost_left = csic_delta_*'s cost(x), the sum over the slots j >= 1 of the folded, centred left residuals of the codes
 *     cost_up   = the sum over the slots j >= 1 of the folded, centred u_j -- u itself, not its left residual
 *     t_g       = 1 iff cost_up < cost_left; a tie is 0 (a constant plane has an all-zero map).  Groups whose references are all 0
 *                 follow the same rule.
 * DIFFERENCE GROUP.  Where t_g = 0 it holds x.  Where t_g = 1 it holds v_j = (u_0 + ... + u_j) mod 2^q: every coding left-predicts
 * inside a group, so the residual it sees at slot j >= 1 is exactly u_j and its anchor is u_0 -- the layer composes with
 * CSIC_CODING_GROUPS, _RICE and _RANS unchanged.  Bits behind a plane's last sample are 0; bytes outside the payload ranges are not
 * written.
 * MAP.  csic_delta_*'s layout exactly: three sections of 4 * ceil(G_p / 32) bytes, bit g of a section (LSB first) is t_g, padding bits
 * are 0; map_bytes is their sum, map_stride the next multiple of 256, the distance of the maps of consecutive frames.
 * INVERSE, in increasing i.  t_g = 1: u_0 = v_0, u_j = (v_j - v_(j - 1)) mod 2^q, x_i = (u_i + ref(i)) mod 2^q.  t_g = 0: x = D.
 *
 * DECODING ORDER.  Inside a band, step s is the groups [s K, (s + 1) K).  Since 32 K <= w, a group of step s refers only to samples of
 * steps s - 1 and s - 2: with delta = w - 32 K (0 .. 31), slots j >= delta of band-local group s K + k refer to group (s - 1) K + k,
 * slots j < delta to the group before that one.  Bands are independent, a band is CSIC_ROWS_BAND dependent steps, and the encoder has
 * no dependency at all: its references are source samples.
 *
 * Worked vectors, one plane alone, w = 32 and two rows unless said otherwise (bytes: the plane's payload in the bit layout):
 *     a row repeated   q = 3, both rows 1,2,3,4,5,6,7,0 four times.  Group 0 has no reference: cost_up = 110 > cost_left = 62, it
 *                      stays.  Group 1: u = 0 x 32, cost_up = 0 < 62 -> map 02 00 00 00, D = d1 58 1f x 4, then 00 x 12
 *     a tie            q = 3, row 0 all 0, row 1 is 31 zeros and a 1: cost_up = 2 = cost_left -> map 00 00 00 00, D = x
 *     the wrap         q = 3, row 0 is 7,3 sixteen times, row 1 is 0,4 sixteen times (2^q - 1 above a 0): u = 1 x 32, cost_up = 62 <
 *                      cost_left = 217 -> v = 1,2,3,4,5,6,7,0 four times: group 1 of D = d1 58 1f x 4; back: (1 + 7) mod 8 = 0.
 *                      (Group 0 is taken too, against references of 0: cost_up = 111 < 217, v = 7,2,1,4,3,6,5,0 four times; map 03.)
 *     a ragged group   q = 2, n = 34: row 0 is 1,2,3,0 eight times, group 1 has the two samples 1,2.  u = 0,0, cost_up = 0 <
 *                      cost_left = 2 -> bit 1 of the map; the 30 slots behind sample 33 take no part and are stored as zero bits.
 *                      (Group 0: cost_up = 46 < 62, v = 1,3,2,2,3,1,0,0 eight times; map 03 00 00 00, D = ad 07 x 4, then 00.)
 *     w = 33           q = 3, x_i = 5 (i mod 33) mod 8 for i < 66: K = 1, delta = 1.  Sample 32 ends row 0 and has no reference;
 *                      sample 33 + j refers to sample j: slot 0 of group 1 is on its own, its slots j >= 1 refer to group 0, and group
 *                      2 (samples 64, 65) refers to slots 31 of group 0 and 0 of group 1.  u = 0 from sample 32 on -> map 07 00 00 00
 *                      (group 0, against 0: 112 < 155), D = e8 ad 85 cc e4 17 twice, then 00 x 13
 *
 * Host codec (no GPU; parameters and statuses as for csic_delta_*):
 *   csic_rows_layout_of : groups, w, K, S, the sections' offsets, map_bytes and map_stride of these parameters.
 *   csic_rows_host      : frames (frame_bytes apart) -> diff (frame_bytes apart) and maps (map_stride apart).
 *   csic_unrows_host    : the inverse.  The maps are untrusted: a padding bit that is set, or a set bit in a plane with K = 0, gives
 *                         CSIC_EFORMAT; a refused call writes nothing.
 * Device codec (gfx950): asynchronous on `hip_stream`, no allocation, no synchronisation, no workspace, hipGraph-capturable; one launch
 * per run of planes of one bit width, frames on grid z.
 *   csic_rows_device    : d_frames -> d_diff and d_maps, one lane per group; the source is only read.
 *   csic_unrows_device  : the inverse, one workgroup per band, lane k walks the band-local groups k, K + k, ... down the steps.  It
 *                         does NOT validate and has nothing to clamp: any map bit decodes to valid codes; a bit of a plane with K = 0
 *                         is ignored.
 *   csic_rows_kernel_name : "k_rows<q6,5,5,nt>", as csic_delta_kernel_name.
 * Forward calls: ANY overlap of the frames, the difference frames and the maps is CSIC_EINVAL_SIZE -- a group reads other groups of
 * the source.  Inverse calls: diff == frames, exactly in place, is allowed, any other overlap is CSIC_EINVAL_SIZE.  nframes outside
 * 1..65535 and, on the device, a buffer that is not 256-byte aligned: CSIC_EINVAL_SIZE.  NULL arguments: CSIC_EINVAL_NULL; parameters
 * the container does not take: csic_validate's status -- all before any device is touched.  CSIC_TUNE_NONTEMPORAL applies to the
 * accesses of the frames. */
#define CSIC_ROWS_BAND 16
typedef struct csic_rows_layout {
    int64_t groups[3];             /* G_p                                                              */
    int64_t width[3];              /* w_p                                                              */
    int64_t k[3];                  /* K = floor(w_p / 32); 0: the plane takes no part                  */
    int64_t band[3];               /* S = 32 * K * CSIC_ROWS_BAND samples                              */
    int64_t map_offset[3];         /* byte offsets of the sections inside a map                        */
    int64_t map_bytes;             /* sum_p 4 * ceil(G_p / 32)                                         */
    int64_t map_stride;            /* multiple of 256: the distance of maps in a buffer of maps        */
} csic_rows_layout;
int  csic_rows_layout_of(const csic_params *p, csic_rows_layout *layout);
int  csic_rows_host(const csic_params *p, const void *frames, int32_t nframes, void *diff, void *maps);
int  csic_unrows_host(const csic_params *p, const void *diff, const void *maps, int32_t nframes, void *frames);
int  csic_rows_device(csic_plan *plan, const void *d_frames, int32_t nframes, void *d_diff, void *d_maps, void *hip_stream);
int  csic_unrows_device(csic_plan *plan, const void *d_diff, const void *d_maps, int32_t nframes, void *d_frames, void *hip_stream);
const char *csic_rows_kernel_name(const csic_plan *plan);

/* ---- .csic files: the compressed frames on disk (host only, usable without a GPU) --------------------------------------------
 * A container holds `nframes` CSIC_FMT_PLANAR_BITS frames of one parameter set: the only thing this library writes to a file that
 * is smaller than its input (a 6/5/5 4:2:0 frame: 1.06 bytes per pixel at factor 1; group-coded, version 3 below, less).  Version 1,
 * every integer little endian:
 *
 *     offset  size                     content
 *          0     4                     magic 43 53 49 43 ("CSIC")
 *          4     4                     uint32 version = 1
 *          8     4                     uint32 nframes, 1 .. 65535
 *         12     4                     uint32 CRC-32 (zlib's crc32) of bytes [16, end of file)
 *         16    64                     csic_params as 16 int32 in the struct's field order; out_format = CSIC_FMT_PLANAR_BITS,
 *                                      in_format = CSIC_FMT_ARGB8888
 *         80     nframes * payload     per frame: the Y plane's y_bytes, then cb_bytes, then cr_bytes, back to back
 *                                      (csic_planar_bits_layout_of; payload = payload_bytes)
 *
 * `frames` is what csic_process_host and csic_pipeline_collect hand out for a PLANAR_BITS plan: nframes frame buffers, frame_bytes
 * apart, in host memory.  Only the three payload ranges of each buffer are written -- its padding is undefined and never reaches
 * the file -- and csic_container_read zeroes every byte of the buffers outside those ranges, so what it returns is deterministic.
 *   csic_container_write   : stores out_format = CSIC_FMT_PLANAR_BITS whatever p->out_format says; fails with csic_validate's status
 *                            when the parameters are invalid or p->in_format is not ARGB; nframes outside 1 .. 65535: CSIC_EINVAL_SIZE.
 *   csic_container_info_of : header, parameters and length of a file (everything csic_container_read checks except the CRC).
 *   csic_container_read    : frames_bytes must equal nframes * frame_bytes (CSIC_EINVAL_SIZE otherwise; ask csic_container_info_of).
 * CSIC_EFORMAT: bad magic, a version other than 1, 3, 4, 5, 6, 7 or 8, nframes out of range, parameters that fail csic_validate (or are not
 * PLANAR_BITS), a length other than 80 + nframes * payload_bytes, a CRC mismatch.  CSIC_EIO: the file cannot be opened, read or
 * written.  NULL arguments: CSIC_EINVAL_NULL.
 *
 * Version 3 holds the frames group-coded (csic_pack_*, CSIC_CODING_GROUPS); version 2 was never written and stays refused.  Bytes
 * 0 .. 79 are as in version 1 with version = 3, the CRC covers [16, end of file) as well, and the body is
 *
 *         80     4                     uint32 coding = 1 (CSIC_CODING_GROUPS)
 *         84     4                     uint32 reserved = 0
 *         88     8 * nframes           uint64 coded_bytes of each frame
 *         88 + 8 * nframes             the coded frames back to back, each exactly its coded_bytes
 *
 *   csic_container_write_ex    : coding = CSIC_CODING_RAW writes what csic_container_write writes, byte for byte; CSIC_CODING_GROUPS
 *                                packs every frame on the host (csic_pack_host) and writes version 3; CSIC_CODING_RICE and
 *                                CSIC_CODING_RANS: versions 4 and 7 below; another coding (2 and 4 among them): CSIC_EINVAL_FORMAT.
 *   csic_container_write_coded : version 3 from frames that are packed already (csic_pack_device's output copied to the host, say):
 *                                frame k is coded[k * stride_bytes, + sizes[k]).  Every frame is validated as csic_unpack_host would
 *                                before anything is written (CSIC_EFORMAT); sizes[k] > stride_bytes: CSIC_EINVAL_SIZE.
 *   csic_container_read        : reads both versions into PLANAR_BITS frame buffers, padding zeroed.
 *   csic_container_info_of     : reports version 3; payload_bytes keeps its meaning, the raw payload per frame.
 *   csic_container_coded_sizes : the stored bytes of each frame into sizes[0, n), n = the file's nframes (CSIC_EINVAL_SIZE otherwise):
 *                                the table of a version-3 file, payload_bytes for every frame of a version-1 file.
 * CSIC_EFORMAT for a version-3 file, beyond the above: coding != 1, reserved != 0, a coded_bytes below fixed_bytes, above fixed_bytes +
 * 4 sum_p G_p q_p or not a multiple of 4, a length other than 88 + 8 nframes + the sum of the table, any frame csic_unpack_host refuses.
 *
 * Version 4 is version 3's layout byte for byte with version = 4 and coding = 3 (CSIC_CODING_RICE): the frames are Rice-coded
 * (csic_rice_*).  A version / coding pair other than 3 / 1 or 4 / 3 is CSIC_EFORMAT; a version-4 file is refused in the cases of a
 * version-3 file, with the Rice coding's sizes (fixed_bytes .. fixed_bytes + 4 sum_p B_p (248 q_p + 1)) and csic_rice_unpack_host.
 *   csic_container_write_ex       : CSIC_CODING_RICE packs every frame on the host (csic_rice_pack_host) and writes version 4.
 *   csic_container_write_coded_ex : csic_container_write_coded for any of the three codings (CSIC_CODING_GROUPS, CSIC_CODING_RICE, or
 *                                   CSIC_CODING_RANS: version 7 below; another: CSIC_EINVAL_FORMAT); csic_container_write_coded keeps
 *                                   meaning CSIC_CODING_GROUPS.
 *   csic_container_read, csic_container_info_of, csic_container_coded_sizes read every version: 1, 3, 4, 5, 6 and 7.
 *
 * Version 5 holds a SEQUENCE: the frames go through the temporal layer (csic_delta_*) and their difference frames through one of the
 * two codings.  Bytes 0 .. 79 are as in version 1 with version = 5, the CRC covers [16, end of file), and the body is
 *
 *         80     4                     uint32 coding = 1 (CSIC_CODING_GROUPS) or 3 (CSIC_CODING_RICE)
 *         84     4                     uint32 gop, 1 .. 65535
 *         88     8 * nframes           uint64 stored bytes of each frame's record
 *         88 + 8 * nframes             the records back to back: a key frame (k % gop == 0) is its coded frame exactly as in version
 *                                      3 / 4; a delta frame is its map (map_bytes of csic_delta_layout_of) followed by the coded frame
 *                                      of its difference frame
 *
 *   csic_container_write_seq       : delta (csic_delta_host) and packing on the host, version 5 (CSIC_CODING_RANS: version 7 below).
 *                                    coding other than GROUPS, RICE or RANS: CSIC_EINVAL_FORMAT; gop outside 1 .. 65535: CSIC_EINVAL_SIZE.
 *   csic_container_write_coded_seq : version 5 from what the device made: coded difference frames coded[k * stride_bytes, + sizes[k])
 *                                    (sizes[k] is the coded frame's bytes, without the map) and the maps, map_stride apart (the maps of
 *                                    key frames are read too: they must be zero).  Every coded frame and every map is validated
 *                                    before anything is written (CSIC_EFORMAT); sizes[k] > stride_bytes or map_stride < map_bytes:
 *                                    CSIC_EINVAL_SIZE.
 *   csic_container_gop             : the gop of a version-5, -6 or -7 file; 1 for versions 1, 3 and 4 and for a version-7 file whose
 *                                    stored gop is 0 (every frame stands alone).
 *   csic_container_inter_groups    : counts[3 k + p] = the groups of plane p of frame k that are inter, the popcount of that section of
 *                                    the map; n must be 3 * nframes (CSIC_EINVAL_SIZE otherwise).  All zeros for versions 1, 3 and 4.
 *   csic_container_read resolves the chains on the host and returns the frames themselves; csic_container_info_of reports version 5;
 *   csic_container_coded_sizes gives the table (maps included).
 * CSIC_EFORMAT for a version-5 file, beyond the cases of versions 3 / 4 (with the sizes of the file's coding; a delta record holds
 * map_bytes more): a coding other than 1 or 3, a gop out of range, a delta record shorter than map_bytes + fixed_bytes, a padding bit
 * that is set in a map, any coded frame the coding's host decoder refuses.  Versions 1, 3 and 4 keep their behaviour.
 *
 * Version 6 is version 5 through the motion-compensated layer (csic_mc_*): the same layout, the maps are csic_mc_layout_of's (map_bytes
 * of that layout in front of every delta frame's coded difference frame), and the word at 80 is  coding | (R + 1) << 8  with R the range
 * 0 .. 7 and every other bit zero; the word at 84 is the gop.  A motion field of 0 -- what a version-5 body has there -- or above 8 is
 * CSIC_EFORMAT, so a version-5 body behind a version-6 header is refused at the header.
 *   csic_container_write_seq_ex       : csic_container_write_seq with csic_mc_delta_host at `range`: version 6.  range outside 0 .. 7:
 *                                       CSIC_EINVAL_SIZE.
 *   csic_container_write_coded_seq_ex : csic_container_write_coded_seq with the maps of csic_mc_delta_device, validated as
 *                                       csic_mc_undelta_host validates them: version 6.
 *   csic_container_motion             : the range of a version-6 file or of a version-7 file with a motion layer, -1 otherwise.
 *   csic_container_read, _info_of, _coded_sizes and _gop read version 6 as they read version 5; csic_container_inter_groups counts the
 *   nibbles that are not 0.  CSIC_EFORMAT beyond version 5's cases: the motion field, and whatever csic_mc_undelta_host refuses of a map.
 *
 * Version 7 holds everything that is rANS-coded (csic_rans_*, CSIC_CODING_RANS): frames that stand alone, a sequence through the
 * temporal layer, or a sequence through the motion-compensated layer.  Bytes 0 .. 79 are as in version 1 with version = 7, the CRC
 * covers [16, end of file), and the body is
 *
 *         80     4                     uint32  5 | F << 8 : the coding id and the motion field F, every other bit zero.  F = 0: no
 *                                      motion layer; F = R + 1 for the range R = 0 .. 7 of csic_mc_*
 *         84     4                     uint32 gop, 0 .. 65535.  0: every frame stands alone, no record holds a map, and F is 0
 *         88     8 * nframes           uint64 stored bytes of each frame's record
 *         88 + 8 * nframes             the records back to back.  gop = 0: each record is the frame's coded frame (csic_rans_pack_host's
 *                                      bytes).  gop >= 1: as in versions 5 (F = 0: the maps of csic_delta_layout_of) and 6 (F >= 1: the
 *                                      maps of csic_mc_layout_of): a key frame's record is its coded frame, a delta frame's its map
 *                                      followed by the coded frame of its difference frame
 *
 *   csic_container_write_ex, csic_container_write_coded_ex          : coding = CSIC_CODING_RANS writes gop = 0, F = 0.
 *   csic_container_write_seq, csic_container_write_coded_seq        : coding = CSIC_CODING_RANS writes the gop and F = 0.
 *   csic_container_write_seq_ex, csic_container_write_coded_seq_ex  : coding = CSIC_CODING_RANS writes the gop and F = range + 1.
 *       The refusals are those of the same calls with the other codings; the _coded writers validate every coded frame as
 *       csic_rans_unpack_host would, and every map as its layer's decoder would, before anything is written.
 *   csic_container_read, _info_of, _coded_sizes read version 7 as they read versions 3 to 6; csic_container_gop gives the stored gop,
 *   or 1 when it is 0; csic_container_motion gives F - 1 (so -1 without a motion layer); csic_container_inter_groups counts as for
 *   version 5 (F = 0) or 6 (F >= 1), and gives all zeros when the gop is 0.
 * CSIC_EFORMAT for a version-7 file, beyond the cases of versions 3 to 6 (with the rANS coding's sizes: fixed_bytes .. fixed_bytes + the
 * raw chunks of all blocks, plus map_bytes for a delta record): a coding id other than 5 in the low byte; F above 8 or any higher bit
 * set; a gop above 65535; F other than 0 with a gop of 0; any coded frame csic_rans_unpack_host refuses; a record that holds a map
 * where the gop says it has none, or none where it has one (refused by its size or by the decoders).  Coding id 5 under versions 3,
 * 4, 5 or 6 is CSIC_EFORMAT as well: those versions keep their codings, their bytes and their refusals.
 *
 * Version 8 holds frames that stand alone, each through the row-prediction layer (csic_rows_*) and then one of the three codings.
 * Bytes 0 .. 79 are as in version 1 with version = 8, the CRC covers [16, end of file), and the body is
 *
 *         80     4                     uint32  coding | 1 << 16 : the coding id 1, 3 or 5, and bit 16, the layer; every other bit zero
 *         84     4                     uint32  0
 *         88     8 * nframes           uint64 stored bytes of each frame's record
 *         88 + 8 * nframes             the records back to back: the frame's map (map_bytes of csic_rows_layout_of) followed by the
 *                                      coded frame of its difference frame
 *
 *   csic_container_write_rows       : the layer (csic_rows_host) and the coding on the host.  coding CSIC_CODING_RAW -- the layer gains
 *                                     nothing without a coder -- or any other than GROUPS, RICE, RANS: CSIC_EINVAL_FORMAT.
 *   csic_container_write_coded_rows : version 8 from what the device made: coded difference frames coded[k * stride_bytes, + sizes[k])
 *                                     (without the maps) and the maps, map_stride apart.  Every coded frame and every map is validated
 *                                     before anything is written (CSIC_EFORMAT); sizes[k] > stride_bytes or map_stride < map_bytes:
 *                                     CSIC_EINVAL_SIZE.
 *   csic_container_rows             : *flag = 1 for a version-8 file, 0 for every other version.
 *   csic_container_read resolves the layer on the host and returns the frames themselves; _info_of reports version 8; _coded_sizes
 *   gives the table (maps included); _gop gives 1 and _motion -1; csic_container_inter_groups counts the groups predicted from the row
 *   above, the popcount of each section of each frame's map.
 * CSIC_EFORMAT for a version-8 file, beyond the cases of versions 3 / 4 / 7 without a gop (with the sizes of the file's coding plus
 * map_bytes): a coding id other than 1, 3 or 5; any bit of the word at 80 other than the id and bit 16 -- a version-7 body behind a
 * version-8 header is refused at the header --; a word at 84 that is not 0; a padding bit that is set in a map, or a set bit in the
 * section of a plane with K = 0; any coded frame the coding's host decoder refuses.  Versions 1 to 7 keep their bytes and refusals. */
typedef struct csic_container_info {
    csic_params params;            /* out_format = CSIC_FMT_PLANAR_BITS, in_format = CSIC_FMT_ARGB8888 */
    int32_t version, nframes;
    int64_t payload_bytes;         /* per frame = csic_planar_bits_layout_of(params).payload_bytes */
    int64_t file_bytes;
} csic_container_info;
int  csic_container_info_of(const char *path, csic_container_info *info);
int  csic_container_write(const char *path, const csic_params *p, const void *frames, int32_t nframes);
int  csic_container_read(const char *path, void *frames, size_t frames_bytes);
int  csic_container_write_ex(const char *path, const csic_params *p, const void *frames, int32_t nframes, int32_t coding);
int  csic_container_write_coded(const char *path, const csic_params *p, const void *coded, size_t stride_bytes, const uint64_t *sizes,
                                int32_t nframes);
int  csic_container_write_coded_ex(const char *path, const csic_params *p, const void *coded, size_t stride_bytes, const uint64_t *sizes,
                                   int32_t nframes, int32_t coding);
int  csic_container_coded_sizes(const char *path, uint64_t *sizes, int32_t n);
int  csic_container_write_seq(const char *path, const csic_params *p, const void *frames, int32_t nframes, int32_t coding, int32_t gop);
int  csic_container_write_coded_seq(const char *path, const csic_params *p, const void *coded, size_t stride_bytes, const uint64_t *sizes,
                                    const void *maps, size_t map_stride, int32_t nframes, int32_t coding, int32_t gop);
int  csic_container_gop(const char *path, int32_t *gop);
int  csic_container_inter_groups(const char *path, uint64_t *counts, int32_t n);
int  csic_container_write_seq_ex(const char *path, const csic_params *p, const void *frames, int32_t nframes, int32_t coding, int32_t gop,
                                 int32_t range);
int  csic_container_write_coded_seq_ex(const char *path, const csic_params *p, const void *coded, size_t stride_bytes, const uint64_t *sizes,
                                       const void *maps, size_t map_stride, int32_t nframes, int32_t coding, int32_t gop, int32_t range);
int  csic_container_motion(const char *path, int32_t *range);
int  csic_container_write_rows(const char *path, const csic_params *p, const void *frames, int32_t nframes, int32_t coding);
int  csic_container_write_coded_rows(const char *path, const csic_params *p, const void *coded, size_t stride_bytes, const uint64_t *sizes,
                                     const void *maps, size_t map_stride, int32_t nframes, int32_t coding);
int  csic_container_rows(const char *path, int32_t *flag);

/* ---- host-frame pipeline (the step either side of the hot path) -----------------------------------
 * Replaces the reference's per-image  readImage -> per-pixel poke ... peek -> writeImage  flow
 * (ImageProcessorModel.scala:14-52, ImageCompressorTopApp.scala:39-41,76-144) for streams of frames that
 * live in host memory: `depth` slots, each with pinned host input/output staging, device buffers and its
 * own HIP stream, so that frame k+1's H2D copy, frame k's kernel and frame k-1's D2H copy overlap.
 *
 *   csic_pipeline_acquire_input : pointer to the next slot's pinned input buffer (width*height pixels);
 *                                 decode/write the frame straight into it.  Fails with CSIC_EINVAL_SIZE
 *                                 when every slot still holds an uncollected frame.
 *   csic_pipeline_submit        : enqueue H2D + kernel + D2H for the acquired buffer (asynchronous).
 *   csic_pipeline_collect       : wait for the OLDEST submitted frame; *host_out points at its pinned
 *                                 output (out_width*out_height pixels; for a CSIC_FMT_PLANAR plan the planar
 *                                 frame buffer of csic_planar_layout_of, frame_bytes long -- 1.5 bytes per
 *                                 pixel instead of 4 on the way back for 4:2:0), valid until that slot is
 *                                 submitted again.  Frames complete in submission order; *ticket counts from 0.
 * The plan must outlive the pipeline.  Not thread-safe (one producer/consumer thread). */
typedef struct csic_pipeline csic_pipeline;
int  csic_pipeline_create(csic_plan *plan, int32_t depth, csic_pipeline **out);
int  csic_pipeline_destroy(csic_pipeline *pipeline);
int  csic_pipeline_acquire_input(csic_pipeline *pipeline, uint32_t **host_in);
int  csic_pipeline_submit(csic_pipeline *pipeline, int64_t *ticket);
int  csic_pipeline_collect(csic_pipeline *pipeline, const uint32_t **host_out, int64_t *ticket);
int  csic_pipeline_pending(const csic_pipeline *pipeline);
/* CSIC_PIPELINE_ZERO_COPY (default): the kernel reads the pinned host input and writes the pinned host
 *     output directly over PCIe: dead input rows (r % factor != 0) never cross the bus and both PCIe
 *     directions are busy inside one launch (8192x8192 sf=2: 2.4 ms/frame vs 5.9 ms staged).
 * CSIC_PIPELINE_STAGED: hipMemcpyAsync H2D -> kernel -> hipMemcpyAsync D2H through device buffers; keeps
 *     the CUs free while the copy engines move the frame. */
#define CSIC_PIPELINE_STAGED    0
#define CSIC_PIPELINE_ZERO_COPY 1
int  csic_pipeline_set_mode(csic_pipeline *pipeline, int32_t mode);

/* ---- PNG files in, PNG files out: the pipeline with the codec on worker threads ---------------------------------
 * The batch counterpart of the reference's per-image  readImage -> DUT -> writeImage  flow (ImageProcessorModel.scala:14-52,
 * ImageCompressorTopApp.scala:39-41,133-144) for `nfiles` PNGs that are all frames of `plan`: `decode_threads` workers
 * decode straight into pinned frame slots and launch the fused kernel on the slot's stream (zero-copy over PCIe, as
 * CSIC_PIPELINE_ZERO_COPY), `encode_threads` workers wait for a slot and write out_paths[i] (8-bit RGB, zlib `png_level`).
 * <= 0 threads = the library's choice (up to 32 decoders / 16 encoders, never more than files or host cores); the slots
 * between the two pools are bounded (workers + 2, at most 8 GiB of pinned memory).  final_width / final_height > 0 select
 * what the reference's collector keeps when the dimensions do not divide by the factor -- the first final_width *
 * final_height pixels of the output stream, final_width per row, missing pixels magenta (ImageCompressorTopApp.scala:44-45,
 * 133-142); 0 = the plan's output size.  Every output file is byte for byte what csic_png_read_argb -> csic_pipeline_* ->
 * csic_png_write_argb on one thread writes for the same input.  The parent directories of out_paths must exist.
 * Synchronous; the first failure stops the batch and is returned (message: "file <i>: ...").  *stats may be NULL. */
typedef struct csic_files_stats {
    int64_t frames;                   /* files written                                                                   */
    double  wall_s;                   /* first worker started -> last worker finished                                     */
    double  decode_s, encode_s;       /* summed over the workers of each pool: seconds inside the PNG decoder / encoder   */
    double  gpu_wait_s, slot_wait_s;  /* encoders waiting for the GPU; decoders waiting for a free slot                    */
    int32_t decode_threads, encode_threads, slots, max_in_flight;   /* slots = pinned frame slots actually allocated */
    int64_t in_pixels, out_pixels;
} csic_files_stats;
int  csic_process_png_files(csic_plan *plan, const char *const *in_paths, const char *const *out_paths, int32_t nfiles,
                            int32_t decode_threads, int32_t encode_threads, int32_t png_level,
                            int32_t final_width, int32_t final_height, csic_files_stats *stats);

/* ---- cycle-level model of the Decoupled pixel stream (host only) ---------------------------
 * What the reference's users simulate is not a function from frames to frames but hardware: modules that exchange one
 * pixel per ready/valid handshake (ImageCompressorTop.scala:33-38), and its tests check the handshake as well as the
 * pixels (back-pressure: SpatialDownsamplerSpec.scala:48-58; the cycle budget of the app's collector:
 * ImageCompressorTopApp.scala:110).  A csic_stream is that interface, clock edge by clock edge, for
 *   CSIC_STREAM_TOP        class ImageCompressorTop: RGB2YCbCr -> Queue(1) -> op1 -> Queue(1) -> op2 -> Queue(1) -> op3
 *                          (ImageCompressorTop.scala:63-65,80-114; the queues are chisel3.util.Queue, pipe = flow = false)
 *   CSIC_STREAM_PROCESSOR  class ImageProcessor: RGB2YCbCr -> ChromaSubsampler -> SpatialDownsampler, no queues
 *                          (ImageProcessor.scala:42-62)
 *   CSIC_STREAM_RGB2YCBCR / _CHROMA / _SPATIAL / _QUANT   one module alone, as the reference's specs drive it
 * built from the same csic_params (and rejected by the same require()s; FLOOR_HW and HOLD_DECIMATE only: the RTL has no
 * other rounding or sampling).  in_bits is a PixelBundle (CSIC_FMT_ARGB8888) where the chain starts with RGB2YCbCr, else
 * a PixelYCbCrBundle (CSIC_FMT_YCBCR888X); out_bits is the PixelYCbCrBundle on io.out, or -- params.out_format ==
 * CSIC_FMT_ARGB8888 -- that pixel put through YCbCrUtils.ycbcr2rgb as the harness does (ImageCompressorTopApp.scala:118).
 * sof / eol are accepted and, as in the RTL (SpatialDownsampler.scala:11-12), read by no logic.
 *
 * This is a simulator of interface timing (a few Mpixel/s on one host core), NOT a compute path: no csic_process_* /
 * csic_plan_* / csic_frame_graph_* call ever reaches it, and they still fail with CSIC_ENODEVICE without a GPU.  RTL /
 * FIRRTL emission would need Chisel and is out of scope.
 *
 *   csic_stream_eval : the combinational outputs (in_ready, out_valid, out_bits) for the present state and inputs -- a
 *                      chiseltest peek(); the state does not change.
 *   csic_stream_step : the same outputs (may be NULL), then one rising clock edge -- poke(...); clock.step().
 *   csic_stream_run  : the reference harness's two loops in one call (ImageCompressorTopApp.scala:76-124): the driver keeps
 *                      a pixel on the wires until the edge at which in_ready is high, the collector takes a pixel at every
 *                      edge where out_valid && out_ready and stops after max_out pixels or max_cycles cycles (< 0: until the
 *                      input is used up and the pipeline has drained).  in_valid_pattern / out_ready_pattern (cyclic over
 *                      the cycle number, NULL = always 1) add producer gaps and back-pressure.  *n_out pixels were
 *                      collected in *cycles cycles; the stream's state carries over to the next call. */
#define CSIC_STREAM_TOP        0
#define CSIC_STREAM_PROCESSOR  1
#define CSIC_STREAM_RGB2YCBCR  2
#define CSIC_STREAM_CHROMA     3
#define CSIC_STREAM_SPATIAL    4
#define CSIC_STREAM_QUANT      5
typedef struct csic_stream csic_stream;
typedef struct csic_stream_in  { int32_t in_valid; uint32_t in_bits; int32_t out_ready; int32_t sof, eol; } csic_stream_in;
typedef struct csic_stream_out { int32_t in_ready; int32_t out_valid; uint32_t out_bits; } csic_stream_out;
int     csic_stream_create(const csic_params *p, int32_t kind, csic_stream **out);
int     csic_stream_destroy(csic_stream *stream);
int     csic_stream_reset(csic_stream *stream);                       /* every register back to its RegInit value, cycle count 0 */
int     csic_stream_eval(const csic_stream *stream, const csic_stream_in *in, csic_stream_out *out);
int     csic_stream_step(csic_stream *stream, const csic_stream_in *in, csic_stream_out *out);
int64_t csic_stream_cycles(const csic_stream *stream);                /* clock edges since creation / reset */
int     csic_stream_depth(const csic_stream *stream);                 /* modules in the chain (queues included): 7 for TOP */
int     csic_stream_run(csic_stream *stream, const uint32_t *in, size_t n_in, uint32_t *out, size_t max_out, int64_t max_cycles,
                        const uint8_t *in_valid_pattern, size_t in_pattern_len,
                        const uint8_t *out_ready_pattern, size_t out_pattern_len, size_t *n_out, int64_t *cycles);

/* ---- several devices from one process --------------------------------------------------------------
 * The same aligned row-stripe partition as csic_stripe_rows, for hosts that own all GPUs in ONE process
 * (a JVM, a C++ service); bench.py and the Python driver use one process per GPU instead.  Stripe i runs on
 * devices[i] (a device may be listed more than once) on a stream of its own; stripes are independent images,
 * so there is no halo and no peer traffic.
 *   csic_multi_process_device : d_in[i] / d_out[i] are device pointers ON devices[i] holding stripe i's input
 *                               rows / receiving its output rows (see csic_multi_stripe); asynchronous --
 *                               finish with csic_multi_synchronize.
 *   csic_multi_process_host   : whole frame in host memory: scatter, process, gather; synchronous. */
typedef struct csic_multi csic_multi;
int  csic_multi_create(const csic_params *p, const int32_t *devices, int32_t ndev, csic_multi **out);
int  csic_multi_destroy(csic_multi *multi);
int  csic_multi_count(const csic_multi *multi);
int  csic_multi_stripe(const csic_multi *multi, int32_t idx, int32_t *device, int32_t *row0, int32_t *nrows,
                       int32_t *out_row0, int32_t *out_nrows);
int  csic_multi_process_device(csic_multi *multi, const void *const *d_in, void *const *d_out);
int  csic_multi_synchronize(csic_multi *multi);
int  csic_multi_process_host(csic_multi *multi, const uint32_t *in, size_t in_px, uint32_t *out, size_t out_px);

#ifdef __cplusplus
}
#endif
#endif /* CSIC_H */
