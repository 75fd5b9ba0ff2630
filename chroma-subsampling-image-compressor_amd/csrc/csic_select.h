// csic_select.h -- the host-only planner: which packed kernel a parameter set takes (select_kernel), what it is called
// (kernel_name) and with what grid, block and kernel arguments it is launched (plan_launch); which kernel the measurement units
// take (measure_kind, measure_kernel_name); and the same three decisions for the plane units (plan_planar, plan_planar_bits,
// plan_reconstruct, plan_decode, plan_view and their name functions).  Pure integer arithmetic on csic_params, Geometry, the layouts of
// csic_internal.h and the tuning knobs: no HIP header, no device; csic_kernels.hip turns a KernelId into a function pointer
// (resolve), csic_measure.h and the plane units a kind into one, and tests/cpp/launch_table.cpp prints the whole table on a
// machine without a GPU.
#pragma once
#include "csic_internal.h"

namespace csic {

// ---- kernel arguments (kernarg segment -> SGPRs) ----------------------------------------------------
struct KArgs {
    const uint32_t *in;
    uint32_t *out;
    int32_t W, H, Wo, Ho;
    int32_t last_sample_col;
    uint32_t my, mcb, mcr;
    int32_t f, hmask, vmask, s_first;   // hmask = h-1, vmask = v-1 (generic kernel; vmask also k_dec SROWS)
    int32_t sc_shift, bc_row_off, bc_col_in;   // k_dec SROWS: log2 f; held-sample decimated row offset / input column
    int32_t edge_y0;                    // k_avg: first row of edge blocks along grid y (in what used to be padding: the size stays 152)
    int64_t in_frame_px, out_frame_px;  // batch strides (grid z = frame)
    int32_t bdx, bdy, row_step;         // block width/height and gridDim.y * bdy, passed explicitly (see pin_args)
    int32_t ip, op;                     // row pitch of the input / output frame in pixels (>= W / Wo; == when packed)
    uint32_t mW, mWo, kW, kWo;          // k_generic: exact n / W and n / Wo for n < 2^31 as (n * m) >> k (see magic_div)
    const uint32_t *const *in_tab;      // frame-table mode (CSIC_FRAME_GRAPH_FUSED): frame z reads in_tab[z] and writes out_tab[z];
    uint32_t *const *out_tab;           //   null = frames lie back to back behind `in` / `out`
};

// The direct-dispatch engine copies sizeof(KArgs) bytes into raw kernarg memory (csic_graph.hip): every translation unit must
// see this one layout -- there is exactly one copy of this header (tests/test_bench_contract.py checks that, too).
static_assert(sizeof(KArgs) == 152 && alignof(KArgs) == 8, "KArgs layout changed: check the kernarg blocks built in csic_graph.hip");

// The tuning knobs of csic_plan_tune.
struct Tune {
    int variant;         // CSIC_TUNE_VARIANT
    int force_generic;   // CSIC_TUNE_FORCE_GENERIC
    int no_vec;          // CSIC_TUNE_NO_VECTOR: 1 = no 16-byte vector kernels
    int no_nt;           // 1 = plain (cached) loads/stores instead of non-temporal ones
    int block_threads;   // 0 = default (256); 64 / 128 / 256 = that many (CSIC_TUNE_BLOCK_THREADS)
};

// What only a launch knows (its pointers, pitches and extents) and selection has to respect.
struct Constraints {
    bool no_flat;        // the frame's extents pass the 32-bit byte offsets / 24-bit row multiplies of the flat kernels
    bool no_vec;         // pointers or pitches that are only 4-byte aligned: no 16-byte vector kernels
};

// FAM_PLANAR: out_format CSIC_FMT_PLANAR / CSIC_FMT_PLANAR_BITS -- no packed kernel; plan_planar / plan_planar_bits below pick theirs.
enum Family { FAM_F1X4, FAM_DEC, FAM_DEC2V1, FAM_DEC2V2, FAM_GENERIC, FAM_AVG, FAM_AVG_GENERIC, FAM_DECFLAT, FAM_FLATGEN, FAM_F1FLAT, FAM_PLANAR };

constexpr int DEC_K = 4;     // output pixels per lane of k_dec / k_decflat / k_flatgen

// One instantiation of a packed kernel: the family and exactly the values that become its template arguments (the others are 0).
struct KernelId {
    Family fam;
    int round, fmt;      // csic_params.rounding / out_format: every family
    int infmt;           // csic_params.in_format: k_generic, k_avg_generic
    int f;               // k_dec, k_decflat, k_avg
    int h;               // k_f1x4, k_f1flat, k_avg: chroma hold h; k_dec, k_decflat: lane-hold distance (1, 2 or 4)
    int v;               // k_f1x4, k_f1flat, k_avg
    bool srows;          // k_dec, k_decflat: chroma rows follow the decimated stream and v = 2
    bool nt;             // non-temporal accesses (every family but the two generic ones)
    int tiles;           // k_avg: tiles per lane
};

struct Selection {
    KernelId id;
    int units_per_row;   // units along x
    int k_per_lane;      // x units consumed per lane
};

struct Dim3 { uint32_t x, y, z; };

// One fully planned launch: csic_kernels.hip adds the function pointer and where the frames are.
struct LaunchPlan {
    KernelId id;
    Dim3 grid, block;
    KArgs args;
};

Selection select_kernel(const csic_params &p, const Geometry &g, const Tune &t, const Constraints &c);
void kernel_name(const KernelId &id, const Geometry &g, char *buf, size_t len);
// The geometry half of the kernel arguments (what does not depend on the kernel family or the launch shape).
void fill_base_args(const Geometry &g, int32_t ip, int32_t op, KArgs *a);
// Threads per block of the kernels that take CSIC_TUNE_BLOCK_THREADS: 64 / 128 / 256 as tuned, `dflt` (the kernel's own; 0 = "not
// tuned") otherwise.  The one statement of that rule.
int tune_block_threads(const Tune &t, int dflt);
// Kernel, grid, block and arguments for `nframes` frames (<= 65535, the grid z limit) whose base pointers OR to `align_bits`,
// rows `in_pitch` / `out_pitch` pixels apart (0 = packed); the pointers in lp->args stay null.  Returns a csic status.
int plan_launch(const csic_params &p, const Geometry &g, const Tune &t, uintptr_t align_bits, int nframes, int32_t in_pitch,
                int32_t out_pitch, LaunchPlan *lp);

// ---- the measurement units (csic_distortion.hip, csic_ssim.hip) -----------------------------------------
enum MeasureFamily { MEASURE_DIST, MEASURE_SSIM };
// 0 = the unit's general kernel (k_dist_gen / k_ssim_gen), 1 / 2 = its fast kernel (k_dist_fast / k_ssim_fast) at factor 1 / 2
int measure_kind(const csic_params &p, const Geometry &g, const Tune &t, MeasureFamily fam);
// "k_dist_fast<f1>", "k_ssim_gen<avg,ycc-in>", ...: a static string
const char *measure_kernel_name(MeasureFamily fam, int kind, const csic_params &p);

// ---- code statistics (csic_code_stats.hip) ----------------------------------------------------------------
// CSTAT_GEN = k_cstat_gen (either source format), CSTAT_BYTES = k_cstat_bytes (CSIC_FMT_PLANAR), CSTAT_BITS = k_cstat_bits (CSIC_FMT_PLANAR_BITS)
enum CodeStatsKind { CSTAT_GEN, CSTAT_BYTES, CSTAT_BITS };
constexpr int CSTAT_T = 256;                    // threads per block
constexpr int64_t CSTAT_BLOCK_SAMPLES = 65536;  // consecutive samples of one plane that one block counts, whichever kernel
// src_format: CSIC_FMT_PLANAR or CSIC_FMT_PLANAR_BITS (validated by the caller)
CodeStatsKind code_stats_kind(int src_format, const Tune &t);
// "k_cstat_bytes<nt>", "k_cstat_bits<q6,5,5,nt>" (the Q of the Y, Cb and Cr launches), "k_cstat_gen<planar>" / "<bits>"
void code_stats_kernel_name(CodeStatsKind kind, int src_format, const csic_params &p, const Tune &t, char *buf, size_t len);

// ---- the plane units (csic_planar.hip, csic_planar_bits.hip, csic_decode.hip; reconstruct_device of csic_hip_common.h) ------
// Per-lane constants that planner and kernels share: groups of 4 positions per lane of k_planar_flat, k_pbits_f1, k_recon and
// k_rbits, and the 16-byte pieces per lane of k_decode at a factor.
constexpr int PLANAR_K = 4, PBITS_K = 4, RBITS_K = 4;
#ifndef CSIC_RECON_K
#define CSIC_RECON_K 4
#endif
constexpr int RECON_K = CSIC_RECON_K;
constexpr int dec_pieces_per_lane(int f) { return f == 1 ? 4 : f == 2 ? 2 : 1; }

// One kernel each.  PLANAR_FLAT_* are k_planar_flat's MODE 0 / 2 / 1 (PLANAR_FLAT_4PL, 4 consecutive positions per lane, is the first
// form of PLANAR_STRIDED: CSIC_TUNE_VARIANT 10, A/B); DEC_RECON is csic_reconstruct_device / csic_reconstruct_bits_device.
enum PlanarKind { PLANAR_FLAT_GEN, PLANAR_STRIDED, PLANAR_FLAT_F1X4, PLANAR_AVG_F1, PLANAR_AVG_GEN, PLANAR_FLAT_4PL, PLANAR_AVG_TILE };
enum BitsKind { PBITS_GEN, PBITS_F1, PBITS_STRIDED };
enum DecodeKind { DEC_GEN, DEC_FAST, DEC_RECON };

// The launch half of a plane unit's plan.  grid.z is nframes (at most 65535: the units cut longer calls into batches, which differ
// in z only).  T is the threads per block that PExtra / BExtra / DecArgs carry; bdx, bdy and row_step are what the unit sets in
// KArgs (0 where it sets none: reconstruct and decode).
struct PlaneLaunch {
    Dim3 grid, block;
    int32_t T, bdx, bdy, row_step;
};
struct PlanarPlan : PlaneLaunch { PlanarKind kind; KArgs args; };   // args: complete but for the pointers (PLANAR_AVG_TILE: the packed twin's)
struct BitsPlan : PlaneLaunch { BitsKind kind; };
struct ReconPlan : PlaneLaunch { bool fast; };
struct DecodePlan : PlaneLaunch { DecodeKind kind; bool recon_fast; };   // DEC_RECON: the reconstruct launch, and its kernel's FAST

// Forward to CSIC_FMT_PLANAR over `nframes` <= 65535 frames.  `align_bits` (the OR of the frame pointers, as plan_launch takes it)
// is NOT consulted: the 16-byte-load kernels are taken at any 4-byte alignment.  PLANAR_AVG_TILE launches as the k_avg
// of the plan's packed twin does (plan_launch); CSIC_EHIP if that twin turns out not to be FAM_AVG.
int plan_planar(const csic_params &p, const Geometry &g, const Tune &t, uintptr_t align_bits, int nframes, PlanarPlan *pp);
// Forward to CSIC_FMT_PLANAR_BITS; `in_align_bits`: the input pointer (k_pbits_f1's 16-byte loads need it 16-byte aligned).
// CSIC_EINVAL_SIZE for a frame of more than 2^31 - 1 blocks.
int plan_planar_bits(const csic_params &p, const Geometry &g, const Tune &t, uintptr_t in_align_bits, int nframes, BitsPlan *pp);
// Either reconstruct: `module_width` of the source's layout, K = RECON_K / RBITS_K groups per lane.
int plan_reconstruct(const Geometry &g, const Tune &t, int32_t module_width, int K, int nframes, ReconPlan *pp);
// csic_decode_device from `src_format` (any CSIC_FMT_*); align_bits: the output pointer, OR-ed with the source pointer for a packed source.
int plan_decode(const csic_params &p, const Geometry &g, const Tune &t, int src_format, uintptr_t align_bits, int nframes, DecodePlan *pp);
// "k_planar_flat<floor,f1x4,h2,v2,nt>", "k_pbits_gen<trunc,avg,h1,v1>", "k_recon<argb,fast,nt>", "k_decode<bits,ycc,f2,cached>", ...
void planar_kernel_name(PlanarKind kind, const csic_params &p, const Geometry &g, const Tune &t, char *buf, size_t len);
void planar_bits_kernel_name(BitsKind kind, const csic_params &p, const Geometry &g, const Tune &t, char *buf, size_t len);
void reconstruct_kernel_name(int src_format, int out_format, bool fast, const Tune &t, char *buf, size_t len);
void decode_kernel_name(const DecodePlan &pp, const Geometry &g, const Tune &t, int src_format, int out_format, char *buf, size_t len);

// ---- view decode (csic_decode_view_*, csic_decode.hip) ----------------------------------------------------------------------
constexpr int VIEW_PX = 4;                      // output pixels per lane of k_view (one 16-byte store)
enum ViewKind { VIEW_GEN, VIEW_FAST };
// T lanes per block along x, one UNIT per lane: VIEW_PX consecutive output pixels of a row (k_view; units_per_row = width / 4) or
// one output pixel (k_view_gen; units_per_row = width); grid.x * T >= units = units_per_row * view.height.  ncx / ncy: the most
// decimated columns / rows one s x s box can touch -- s / f, one more where the view's origin is no multiple of f; 1 or 2 at s < f.
struct ViewPlan : PlaneLaunch {
    ViewKind kind;
    int32_t ls;                                 // log2 scale
    int32_t units_per_row, ncx, ncy;
    int64_t units;
};
// CSIC_OK, or CSIC_EINVAL_SIZE for a scale outside {1, 2, 4, 8, 16} or a source rectangle that leaves the frame (64-bit arithmetic)
int check_view(const Geometry &g, const csic_view &v);
// csic_decode_view_device for a checked view; align_bits: the output pointer.  The fast kernel is taken when view.width % 4 == 0, the
// output is 16-byte aligned, the view has at most 2^30 pixels and no knob (variant 9, NO_VECTOR, FORCE_GENERIC) asks for the general one.
int plan_view(const Geometry &g, const Tune &t, const csic_view &v, uintptr_t align_bits, int nframes, ViewPlan *pp);
// "k_view<s8,bits,argb,nt>", "k_view_gen<planar,ycc>"
void view_kernel_name(const ViewPlan &pp, const Tune &t, int src_format, int out_format, char *buf, size_t len);

} // namespace csic
