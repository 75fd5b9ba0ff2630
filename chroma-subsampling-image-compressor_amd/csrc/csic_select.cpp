// csic_select.cpp -- kernel selection, kernel names and launch geometry of the packed kernels and of the plane units (planar and
// bit-plane forward, reconstruct, decode), kernel selection and names of the measurement units (see csic_select.h).  Host only.
// Every rule here is backed by a measurement under profiles/; tests/data/launch_table.txt records what the rules give.
#include "csic_select.h"

#include <cstdio>
#include <cstring>
#include <initializer_list>

namespace csic {

// Block width k_dec would take for `lanes_x` lanes per row in blocks of `tpb` threads (launch_dec): a width that divides
// the row exactly when there is one between tpb / 2 and tpb lanes, else the power of two that leaves a partial chunk.
static int dec_block_x(int lanes_x, int tpb, int hold)
{
    int bx = 1;
    while (bx < lanes_x) bx <<= 1;
    if (bx > tpb) bx = tpb;
    if (lanes_x <= tpb) {
        if (lanes_x % hold == 0) bx = lanes_x;
    } else {
        for (int m = (lanes_x + tpb - 1) / tpb; m <= lanes_x / (tpb / 2); ++m)
            if (lanes_x % m == 0 && (lanes_x / m) % hold == 0) { bx = lanes_x / m; break; }
    }
    return bx;
}

// One-wave blocks for narrow rows (a row needs at most two waves and tiles into them): see launch_dec.
static bool dec_one_wave_blocks(int lanes_x, int f, int hold)
{
    if (lanes_x < 16 || lanes_x > 128) return false;
    bool tiles = (f >= 4 && lanes_x < 64) || (lanes_x & (lanes_x - 1)) == 0;       // 16, 32, 64, 128; any < 64 for f >= 4
    for (int w = 64; !tiles && w >= 48; --w) tiles = lanes_x % w == 0 && w % hold == 0;
    return tiles && (lanes_x >= 64 || lanes_x % hold == 0);
}

// Should a chroma-before-spatial, hold-free plan cover the flat decimated stream (k_decflat) instead of rows (k_dec)?
// Measured over 22 shapes (tools/probe_flat.py, profiles/r03_probe_flat.log; batched launches, k_dec | flat):
//  * rows k_dec cannot cut into whole blocks -- not a whole number of K-pixel lanes, or lanes without a usable divisor: every
//    block of k_dec runs its bounds-checked path (1000x1000 f = 4 / 8: 66 / 63 | 73 / 71 %; 1366x768 f = 2: 68 | 79 %);
//  * rows of a few partly filled waves that straddle two rows at odd offsets (1000x1000 f = 2: 70 | 78 %, 720x480 f = 2:
//    70 | 78 %, 352x288 f = 2: 70 | 81 %, 1280x720 f = 2: 78.5 | 81.5 %);
//  * rows of whole waves: level or slightly ahead (8192x8192 f = 2 / 4 / 8: 79.8 | 82.6, 76.3 | 76.9, 74.3 | 77.0 %; 3840x2160
//    f = 4: 75.3 | 76.7 %; 1080p / 4K f = 2: 79.6 | 80.4 %), and on the headline -- ONE 8192x8192 frame per launch -- four
//    interleaved repeats give 32.09 | 31.85 us = 78.4 | 79.0 % (profiles/r03_headline_flat_ab.jsonl);
//  * the one exception: shapes that take k_dec's one-wave blocks (512x512 f = 2: 77 | 65-73 %; 1024x1024 f = 8: 79 | 70-78 %;
//    640x480 f = 4 and 1920x1080 f = 4 level) stay with k_dec;
//  * the same picture with a lane hold and with spatial before chroma (profiles/r03_probe_flat_{csq411,scq444,scq422,scq420}.log;
//    4:2:0 spatial before chroma: 1000x1000 f = 2: 60 | 78 %, 352x288 f = 2: 61 | 80 %, 8192x8192 f = 2 / 4 / 8: 79.4 | 82.6,
//    77.0 | 77.8, 75.2 | 77.5 % -- once the held-pixel load of the odd chroma rows is skipped wave-uniformly; loaded
//    unconditionally it cost 8192x8192 f = 8 twenty points).
static bool dec_prefers_flat(const Geometry &g, int hold)
{
    if (g.Wo % DEC_K != 0) return true;
    return !dec_one_wave_blocks(g.Wo / DEC_K, g.f, hold);
}

// Can the k_dec family handle this geometry?  Chroma before spatial: always, except that a hold across
// lanes (4:1:1 with f = 2) needs whole quads in a row.  Spatial before chroma: only when chroma rows
// coincide with groups of decimated rows (f | W) and the in-row hold is lane-aligned (h | Wo).
static bool dec_fast_ok(const Geometry &g)
{
    const int hold = (g.s_first || g.f == 1) ? g.h : (g.h > g.f ? g.h / g.f : 1);
    const int lanes_x = (g.Wo + DEC_K - 1) / DEC_K;
    if (hold > 1 && lanes_x < 3) return false;            // block width < 4 lanes: quads would span rows
    if (!g.s_first) return true;
    return (g.W % g.f == 0) && (g.Wo % g.h == 0);
}

Selection select_kernel(const csic_params &p, const Geometry &g, const Tune &t, const Constraints &c)
{
    Selection s{};
    KernelId &id = s.id;
    if (p.out_format == CSIC_FMT_PLANAR || p.out_format == CSIC_FMT_PLANAR_BITS) {
        id.fam = FAM_PLANAR;
        return s;
    }
    id.round = p.rounding; id.fmt = p.out_format;
    const bool nt = !t.no_nt, no_vec = t.no_vec || c.no_vec;
    // A YCbCr input stream (single-stage driving, the reference's spec style) is a test-oriented path:
    // it is served by the run-time-parameter kernels only.
    const bool ycc_in = p.in_format == CSIC_FMT_YCBCR888X;
    if (p.sampling == CSIC_SAMPLING_AVG) {
        const int th = g.f > g.v ? g.f : g.v;
        const int tw = g.f == 8 ? 8 : 4;
        // any shape with at least one whole tile (pair of tiles at f = 8) and tile row: the frame's cut tiles take the definition's
        // clamped form inside k_avg; variant 8 keeps the rule of rounds 1-3 (whole tiles only, everything else generic) for A/B
        const bool whole = g.W % tw == 0 && g.H % th == 0;
        if (!t.force_generic && !ycc_in && !no_vec && g.W >= tw && g.H >= th && (whole || t.variant != 8)) {
            id.fam = FAM_AVG; id.f = g.f; id.h = g.h; id.v = g.v; id.nt = nt;
            id.tiles = (g.f <= 2) ? 2 : 1;               // TILES of k_avg
            s.units_per_row = (g.W + 3) / 4;
            s.k_per_lane = id.tiles;
        } else {
            id.fam = FAM_AVG_GENERIC; id.infmt = p.in_format;
            s.units_per_row = g.Wo;
            s.k_per_lane = 1;
        }
        return s;
    }
    // f = 1: the 16-byte kernel wins whenever it applies (8192^2: 4:4:4 84.0 vs 88.0 us, 4:2:0 84.5 vs 85.9 us for
    // the 4-byte k_dec<f1>, which serves the other widths / alignments; variant 4 forces k_dec<f1> for A/B).
    const bool f1x4_ok = !t.force_generic && !ycc_in && !no_vec && g.f == 1 && g.W % 4 == 0;
    if (f1x4_ok && t.variant != 11 && t.variant != 4 && !c.no_flat) {
        // the flat mapping (round 4): ahead of k_f1x4 at every chroma mode and on 10 of 12 frame sizes -- 8192x8192 4:2:0 77.0 ->
        // 79.3 %, 4:2:2 77.5 -> 80.3 %, 4:4:4 78.8 -> 79.8 %, 4:1:0 76.5 -> 79.5 %, 4096x4096 76.5 -> 79.1 %, 1000x1000 76.6 -> 78.9 %;
        // level (-0.5) on 3840x2160 and 1920x1080 (profiles/r04_f1flat_ab.log).  CSIC_TUNE_VARIANT 11 keeps k_f1x4 for A/B.
        id.fam = FAM_F1FLAT; id.h = g.h; id.v = g.v; id.nt = nt;
        s.units_per_row = g.W / 4;
        s.k_per_lane = 1;
    } else if (f1x4_ok && (t.variant != 4 || !dec_fast_ok(g))) {
        id.fam = FAM_F1X4; id.h = g.h; id.v = g.v; id.nt = nt;
        s.units_per_row = g.W / 4;
        s.k_per_lane = 1;
    } else if (!t.force_generic && !ycc_in && dec_fast_ok(g)) {
        // in-row chroma hold distance in decimated lanes; srows = chroma rows follow the decimated stream
        // (with f = 1 the decimated stream IS the image and both order classes coincide: any width, any
        // 4-byte-aligned pointer, 4-byte accesses)
        const bool srows = g.s_first != 0 || g.f == 1;
        const int hold = srows ? g.h : (g.h > g.f ? g.h / g.f : 1);
        if (g.f == 2 && hold == 1 && !srows && !no_vec && g.W % 8 == 0 && (t.variant == 1 || t.variant == 2)) {
            id.fam = t.variant == 1 ? FAM_DEC2V1 : FAM_DEC2V2; id.nt = nt;
            s.units_per_row = g.Wo / (t.variant == 1 ? 2 : 4);
            s.k_per_lane = 1;
        } else {
            // lanes over the flat decimated stream (variant 5 keeps k_dec, variant 6 takes k_decflat wherever it applies: A/B);
            // a hold group must not straddle two rows: hold | Wo (spatial before chroma has that from dec_fast_ok)
            const bool flat = g.f >= 2 && g.Wo % hold == 0 && t.variant != 5 && !c.no_flat && (t.variant == 6 || dec_prefers_flat(g, hold));
            id.fam = flat ? FAM_DECFLAT : FAM_DEC;
            id.f = g.f; id.h = hold; id.srows = srows && g.v == 2; id.nt = nt;
            s.units_per_row = g.Wo;
            s.k_per_lane = DEC_K;
        }
    } else if (!t.force_generic && !ycc_in && g.f >= 2 && t.variant != 7 && !c.no_flat) {
        // what k_dec / k_decflat cannot take (spatial before chroma with f not dividing W or h not dividing Wo; tiny frames with a
        // hold): the general flat kernel; variant 7 keeps the one-pixel-per-lane k_generic for A/B
        id.fam = FAM_FLATGEN; id.nt = nt;
        s.units_per_row = g.Wo;
        s.k_per_lane = DEC_K;
    } else {
        id.fam = FAM_GENERIC; id.infmt = p.in_format;
        s.units_per_row = g.Wo;
        s.k_per_lane = 1;
    }
    return s;
}

void kernel_name(const KernelId &id, const Geometry &g, char *buf, size_t len)
{
    const char *rn = id.round == CSIC_ROUND_FLOOR_HW ? "floor" : "trunc";
    const char *fn = id.fmt == CSIC_FMT_ARGB8888 ? "argb" : "ycc";
    const char *ntn = id.nt ? "nt" : "cached";
    const char *ycc_in = id.infmt == CSIC_FMT_YCBCR888X ? ",ycc-in" : "";
    const bool srows = g.s_first != 0 || g.f == 1;       // the order class as select_kernel sees it
    const char *order = srows ? (g.v == 2 ? "s>c,v2" : "s>c") : "c>s";
    switch (id.fam) {
    case FAM_AVG: snprintf(buf, len, "k_avg<%s,%s,f%d,h%d,v%d,%s>", rn, fn, id.f, id.h, id.v, ntn); break;
    case FAM_AVG_GENERIC: snprintf(buf, len, "k_avg_generic<%s,%s%s>", rn, fn, ycc_in); break;
    case FAM_F1FLAT: snprintf(buf, len, "k_f1flat<%s,%s,h%d,v%d,%s>", rn, fn, id.h, id.v, ntn); break;
    case FAM_F1X4: snprintf(buf, len, "k_f1x4<%s,%s,h%d,v%d,%s>", rn, fn, id.h, id.v, ntn); break;
    case FAM_DEC2V1:
    case FAM_DEC2V2: snprintf(buf, len, "k_dec2v<%s,%s,var%d,%s>", rn, fn, id.fam == FAM_DEC2V1 ? 1 : 2, ntn); break;
    case FAM_DECFLAT:
        if (id.h == 1 && !srows) snprintf(buf, len, "k_decflat<%s,%s,f%d,K%d,%s>", rn, fn, id.f, DEC_K, ntn);
        else snprintf(buf, len, "k_decflat<%s,%s,f%d,hold%d,%s,K%d,%s>", rn, fn, id.f, id.h, order, DEC_K, ntn);
        break;
    case FAM_DEC:
        snprintf(buf, len, "k_dec<%s,%s,f%d,hold%d,%s,K%d,%s>", rn, fn, id.f, id.h, id.f == 1 ? (g.v == 2 ? "v2" : "v1") : order, DEC_K, ntn);
        break;
    case FAM_FLATGEN: snprintf(buf, len, "k_flatgen<%s,%s,K%d,%s>", rn, fn, DEC_K, ntn); break;
    case FAM_GENERIC: snprintf(buf, len, "k_generic<%s,%s%s>", rn, fn, ycc_in); break;
    case FAM_PLANAR: snprintf(buf, len, "%s", ""); break;   // planar_kernel_name / planar_bits_kernel_name below
    }
}

static int pow2_ceil(int x) { int p = 1; while (p < x) p <<= 1; return p; }

void fill_base_args(const Geometry &g, int32_t ip, int32_t op, KArgs *pa)
{
    KArgs &a = *pa;
    std::memset(&a, 0, sizeof a);
    a.W = g.W; a.H = g.H; a.Wo = g.Wo; a.Ho = g.Ho;
    a.last_sample_col = g.last_sample_col;
    a.my = g.mask_y; a.mcb = g.mask_cb; a.mcr = g.mask_cr;
    a.f = g.f; a.hmask = g.h - 1; a.vmask = g.v - 1; a.s_first = g.s_first;
    a.ip = ip; a.op = op;
    a.in_frame_px = (int64_t)ip * g.H;
    a.out_frame_px = (int64_t)op * g.Ho;
    a.sc_shift = (g.f == 8) ? 3 : (g.f == 4) ? 2 : (g.f == 2) ? 1 : 0;
    a.bc_row_off = g.last_sample_col / g.Wo;             // only meaningful (and only used) when f | W
    a.bc_col_in = (g.last_sample_col % g.Wo) * g.f;
    magic_div((uint32_t)g.W, &a.mW, &a.kW);
    magic_div((uint32_t)g.Wo, &a.mWo, &a.kWo);
}

// ---- launch geometry, one function per mapping -------------------------------------------------------------------------
int tune_block_threads(const Tune &t, int dflt)
{
    return (t.block_threads == 64 || t.block_threads == 128 || t.block_threads == 256) ? t.block_threads : dflt;
}

static int64_t flat_blocks(int64_t n, int K, int T)
{
    const int64_t per_block = (int64_t)T * K;
    return (n + per_block - 1) / per_block;
}

// Lanes over a flat stream of `n` units, K per lane spaced by the block: one-dimensional blocks of T threads.
static void launch_flat(int64_t n, int K, int T, int nframes, LaunchPlan *lp)
{
    lp->block = Dim3{(uint32_t)T, 1, 1};
    lp->args.bdx = T; lp->args.bdy = 1; lp->args.row_step = 1;
    lp->grid = Dim3{(uint32_t)flat_blocks(n, K, T), 1, (uint32_t)nframes};
}

// Blocks of bx lanes by tpb / bx rows over `lanes_x` lanes and `rows` rows; the kernels stride over rows past the grid y limit.
// nedge >= 0: k_avg, whose edge blocks -- one lane per output pixel that no whole tile produces (see k_avg) -- lie in rows of
// blocks below the grid.
static void launch_rows(int lanes_x, int rows, int bx, int tpb, int64_t nedge, int nframes, LaunchPlan *lp)
{
    const int by = tpb / bx > 0 ? tpb / bx : 1;
    const uint32_t gx = (uint32_t)((lanes_x + bx - 1) / bx);
    uint32_t gy_edge = 0;
    if (nedge >= 0) {
        const int64_t nblocks = (nedge + (int64_t)bx * by - 1) / ((int64_t)bx * by);
        gy_edge = (uint32_t)((nblocks + gx - 1) / gx);
    }
    uint32_t gy = (uint32_t)((rows + by - 1) / by);
    if (gy > 65535u - gy_edge - 1u) gy = 65535u - gy_edge - 1u;  // kernels stride over rows
    if (gy_edge > 0 && nframes > 1 && (gx * (gy + gy_edge)) % 8u == 0) {
        // XCD-aware: workgroups go to the 8 XCDs round-robin in dispatch order, so with a multiple of 8 blocks per frame the
        // few (slower, latency-bound) edge blocks of EVERY frame of a batch land on the same XCDs.  1922x1082 at f = 2 -- 541 + 3
        // block rows -- ran at 66 % where 1922x1080 and 1922x1084 ran at 74 % (profiles/r04_avg_1922_sweep.log).  One more
        // (empty) block row per frame rotates them.
        gy_edge += 1;
    }
    lp->block = Dim3{(uint32_t)bx, (uint32_t)by, 1};
    lp->args.bdx = bx; lp->args.bdy = by; lp->args.row_step = (int32_t)gy * by;
    lp->args.edge_y0 = nedge >= 0 ? (int32_t)gy : 0x7FFFFFFF;
    lp->grid = Dim3{gx, gy + gy_edge, (uint32_t)nframes};
}

static int pow2_block_x(int lanes_x, int tpb)
{
    int bx = pow2_ceil(lanes_x);
    if (bx > tpb) bx = tpb;
    return bx < 1 ? 1 : bx;
}

static void launch_f1flat(const Geometry &g, const Tune &t, int nframes, LaunchPlan *lp)
{
    launch_flat((int64_t)(g.W / 4) * g.H, 4, tune_block_threads(t, 64), nframes, lp);
}

static void launch_decflat(const Geometry &g, const Tune &t, int nframes, LaunchPlan *lp)
{
    // lanes over the flat decimated stream: blocks of whole waves, K indices per lane spaced by the block size
    // Two-wave blocks at f = 2 (1000x1000 77.8 -> 78.6 %, 1366x768 77.1 -> 79.0, 352x288 80.5 -> 81.8, 8192x8192 80.0 -> 82.6)
    // and for long rows at f = 4 / 8 (3840x2160 f = 4: 74.7 -> 76.7 %, 8192x8192 f = 8: 75.9 -> 77.0); four-wave blocks for
    // short rows at f = 4 / 8 (1000x1000 f = 4: 72.3 % against 69.4 / 68.4 % with 128 / 64 threads; 1920x1080 f = 8: 75.7
    // against 75.2 / 71.1).                                                      profiles/r03_probe_flat.log
    launch_flat((int64_t)g.Wo * g.Ho, DEC_K, tune_block_threads(t, (g.f == 2 || g.Wo >= 512) ? 128 : 256), nframes, lp);
}

static void launch_dec(const Geometry &g, const Tune &t, int hold, int nframes, LaunchPlan *lp)
{
    // Threads per block.  256 by default; k_dec takes two-wave blocks (128 threads) for a single frame of >= 64 MB whose rows
    // tile into full waves at that width: measured on one-frame-per-launch streams (profiles/r02_probe_block_shapes.log)
    // 8192x8192 f=2 32.48 -> 31.89 us, 16384x4096 32.56 -> 31.98, 8192x4096 17.44 -> 17.27, 6144x6144 19.38 -> 19.18,
    // 8192x8192 f=4 15.52 -> 15.37; no gain below ~64 MB (8192x2048: 9.88 / 9.88), none for batched launches, and a loss
    // where 128 lanes do not divide the row into full waves (7680x4320: 17.29 -> 17.93).  CSIC_TUNE_BLOCK_THREADS overrides.
    const int lanes_x = (g.Wo + DEC_K - 1) / DEC_K;
    const bool whole = g.Wo % DEC_K == 0;
    const int forced = tune_block_threads(t, 0);
    int tpb = 256;
    if (forced) tpb = forced;
    else if (nframes == 1 && whole && lanes_x % 128 == 0 && 4ll * ((int64_t)g.W * g.Ho + (int64_t)g.Wo * g.Ho) >= (64ll << 20))
        tpb = 128;
    else if (whole && lanes_x >= 16 && lanes_x <= 128) {
        // Narrow rows (a row needs at most two waves): one-wave blocks, when the row tiles into them, beat blocks that stack
        // several rows -- batched launches, profiles/r02_probe_block_batched.log: 512x512 f=2 69.1 -> 73.5 %, f=8 69.3 -> 73.2,
        // 1024x1024 f=8 66.8 -> 78.3, 1920x1080 f=4 74.1 -> 75.6, f=8 71.0 -> 73.5; rows that do not tile (1000x1000 f=2: 125
        // lanes) lose (70.8 -> 63.4) and keep the default, as do rows of fewer than 16 lanes (128x128 f=4/8: -1 %).
        // With f >= 4, rows of fewer than 64 lanes fit one wave whatever their width (640x480 f=4, 40 lanes: 74.1 -> 77.7 %;
        // 352x288 f=4 s>c: 62.0 -> 72.4 %); at f = 2 that loses (352x288, 44 lanes: 70.5 -> 59.3 %) and only powers of two qualify.
        if (dec_one_wave_blocks(lanes_x, g.f, hold)) tpb = 64;
    }
    // Rows that do not tile into power-of-two chunks (1920/3840-wide video: Wo = 960, 1920, ...) would put
    // their last chunk on the bounds-checked path.  A block width that divides the row exactly keeps
    // every block on the straight-line path (4K f=2: 70 % -> 80 % of HBM peak).  The width only has to
    // be a multiple of the lane-hold distance so that a DPP hold group never straddles two rows.
    const int bx = whole ? dec_block_x(lanes_x, tpb, hold) : pow2_block_x(lanes_x, tpb);
    launch_rows(lanes_x, g.Ho, bx, tpb, -1, nframes, lp);
}

static void launch_f1x4(const Geometry &g, const Tune &t, int nframes, LaunchPlan *lp)
{
    const int lanes_x = g.W / 4, forced = tune_block_threads(t, 0), tpb = tune_block_threads(t, 256);
    int bx = pow2_block_x(lanes_x, tpb);
    if (!forced) {
        // One 16-byte load and store per lane: this kernel lives on the wave launch rate, so waves that exit at once (the idle
        // part of a block's last chunk) or run partly filled cost in proportion.  1280-wide rows are 320 lanes: [256][64 + 192
        // idle] runs at 61 %, 5 x 64 lanes (four rows to a block) at 78 % (profiles/r02_probe_block_batched_video.log).
        if (lanes_x % 64 == 0) {
            for (int w : {256, 192, 128, 64}) if (lanes_x % w == 0) { bx = w; break; }
        } else if (lanes_x <= 256) {
            bx = lanes_x;                                      // one partly filled wave per row instead of idle ones
        }
    }
    launch_rows(lanes_x, g.H, bx, tpb, -1, nframes, lp);
}

static void launch_avg(const Geometry &g, const Tune &t, int tiles, int nframes, LaunchPlan *lp)
{
    const int units = (g.W + 3) / 4, lanes_x = (units + tiles - 1) / tiles, avg_th = g.f > g.v ? g.f : g.v;
    const int forced = tune_block_threads(t, 0), tpb = tune_block_threads(t, 256);
    int bx = pow2_block_x(lanes_x, tpb);
    if (!forced && lanes_x % 64 == 0 && lanes_x > 256 && lanes_x <= 512 && lanes_x % 256 != 0) {
        // the same as k_f1x4 on rows of at most two blocks: 1280-wide f = 4 / 8 (320 lanes) 64 / 61 % -> 80 % with blocks of whole
        // waves that tile the row (profiles/r02_probe_block_avg.log)
        for (int w : {192, 128, 64}) if (lanes_x % w == 0) { bx = w; break; }
    } else if (!forced && lanes_x > tpb && lanes_x % tpb != 0 && lanes_x <= 8 * tpb) {
        // rows of a few blocks that do not tile (1368-wide f = 4: 342 lanes = [256][86 + 170 idle]): equal blocks instead of a
        // nearly empty last one
        // (a multiple of 4 lanes: at f = 8 the two tiles of an output are neighbouring lanes of one quad -- the DPP swap -- so a
        // block must not start on an odd tile; tools/fuzz_gpu.py found 1032x8 with 129-lane blocks)
        const int m = (lanes_x + tpb - 1) / tpb;
        bx = ((lanes_x + m - 1) / m + 3) & ~3;
        if (bx > tpb) bx = tpb;
    }
    // the output pixels that no whole tile produces
    const int W4f = g.W / 4, ntrf = g.H / avg_th;
    const int Cw = g.f == 8 ? W4f / 2 : W4f * (4 / g.f), Rw = g.f == 8 ? ntrf : ntrf * (avg_th / g.f);
    const int64_t nedge = (int64_t)(g.Wo - Cw) * g.Ho + (int64_t)(g.Ho - Rw) * Cw;
    launch_rows(lanes_x, (g.H + avg_th - 1) / avg_th, bx, tpb, nedge, nframes, lp);
}

// k_dec2v, k_generic, k_avg_generic: one unit per lane along x, rows of the output along y
static void launch_per_lane(const Geometry &g, const Tune &t, int units, int nframes, LaunchPlan *lp)
{
    const int tpb = tune_block_threads(t, 256);
    launch_rows(units, g.Ho, pow2_block_x(units, tpb), tpb, -1, nframes, lp);
}

int plan_launch(const csic_params &p, const Geometry &g, const Tune &t, uintptr_t align_bits, int nframes, int32_t in_pitch,
                int32_t out_pitch, LaunchPlan *lp)
{
    if (nframes <= 0 || nframes > 65535)
        return set_error(CSIC_EINVAL_SIZE, "nframes per launch must be in 1..65535. Got %d", nframes);
    if (p.out_format == CSIC_FMT_PLANAR_BITS)
        return set_error(CSIC_EINVAL_FORMAT, "CSIC_FMT_PLANAR_BITS plans go through csic_process_device / csic_process_batch_device / "
                                              "csic_process_host and csic_pipeline_* only (no row pitches, frame graphs, file pools or csic_multi)");
    if (p.out_format == CSIC_FMT_PLANAR)
        return set_error(CSIC_EINVAL_FORMAT, "planar plans go through csic_process_device / csic_process_batch_device / csic_process_host, "
                                              "csic_pipeline_* and fused frame graphs only (no row pitches, per-frame-launch graphs, file pools or csic_multi)");
    const int32_t ip = in_pitch > 0 ? in_pitch : g.W, op = out_pitch > 0 ? out_pitch : g.Wo;
    if (ip < g.W || op < g.Wo)
        return set_error(CSIC_EINVAL_SIZE, "row pitch (%d, %d px) smaller than the frame width (%d, %d px)", ip, op, g.W, g.Wo);

    Selection s = select_kernel(p, g, t, Constraints{false, false});
    const Family fam = s.id.fam;
    // The vector kernels need 16-byte aligned frame bases; otherwise take the 4-byte-access kernels.
    // (k_avg takes any 4-byte alignment: gfx950 executes its 16-byte accesses at any dword address, tools/ubench_unaligned.hip;
    // the others keep the rule because their 4-byte fallbacks are as fast as a misaligned vector access would be)
    const bool vec = (fam == FAM_F1X4 || fam == FAM_DEC2V1 || fam == FAM_DEC2V2 || fam == FAM_F1FLAT);
    // The flat kernels address a pixel by a 32-bit BYTE offset from its frame's base (decflat_body): frames whose extents -- pitch
    // included -- pass 2^30 pixels (4 GiB) take the row kernels, which keep 64-bit offsets.
    // (and whose rows and pitch -- times the factor -- fit 24 bits, for the full-rate 24-bit multiplies of the row offsets)
    const int64_t flat_limit = 1ll << 30;
    const bool too_wide = (fam == FAM_DECFLAT || fam == FAM_FLATGEN || fam == FAM_F1FLAT) &&
                          ((int64_t)(g.H - 1) * ip + g.W > flat_limit || (int64_t)(g.Ho - 1) * op + g.Wo > flat_limit ||
                           g.H >= (1 << 24) || (int64_t)ip * g.f >= (1 << 24) || op >= (1 << 24));
    const bool misaligned = vec && ((align_bits & 15u) || ((ip | op) & 3));
    if (too_wide || misaligned) s = select_kernel(p, g, t, Constraints{too_wide, misaligned});

    lp->id = s.id;
    fill_base_args(g, ip, op, &lp->args);
    switch (s.id.fam) {
    case FAM_F1FLAT: launch_f1flat(g, t, nframes, lp); break;
    case FAM_DECFLAT:
    case FAM_FLATGEN: launch_decflat(g, t, nframes, lp); break;
    case FAM_DEC: launch_dec(g, t, s.id.h, nframes, lp); break;
    case FAM_F1X4: launch_f1x4(g, t, nframes, lp); break;
    case FAM_AVG: launch_avg(g, t, s.id.tiles, nframes, lp); break;
    default: launch_per_lane(g, t, s.units_per_row, nframes, lp); break;
    }
    return CSIC_OK;
}

// ---- the measurement units ----------------------------------------------------------------------------------------------
// The fast kernels serve the reference's sampling on ARGB input at factor 1 and, chroma before spatial, at factor 2 (spatial
// before chroma at factor 2 is excluded: the chroma counters then run over the decimated stream modulo the full width, and a
// lane's held sample need not lie among the pixels it loads), on frames that its units tile: 4 columns x f rows for
// k_dist_fast, the 8 x 8 window for k_ssim_fast.
int measure_kind(const csic_params &p, const Geometry &g, const Tune &t, MeasureFamily fam)
{
    const int tile_w = fam == MEASURE_DIST ? 4 : CSIC_SSIM_WINDOW, tile_h = fam == MEASURE_DIST ? g.f : CSIC_SSIM_WINDOW;
    if (t.force_generic || p.sampling != CSIC_SAMPLING_HOLD_DECIMATE || p.in_format != CSIC_FMT_ARGB8888) return 0;
    if (g.f > 2 || (g.f == 2 && g.s_first)) return 0;
    if (g.W % tile_w != 0 || g.H % tile_h != 0) return 0;
    // 32-bit offsets (in1n / in4n) and 24-bit row multiplies
    if ((int64_t)g.W * g.H > (1ll << 30) || g.W >= (1 << 24) || g.H >= (1 << 24)) return 0;
    return g.f;
}

const char *measure_kernel_name(MeasureFamily fam, int kind, const csic_params &p)
{
#define CSIC_MEASURE_NAMES(k) {k "_gen<hold>", k "_gen<hold,ycc-in>", k "_gen<avg>", k "_gen<avg,ycc-in>", k "_fast<f1>", k "_fast<f2>"}
    static const char *const names[2][6] = {CSIC_MEASURE_NAMES("k_dist"), CSIC_MEASURE_NAMES("k_ssim")};
#undef CSIC_MEASURE_NAMES
    const int gen = (p.sampling == CSIC_SAMPLING_AVG ? 2 : 0) + (p.in_format == CSIC_FMT_YCBCR888X ? 1 : 0);
    return names[fam == MEASURE_DIST ? 0 : 1][kind == 0 ? gen : 3 + kind];
}

CodeStatsKind code_stats_kind(int src_format, const Tune &t)
{
    if (t.force_generic || t.variant == 9) return CSTAT_GEN;
    if (src_format == CSIC_FMT_PLANAR_BITS) return CSTAT_BITS;
    return t.no_vec ? CSTAT_GEN : CSTAT_BYTES;         // k_cstat_bytes is 16-byte loads throughout
}

void code_stats_kernel_name(CodeStatsKind kind, int src_format, const csic_params &p, const Tune &t, char *buf, size_t len)
{
    const char *nt = t.no_nt ? "cached" : "nt";
    switch (kind) {
    case CSTAT_BYTES: snprintf(buf, len, "k_cstat_bytes<%s>", nt); break;
    case CSTAT_BITS: snprintf(buf, len, "k_cstat_bits<q%d,%d,%d,%s>", p.y_bits, p.cb_bits, p.cr_bits, nt); break;
    default: snprintf(buf, len, "k_cstat_gen<%s>", src_format == CSIC_FMT_PLANAR_BITS ? "bits" : "planar"); break;
    }
}

// ---- the plane units ------------------------------------------------------------------------------------------------------
// a flat launch (launch_flat) as a plane unit's plan
static void plane_flat(int64_t n, int K, int T, int nframes, PlaneLaunch *pl)
{
    LaunchPlan lp;
    launch_flat(n, K, T, nframes, &lp);
    *pl = PlaneLaunch{lp.grid, lp.block, T, lp.args.bdx, lp.args.bdy, lp.args.row_step};
}

// The packed-output plan whose k_avg the planar AVG tile kernel follows (same body, csic_avg_tile.h; same selection and geometry).
static csic_params packed_twin(csic_params p)
{
    p.out_format = CSIC_FMT_YCBCR888X;
    return p;
}

static PlanarKind planar_kind(const csic_params &p, const Geometry &g, const Tune &t, const csic_planar_layout &L)
{
    const bool general = t.variant == 9;                        // CSIC_TUNE_VARIANT 9: the general kernels (A/B, tests)
    if (p.sampling == CSIC_SAMPLING_AVG) {
        const bool f1_whole = g.f == 1 && g.W % 4 == 0 && g.H % g.v == 0;
        // factor 1 on frames of whole tiles: the dedicated kernel (Y bytes straight from the loaded pixels, no per-pixel write-back of
        // the block averages) is 3 points ahead of k_avg's body there -- 8192x8192 4:2:0: 77.5 against 74.1 % of the roofline,
        // profiles/r04_planar_avg_tile_ab.log; CSIC_TUNE_VARIANT 12 takes the tile body all the same (A/B, tests)
        if (!general && f1_whole && (t.variant != 12 || t.no_nt)) return PLANAR_AVG_F1;
        if (!general && !t.no_nt) {                             // k_avg's body wherever k_avg itself would run
            if (select_kernel(packed_twin(p), g, t, Constraints{false, false}).id.fam == FAM_AVG) return PLANAR_AVG_TILE;
        }
        return (!general && f1_whole) ? PLANAR_AVG_F1 : PLANAR_AVG_GEN;
    }
    if (general || L.module_width % 4 != 0) return PLANAR_FLAT_GEN;
    if (g.f == 1 && g.W % 4 == 0) return PLANAR_FLAT_F1X4;
    return t.variant == 10 ? PLANAR_FLAT_4PL : PLANAR_STRIDED;
}

int plan_planar(const csic_params &p, const Geometry &g, const Tune &t, uintptr_t align_bits, int nframes, PlanarPlan *pp)
{
    (void)align_bits;
    csic_planar_layout L;
    planar_layout(g, &p, &L);
    const int64_t n = (int64_t)g.Wo * g.Ho;
    pp->kind = planar_kind(p, g, t, L);
    fill_base_args(g, g.W, g.Wo, &pp->args);
    switch (pp->kind) {
    case PLANAR_AVG_TILE: {
        // k_avg's own geometry (block shape, edge blocks, XCD rotation): plan_launch on the plan's packed twin
        LaunchPlan lp;
        const int st = plan_launch(packed_twin(p), g, t, 0, nframes, 0, 0, &lp);
        if (st != CSIC_OK) return st;
        if (lp.id.fam != FAM_AVG) return set_error(CSIC_EHIP, "internal: the planar AVG tile kernel was selected for a plan k_avg does not take");
        pp->args = lp.args;
        static_cast<PlaneLaunch &>(*pp) = PlaneLaunch{lp.grid, lp.block, 256, lp.args.bdx, lp.args.bdy, lp.args.row_step};
        return CSIC_OK;
    }
    case PLANAR_STRIDED:                                        // 4 positions per lane, T * 4 positions per block
        plane_flat(n, 4, tune_block_threads(t, 256), nframes, pp);
        break;
    case PLANAR_FLAT_GEN:
    case PLANAR_FLAT_F1X4:
    case PLANAR_FLAT_4PL:
        // one-wave blocks for the 16-byte-load kernel: a wave's four loads then cover 4 KiB of consecutive pixels
        // (8192x8192 4:2:0: 71.7 % of the roofline with 256-thread blocks, 77.6 % with 64; profiles/r04_planar_bt.log)
        plane_flat((n + 3) / 4, PLANAR_K, tune_block_threads(t, pp->kind == PLANAR_FLAT_F1X4 ? 64 : 256), nframes, pp);
        break;
    case PLANAR_AVG_F1:
    case PLANAR_AVG_GEN: {
        // row-tiled kernels: lanes along x (tiles of 4 pixels for avg_f1 with 2 tiles per lane, output pixels for avg_gen), always
        // 256 threads.  Not launch_rows: these kernels clamp grid y at 65535 (launch_rows keeps one row back for edge blocks) and
        // leave KArgs.edge_y0 alone.
        const bool f1 = pp->kind == PLANAR_AVG_F1;
        const int lanes_x = f1 ? (g.W / 4 + 1) / 2 : g.Wo, rows = f1 ? g.H / g.v : g.Ho;
        const int bx = pow2_block_x(lanes_x, 256), by = 256 / bx;
        uint32_t gy = (uint32_t)((rows + by - 1) / by);
        if (gy > 65535u) gy = 65535u;
        static_cast<PlaneLaunch &>(*pp) = PlaneLaunch{Dim3{(uint32_t)((lanes_x + bx - 1) / bx), gy, (uint32_t)nframes},
                                                      Dim3{(uint32_t)bx, (uint32_t)by, 1}, 256, bx, by, (int32_t)gy * by};
        break;
    }
    }
    pp->args.bdx = pp->bdx; pp->args.bdy = pp->bdy; pp->args.row_step = pp->row_step;
    return CSIC_OK;
}

void planar_kernel_name(PlanarKind kind, const csic_params &p, const Geometry &g, const Tune &t, char *buf, size_t len)
{
    csic_planar_layout L;
    planar_layout(g, &p, &L);
    const char *rn = p.rounding == CSIC_ROUND_FLOOR_HW ? "floor" : "trunc";
    const char *nt = !t.no_nt ? "nt" : "cached";
    switch (kind) {
    case PLANAR_FLAT_GEN: snprintf(buf, len, "k_planar_flat<%s,general,h%d,v%d,%s>", rn, L.hold_h, L.hold_v, nt); break;
    case PLANAR_STRIDED: snprintf(buf, len, "k_planar_strided<%s,f%d,h%d,v%d,%s>", rn, g.f, L.hold_h, L.hold_v, nt); break;
    case PLANAR_FLAT_4PL: snprintf(buf, len, "k_planar_flat<%s,f%d,h%d,v%d,%s>", rn, g.f, L.hold_h, L.hold_v, nt); break;
    case PLANAR_FLAT_F1X4: snprintf(buf, len, "k_planar_flat<%s,f1x4,h%d,v%d,%s>", rn, L.hold_h, L.hold_v, nt); break;
    case PLANAR_AVG_F1: snprintf(buf, len, "k_planar_avg_f1<%s,h%d,v%d,%s>", rn, L.hold_h, L.hold_v, nt); break;
    case PLANAR_AVG_TILE: snprintf(buf, len, "k_planar_avg_tile<%s,f%d,h%d,v%d,nt>", rn, g.f, g.h, g.v); break;
    case PLANAR_AVG_GEN: snprintf(buf, len, "k_planar_avg_gen<%s,h%d,v%d>", rn, L.hold_h, L.hold_v); break;
    }
}

int plan_planar_bits(const csic_params &p, const Geometry &g, const Tune &t, uintptr_t in_align_bits, int nframes, BitsPlan *pp)
{
    csic_planar_layout L;
    planar_layout(g, &p, &L);
    const int64_t n = (int64_t)g.Wo * g.Ho;
    // the fast kernels assemble dwords of 32 samples inside one row: every row a whole number of 128 positions (hold_h <= 4)
    if (t.variant == 9 || p.sampling != CSIC_SAMPLING_HOLD_DECIMATE || L.module_width % 128 != 0) pp->kind = PBITS_GEN;
    else if (g.f == 1) pp->kind = (in_align_bits & 15u) ? PBITS_GEN : PBITS_F1;     // its 16-byte loads need a 16-byte aligned input
    else pp->kind = g.s_first ? PBITS_GEN : PBITS_STRIDED;
    // one-wave blocks for the 16-byte-load kernel (as k_planar_flat MODE 2), 256 threads for the others; k_pbits_gen: one lane per
    // group of 8 samples of Y, or of both chroma planes
    const int T = tune_block_threads(t, pp->kind == PBITS_F1 ? 64 : 256);
    const int K = pp->kind == PBITS_F1 ? PBITS_K : pp->kind == PBITS_STRIDED ? 4 : 1;
    const int64_t units = pp->kind == PBITS_F1 ? n / 4 : pp->kind == PBITS_STRIDED ? n : (n + 7) / 8 + (L.chroma_samples + 7) / 8;
    if (flat_blocks(units, K, T) > 0x7FFFFFFF) return set_error(CSIC_EINVAL_SIZE, "frame too large for one launch");
    plane_flat(units, K, T, nframes, pp);
    return CSIC_OK;
}

void planar_bits_kernel_name(BitsKind kind, const csic_params &p, const Geometry &g, const Tune &t, char *buf, size_t len)
{
    csic_planar_layout L;
    planar_layout(g, &p, &L);
    const char *rn = p.rounding == CSIC_ROUND_FLOOR_HW ? "floor" : "trunc";
    const char *nt = !t.no_nt ? "nt" : "cached";
    switch (kind) {
    case PBITS_F1: snprintf(buf, len, "k_pbits_f1<%s,h%d,v%d,%s>", rn, L.hold_h, L.hold_v, nt); break;
    case PBITS_STRIDED: snprintf(buf, len, "k_pbits_strided<%s,f%d,h%d,%s>", rn, g.f, L.hold_h, nt); break;
    case PBITS_GEN:
        snprintf(buf, len, "k_pbits_gen<%s,%s,h%d,v%d>", rn, p.sampling == CSIC_SAMPLING_AVG ? "avg" : "hold", L.hold_h, L.hold_v);
        break;
    }
}

int plan_reconstruct(const Geometry &g, const Tune &t, int32_t module_width, int K, int nframes, ReconPlan *pp)
{
    pp->fast = module_width % 4 == 0 && t.variant != 9;
    plane_flat(((int64_t)g.Wo * g.Ho + 3) / 4, K, tune_block_threads(t, 64), nframes < 65535 ? nframes : 65535, pp);
    pp->bdx = pp->bdy = pp->row_step = 0;                       // the reconstruct kernels read none of KArgs
    return CSIC_OK;
}

void reconstruct_kernel_name(int src_format, int out_format, bool fast, const Tune &t, char *buf, size_t len)
{
    snprintf(buf, len, "%s<%s,%s,%s>", src_format == CSIC_FMT_PLANAR_BITS ? "k_rbits" : "k_recon", out_format == CSIC_FMT_ARGB8888 ? "argb" : "ycc",
             fast ? "fast" : "slow", !t.no_nt ? "nt" : "cached");
}

int plan_decode(const csic_params &p, const Geometry &g, const Tune &t, int src_format, uintptr_t align_bits, int nframes, DecodePlan *pp)
{
    const bool planar = src_format == CSIC_FMT_PLANAR || src_format == CSIC_FMT_PLANAR_BITS;
    const int64_t out_px = (int64_t)g.W * g.H;
    const int nz = nframes < 65535 ? nframes : 65535, T = tune_block_threads(t, 256);
    pp->recon_fast = false;
    if (t.variant == 9 || t.force_generic || t.no_vec || (align_bits & 15u)) pp->kind = DEC_GEN;
    // the reconstruct kernels store 16 bytes at a time from each frame's base: frames after the first start 4 W H bytes further on
    else if (g.f == 1 && planar && (nframes == 1 || out_px % 4 == 0)) pp->kind = DEC_RECON;
    // width % 4 == 0 is all a planar source needs too: the module width is W or out_width, a multiple of NP (4 at factor 1, 2 at 2, 1
    // above), and so is every piece's first stream position
    else if (g.W % 4 != 0 || out_px > ((int64_t)1 << 30)) pp->kind = DEC_GEN;
    else pp->kind = DEC_FAST;
    switch (pp->kind) {
    case DEC_RECON: {
        csic_planar_layout L;
        planar_layout(g, &p, &L);
        ReconPlan rp;
        plan_reconstruct(g, t, L.module_width, src_format == CSIC_FMT_PLANAR_BITS ? RBITS_K : RECON_K, nframes, &rp);
        static_cast<PlaneLaunch &>(*pp) = rp;
        pp->recon_fast = rp.fast;
        return CSIC_OK;
    }
    // a lane takes dec_pieces_per_lane 16-byte pieces of the output, W / 4 of them to a row of the source
    case DEC_FAST: plane_flat((int64_t)(g.W / 4) * g.Ho, dec_pieces_per_lane(g.f), T, nz, pp); break;
    case DEC_GEN: plane_flat(out_px, 1, T, nz, pp); break;     // one output pixel per lane
    }
    pp->bdx = pp->bdy = pp->row_step = 0;                       // DecArgs carries T only
    return CSIC_OK;
}

void decode_kernel_name(const DecodePlan &pp, const Geometry &g, const Tune &t, int src_format, int out_format, char *buf, size_t len)
{
    // an ARGB source runs the YCbCr -> YCbCr instantiation (a copy): the name is the kernel's, as a profiler shows it
    const char *fmt = out_format == CSIC_FMT_ARGB8888 && src_format != CSIC_FMT_ARGB8888 ? "argb" : "ycc";
    const char *src = src_format == CSIC_FMT_PLANAR_BITS ? "bits" : src_format == CSIC_FMT_PLANAR ? "planar" : "ycc";
    switch (pp.kind) {
    case DEC_RECON: reconstruct_kernel_name(src_format, out_format, pp.recon_fast, t, buf, len); break;
    case DEC_FAST: snprintf(buf, len, "k_decode<%s,%s,f%d,%s>", src, fmt, g.f, !t.no_nt ? "nt" : "cached"); break;
    case DEC_GEN: snprintf(buf, len, "k_decode_gen<%s,%s>", src, fmt); break;
    }
}

// ---- view decode ------------------------------------------------------------------------------------------------------------
int check_view(const Geometry &g, const csic_view &v)
{
    const int s = v.scale;
    if (s != 1 && s != 2 && s != 4 && s != 8 && s != 16)
        return set_error(CSIC_EINVAL_SIZE, "a view's scale is 1, 2, 4, 8 or 16. Got %d", s);
    if (v.x0 < 0 || v.y0 < 0 || v.width < 1 || v.height < 1 || (int64_t)v.x0 + (int64_t)v.width * s > g.W || (int64_t)v.y0 + (int64_t)v.height * s > g.H)
        return set_error(CSIC_EINVAL_SIZE, "the view %d x %d at (%d, %d), scale %d, does not lie inside the %d x %d frame", v.width, v.height,
                         v.x0, v.y0, s, g.W, g.H);
    return CSIC_OK;
}

// the most decimated cells a box of s pixels can touch along one axis when boxes start at origin + k s
static int view_cells(int origin, int s, int f)
{
    if (s >= f) return s / f + (origin % f != 0 ? 1 : 0);      // f divides s: every box starts at the same offset inside a cell
    return origin % s != 0 ? 2 : 1;                            // s divides f: a box that starts at a multiple of s stays inside one cell
}

int plan_view(const Geometry &g, const Tune &t, const csic_view &v, uintptr_t align_bits, int nframes, ViewPlan *pp)
{
    const int64_t px = (int64_t)v.width * v.height;
    const int nz = nframes < 65535 ? nframes : 65535;
    const bool general = t.variant == 9 || t.force_generic || t.no_vec;
    pp->kind = (general || (align_bits & 15u) || v.width % VIEW_PX != 0 || px > ((int64_t)1 << 30)) ? VIEW_GEN : VIEW_FAST;
    pp->ls = 0;
    while ((1 << pp->ls) < v.scale) ++pp->ls;
    pp->units_per_row = pp->kind == VIEW_FAST ? v.width / VIEW_PX : v.width;
    pp->units = (int64_t)pp->units_per_row * v.height;
    pp->ncx = view_cells(v.x0, v.scale, g.f);
    pp->ncy = view_cells(v.y0, v.scale, g.f);
    // a lane of k_view walks 4 boxes: one-wave blocks spread a small view over the device; k_view_gen as k_decode_gen
    plane_flat(pp->units, 1, tune_block_threads(t, pp->kind == VIEW_FAST ? 64 : 256), nz, pp);
    pp->bdx = pp->bdy = pp->row_step = 0;
    return CSIC_OK;
}

void view_kernel_name(const ViewPlan &pp, const Tune &t, int src_format, int out_format, char *buf, size_t len)
{
    // an ARGB source runs the YCbCr -> YCbCr instantiation, as in decode_kernel_name
    const char *fmt = out_format == CSIC_FMT_ARGB8888 && src_format != CSIC_FMT_ARGB8888 ? "argb" : "ycc";
    const char *src = src_format == CSIC_FMT_PLANAR_BITS ? "bits" : src_format == CSIC_FMT_PLANAR ? "planar" : "ycc";
    if (pp.kind == VIEW_FAST) snprintf(buf, len, "k_view<s%d,%s,%s,%s>", 1 << pp.ls, src, fmt, !t.no_nt ? "nt" : "cached");
    else snprintf(buf, len, "k_view_gen<%s,%s>", src, fmt);
}

} // namespace csic
