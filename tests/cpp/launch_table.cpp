// launch_table.cpp -- the launch table of the packed kernels, without a GPU: for a structured sweep of parameter sets, knobs,
// batch sizes, alignments and pitches, one line with what csic_select.cpp decides -- status, kernel name, grid, block, the
// block geometry in KArgs and a hash of the other KArgs scalars.  tests/test_launch_table.py compares the output with
// tests/data/launch_table.txt, so a change of a selection or geometry rule shows in that file's diff which shapes moved where.
// For every case the program also asserts what must hold whatever the rules are (check_invariants).
//   launch_table            the committed sweep (thinned: every rule's boundary on both sides, a few hundred lines)
//   launch_table --full     the whole cross product (for comparing two revisions; large)
//   launch_table --check    the whole cross product, invariants only, nothing printed (the sanitizer build runs this)
// g++ -std=c++17, host only: links csic_select.cpp and csic_host.cpp.
//
// Line (3 / 3 / 2 bits kept throughout): WxH a:b f order sampling out in rounding [| variant force_generic no_vec no_nt block_threads]
//       [| nframes align in_pitch,out_pitch] -> status name t=template arguments g=grid b=block a=bdx,bdy,row_step,edge_y0 h=hash
// (the bracketed groups only where they differ from no knob / one frame, 16-byte-aligned pointers, packed rows)
// After the launches, the committed sweep prints what the measurement units take (measure_kind, measure_kernel_name) for each of
// its distinct parameter sets, one line per unit:
//       measure WxH a:b f order sampling in rounding [| g1] -> dist|ssim kind name
// (neither the output format nor, of the knobs, anything but force_generic enters that choice)
// Last come the plane units (plan_planar, plan_planar_bits, plan_reconstruct, plan_decode), one section each, the same head fields
// with the plane format as `out` (what reconstruct and decode READ; `to-` is what they write):
//       planar|bits|recon|decode <head> [to-argb|to-ycc] -> status name g=grid b=block a=bdx,bdy,row_step T=threads [h=hash]
// (h: the KArgs of the packed twin whose k_avg launch k_planar_avg_tile follows; --full adds the kind's number)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <set>
#include <string>
#include <vector>

#include "csic.h"
#include "csic_select.h"

using namespace csic;

struct Case {
    csic_params p;
    Tune t;
    int nframes;
    unsigned align;          // OR of the frame pointers' low bits (0 = 16-byte aligned, 4 = 4-byte aligned)
    int32_t ip, op;          // row pitches in pixels (0 = packed)
};

struct Result {
    int status;
    char name[96], targs[64];    // the kernel's name and its template arguments
    LaunchPlan lp;
};

// The template arguments a KernelId stands for, in the kernel's own order (what resolve() in csic_kernels.hip instantiates)
static void template_args(const KernelId &id, char *buf, size_t len)
{
    switch (id.fam) {
    case FAM_F1X4:
    case FAM_F1FLAT: std::snprintf(buf, len, "%d,%d,%d,%d,%d", id.round, id.fmt, id.h, id.v, id.nt); break;
    case FAM_DEC:
    case FAM_DECFLAT: std::snprintf(buf, len, "%d,%d,%d,%d,%d,%d,%d", id.round, id.fmt, id.f, id.h, id.srows, DEC_K, id.nt); break;
    case FAM_DEC2V1:
    case FAM_DEC2V2: std::snprintf(buf, len, "%d,%d,%d,%d", id.round, id.fmt, id.fam == FAM_DEC2V1 ? 1 : 2, id.nt); break;
    case FAM_AVG: std::snprintf(buf, len, "%d,%d,%d,%d,%d,%d,%d", id.round, id.fmt, id.f, id.h, id.v, id.nt, id.tiles); break;
    case FAM_AVG_GENERIC:
    case FAM_GENERIC: std::snprintf(buf, len, "%d,%d,%d", id.round, id.fmt, id.infmt); break;
    case FAM_FLATGEN: std::snprintf(buf, len, "%d,%d,%d,%d", id.round, id.fmt, DEC_K, id.nt); break;
    case FAM_PLANAR: buf[0] = 0; break;
    }
}

static Result run_case(const Case &c, const Geometry &g)
{
    Result r{};
    r.status = plan_launch(c.p, g, c.t, c.align, c.nframes, c.ip, c.op, &r.lp);
    if (r.status != CSIC_OK) return r;
    kernel_name(r.lp.id, g, r.name, sizeof r.name);
    template_args(r.lp.id, r.targs, sizeof r.targs);
    return r;
}

static bool g_print = true, g_fields = false;
static std::vector<std::string> g_measure;      // the measurement section, in the order of the cases' first appearance
static std::set<std::string> g_measure_seen;
static long g_cases = 0, g_failed = 0;

static uint32_t fnv(uint32_t h, uint64_t v)
{
    for (int i = 0; i < 8; ++i) { h ^= (uint32_t)(v >> (8 * i)) & 0xFFu; h *= 16777619u; }
    return h;
}

static uint32_t args_hash(const KArgs &a)
{
    uint32_t h = 2166136261u;
    for (uint64_t v : {(uint64_t)a.W, (uint64_t)a.H, (uint64_t)a.Wo, (uint64_t)a.Ho, (uint64_t)a.last_sample_col, (uint64_t)a.my,
                       (uint64_t)a.mcb, (uint64_t)a.mcr, (uint64_t)a.f, (uint64_t)a.hmask, (uint64_t)a.vmask, (uint64_t)a.s_first,
                       (uint64_t)a.sc_shift, (uint64_t)a.bc_row_off, (uint64_t)a.bc_col_in, (uint64_t)a.in_frame_px,
                       (uint64_t)a.out_frame_px, (uint64_t)a.ip, (uint64_t)a.op, (uint64_t)a.mW, (uint64_t)a.mWo, (uint64_t)a.kW,
                       (uint64_t)a.kWo})
        h = fnv(h, v);
    return h;
}

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { std::fprintf(stderr, "invariant failed: %s\n", #cond); ok = false; } \
    } while (0)

// What must hold for every launch, whatever the selection and geometry rules are.
static bool check_invariants(const Case &c, const Geometry &g, const LaunchPlan &lp)
{
    bool ok = true;
    const KArgs &a = lp.args;
    const Family fam = lp.id.fam;
    const int32_t ip = c.ip > 0 ? c.ip : g.W, op = c.op > 0 ? c.op : g.Wo;
    const uint64_t threads = (uint64_t)lp.block.x * lp.block.y * lp.block.z;
    REQUIRE(threads >= 1 && threads <= 256 && lp.block.z == 1);
    REQUIRE(lp.grid.x >= 1 && lp.grid.y >= 1 && lp.grid.y <= 65535 && lp.grid.z == (uint32_t)c.nframes);
    REQUIRE(a.bdx == (int32_t)lp.block.x && a.bdy == (int32_t)lp.block.y && a.ip == ip && a.op == op);
    REQUIRE(a.in == nullptr && a.out == nullptr && a.in_tab == nullptr && a.out_tab == nullptr);
    const bool flat = fam == FAM_DECFLAT || fam == FAM_FLATGEN || fam == FAM_F1FLAT;
    const bool vec = fam == FAM_F1X4 || fam == FAM_F1FLAT || fam == FAM_DEC2V1 || fam == FAM_DEC2V2;
    // a family with 16-byte accesses at 16-byte addresses never meets pointers or pitches that are only 4-byte aligned
    if (vec) REQUIRE((c.align & 15u) == 0 && ((ip | op) & 3) == 0 && g.W % 4 == 0);
    if (flat) {
        // 32-bit byte offsets inside a frame, 24-bit row multiplies
        REQUIRE((int64_t)(g.H - 1) * ip + g.W <= (1ll << 30) && (int64_t)(g.Ho - 1) * op + g.Wo <= (1ll << 30));
        REQUIRE(g.H < (1 << 24) && (int64_t)ip * g.f < (1 << 24) && op < (1 << 24));
        const uint64_t n = fam == FAM_F1FLAT ? (uint64_t)(g.W / 4) * g.H : (uint64_t)g.Wo * g.Ho;
        REQUIRE((uint64_t)lp.grid.x * lp.block.x * 4 >= n && lp.block.y == 1 && lp.grid.y == 1 && lp.block.x % 64 == 0);
        return ok;
    }
    // row families: units along x, K per lane; rows along y, strided by row_step past the grid
    int units = g.Wo, K = 1, rows = g.Ho;
    if (fam == FAM_F1X4) { units = g.W / 4; rows = g.H; }
    else if (fam == FAM_DEC) K = DEC_K;
    else if (fam == FAM_DEC2V1) units = g.Wo / 2;
    else if (fam == FAM_DEC2V2) units = g.Wo / 4;
    else if (fam == FAM_AVG) { const int th = g.f > g.v ? g.f : g.v; units = (g.W + 3) / 4; K = lp.id.tiles; rows = (g.H + th - 1) / th; }
    REQUIRE((uint64_t)lp.grid.x * lp.block.x * K >= (uint64_t)units);
    const uint32_t gy = fam == FAM_AVG ? (uint32_t)a.edge_y0 : lp.grid.y;
    REQUIRE(gy >= 1 && gy <= lp.grid.y && a.row_step == (int32_t)(gy * lp.block.y) && rows >= 1);
    if (fam == FAM_DEC && lp.id.h > 1) REQUIRE(lp.block.x % lp.id.h == 0 || lp.grid.x == 1);   // a DPP hold group inside one block row
    if (fam == FAM_AVG) {
        // one lane of the edge blocks for every output pixel that no whole tile produces
        const int th = g.f > g.v ? g.f : g.v, W4 = g.W / 4, ntr = g.H / th;
        const int Cw = g.f == 8 ? W4 / 2 : W4 * (4 / g.f), Rw = g.f == 8 ? ntr : ntr * (th / g.f);
        const int64_t nedge = (int64_t)(g.Wo - Cw) * g.Ho + (int64_t)(g.Ho - Rw) * Cw;
        REQUIRE((int64_t)(lp.grid.y - gy) * lp.grid.x * (int64_t)threads >= nedge);
        // f = 8: the two tiles of an output are neighbouring lanes of one quad, so no block may start on an odd tile
        if (g.f == 8 && lp.grid.x > 1) REQUIRE(lp.block.x % 4 == 0);
    } else {
        REQUIRE(a.edge_y0 == 0x7FFFFFFF);
    }
    return ok;
}

// the measurement units' lines of one parameter set, once
static void note_measure(const Case &c, const Geometry &g)
{
    const csic_params &p = c.p;
    char head[192];
    std::snprintf(head, sizeof head, "measure %dx%d %d:%d f%d o%d%d%d %s %s %s%s", p.width, p.height, p.chroma_a, p.chroma_b, p.factor, p.op[0], p.op[1],
                  p.op[2], p.sampling == CSIC_SAMPLING_AVG ? "avg" : "hold", p.in_format == CSIC_FMT_ARGB8888 ? "argb" : "ycc",
                  p.rounding == CSIC_ROUND_FLOOR_HW ? "floor" : "trunc", c.t.force_generic ? " | g1" : "");
    if (!g_measure_seen.insert(head).second) return;
    for (MeasureFamily fam : {MEASURE_DIST, MEASURE_SSIM}) {
        const int kind = measure_kind(p, g, c.t, fam);
        char line[256];
        std::snprintf(line, sizeof line, "%s -> %s %d %s", head, fam == MEASURE_DIST ? "dist" : "ssim", kind, measure_kernel_name(fam, kind, p));
        g_measure.push_back(line);
    }
}

static const char *format_word(int fmt)
{
    return fmt == CSIC_FMT_ARGB8888 ? "argb" : fmt == CSIC_FMT_YCBCR888X ? "ycc" : fmt == CSIC_FMT_PLANAR ? "planar" : "bits";
}

// the head fields of a line; validates the case and derives its geometry
static void case_head(const Case &c, Geometry *g, char *head, size_t len)
{
    if (derive_geometry(&c.p, g) != CSIC_OK) { std::fprintf(stderr, "bad case: %s\n", csic_last_error()); std::exit(2); }
    const csic_params &p = c.p;
    // knobs and launch settings are printed only where they differ from the default (no knob, one frame, aligned, packed)
    char knobs[96] = "", at[96] = "";
    if (c.t.variant || c.t.force_generic || c.t.no_vec || c.t.no_nt || c.t.block_threads)
        std::snprintf(knobs, sizeof knobs, " | v%d g%d n%d c%d b%d", c.t.variant, c.t.force_generic, c.t.no_vec, c.t.no_nt, c.t.block_threads);
    if (c.nframes != 1 || c.align || c.ip || c.op) std::snprintf(at, sizeof at, " | n%d a%u p%d,%d", c.nframes, c.align, c.ip, c.op);
    std::snprintf(head, len, "%dx%d %d:%d f%d o%d%d%d %s %s %s %s%s%s", p.width, p.height, p.chroma_a, p.chroma_b, p.factor, p.op[0],
                  p.op[1], p.op[2], p.sampling == CSIC_SAMPLING_AVG ? "avg" : "hold", format_word(p.out_format),
                  p.in_format == CSIC_FMT_ARGB8888 ? "argb" : "ycc", p.rounding == CSIC_ROUND_FLOOR_HW ? "floor" : "trunc", knobs, at);
}

static void emit(const Case &c)
{
    Geometry g;
    char head[256];
    case_head(c, &g, head, sizeof head);
    if (g_print && !g_fields) note_measure(c, g);
    const Result r = run_case(c, g);
    ++g_cases;
    if (r.status != CSIC_OK) {
        if (g_print) std::printf("%s -> %d\n", head, r.status);
        return;
    }
    if (!check_invariants(c, g, r.lp)) { std::fprintf(stderr, "  in: %s -> %s\n", head, r.name); ++g_failed; }
    if (!g_print) return;
    const LaunchPlan &lp = r.lp;
    const KArgs &a = lp.args;
    std::printf("%s -> 0 %s t=%s g=%u,%u,%u b=%u,%u,%u a=%d,%d,%d,%d h=%08x", head, r.name, r.targs, lp.grid.x, lp.grid.y, lp.grid.z, lp.block.x, lp.block.y,
                lp.block.z, a.bdx, a.bdy, a.row_step, a.edge_y0, args_hash(a));
    if (g_fields)
        std::printf(" W%d H%d Wo%d Ho%d lsc%d m%x,%x,%x f%d hm%d vm%d sf%d sh%d br%d bc%d fp%" PRId64 ",%" PRId64 " ip%d op%d mg%u,%u,%u,%u", a.W, a.H, a.Wo,
                    a.Ho, a.last_sample_col, a.my, a.mcb, a.mcr, a.f, a.hmask, a.vmask, a.s_first, a.sc_shift, a.bc_row_off, a.bc_col_in,
                    a.in_frame_px, a.out_frame_px, a.ip, a.op, a.mW, a.mWo, a.kW, a.kWo);
    std::printf("\n");
}

// ---- the sweep ------------------------------------------------------------------------------------------------------
struct Shape { int w, h; };
// the shapes the selection and geometry comments and profiles/ name, then tiny and degenerate ones
static const Shape SHAPES[] = {{8192, 8192}, {16384, 4096}, {8192, 2048}, {7680, 4320}, {3840, 2160}, {1920, 1080}, {1922, 1082}, {1280, 720},
                               {1366, 768}, {1368, 768}, {1028, 64}, {1000, 1000}, {1001, 1001}, {1024, 1024}, {1032, 8}, {720, 480},
                               {640, 480}, {512, 512}, {352, 288}, {128, 128}, {1, 1}, {3, 5}, {2, 64}, {7, 3}, {9, 9}, {40, 2}};
static const int NSHAPES = (int)(sizeof SHAPES / sizeof SHAPES[0]);
static const int CHROMA[6][2] = {{4, 4}, {2, 2}, {2, 0}, {1, 1}, {4, 0}, {1, 0}};
static const int ORDERS[6][3] = {{3, 1, 2}, {1, 3, 2}, {3, 2, 1}, {2, 3, 1}, {1, 2, 3}, {2, 1, 3}};   // [0]: chroma first, [1]: spatial first
static const int FACTORS[4] = {1, 2, 4, 8};

static Case make(Shape s, int chroma, int f, int order, bool avg)
{
    Case c{};
    csic_params_default(&c.p, s.w, s.h);
    c.p.chroma_a = CHROMA[chroma][0]; c.p.chroma_b = CHROMA[chroma][1];
    c.p.y_bits = 3; c.p.cb_bits = 3; c.p.cr_bits = 2;
    c.p.factor = f;
    std::memcpy(c.p.op, ORDERS[avg ? 0 : order], sizeof c.p.op);
    c.p.sampling = avg ? CSIC_SAMPLING_AVG : CSIC_SAMPLING_HOLD_DECIMATE;
    c.nframes = 1;
    return c;
}

// every knob setting the table covers: variants 0-12, each other knob on its own, each block size
static const int NTUNES = 13 + 3 + 3;
static Tune tune_set(int k)
{
    Tune t{};
    if (k < 13) t.variant = k;
    else if (k == 13) t.force_generic = 1;
    else if (k == 14) t.no_vec = 1;
    else if (k == 15) t.no_nt = 1;
    else t.block_threads = 64 << (k - 16);
    return t;
}

// the launch-time variations of one case: batch sizes, 4-byte-aligned pointers, padded pitches (by 256 pixels and by 1)
static void emit_launches(Case c, bool all)
{
    Geometry g;
    derive_geometry(&c.p, &g);
    for (int nf : {1, 64, 65535}) {
        c.nframes = nf; c.align = 0; c.ip = c.op = 0;
        if (nf != 1 || all) emit(c);
        if (nf != 1 && !all) continue;
        c.align = 4; emit(c);
        c.align = 0; c.ip = g.W + 256; c.op = g.Wo + 256; emit(c);
        if (all || nf == 1) { c.ip = g.W + 1; c.op = g.Wo + 1; emit(c); }
    }
}

static void sweep_full()
{
    for (int s = 0; s < NSHAPES; ++s)
        for (int ch = 0; ch < 6; ++ch)
            for (int f : FACTORS)
                for (int o = 0; o < 7; ++o)                               // 6 orders of the reference's sampling, then AVG
                    for (int fmt = 0; fmt < 4; ++fmt) {                   // output format x input format
                        Case c = make(SHAPES[s], ch, f, o % 6, o == 6);
                        c.p.out_format = (fmt & 1) ? CSIC_FMT_YCBCR888X : CSIC_FMT_ARGB8888;
                        c.p.in_format = (fmt & 2) ? CSIC_FMT_YCBCR888X : CSIC_FMT_ARGB8888;
                        c.p.rounding = (s + ch + o) & 1 ? CSIC_ROUND_TRUNC_SW : CSIC_ROUND_FLOOR_HW;
                        for (int k = 0; k < NTUNES; ++k) { c.t = tune_set(k); emit(c); }
                        c.t = Tune{};
                        emit_launches(c, true);
                    }
}

static void hold_cases(Shape sh, int ch)                                    // every factor, both order classes (one at factor 1, where they coincide)
{
    for (int f : FACTORS)
        for (int o = 0; o < (f == 1 ? 1 : 2); ++o) emit(make(sh, ch, f, o, false));
}

static void sweep_committed()
{
    // 1. the reference's sampling: every shape at 4:2:0; the other hold distances (4:4:4, 4:2:2, 4:1:1) on a wide, a ragged, a
    //    one-wave and a tiny shape; 4:4:0 / 4:1:0 and the four remaining orders on the ragged one
    for (int s = 0; s < NSHAPES; ++s) hold_cases(SHAPES[s], 2);
    for (int s : {5, 11, 18, 21})
        for (int ch : {0, 1, 3}) hold_cases(SHAPES[s], ch);
    for (int ch : {4, 5}) hold_cases(SHAPES[11], ch);
    for (int f : {2, 8})
        for (int o = 2; o < 6; ++o) emit(make(SHAPES[11], 2, f, o, false));
    // 2. the AVG sampling: every shape x 4:2:0 x factor; 4:4:4 / 4:1:1 / 4:1:0 on a wide and a ragged shape
    for (int s = 0; s < NSHAPES; ++s)
        for (int f : FACTORS) emit(make(SHAPES[s], 2, f, 0, true));
    for (int s : {5, 12})
        for (int ch : {0, 3, 5})
            for (int f : FACTORS) emit(make(SHAPES[s], ch, f, 0, true));
    // 3. YCbCr output, the software rounding, YCbCr input
    for (int s : {5, 11})
        for (int f : {1, 2})
            for (int avg = 0; avg < 2; ++avg) {
                Case c = make(SHAPES[s], 2, f, 1, avg != 0);
                c.p.out_format = CSIC_FMT_YCBCR888X; emit(c);
                c.p.rounding = CSIC_ROUND_TRUNC_SW; emit(c);
                c.p.in_format = CSIC_FMT_YCBCR888X; emit(c);
            }
    // 4. the knobs on 1920x1080 (chroma first, spatial first, AVG): every variant that selection reads, force-generic, no-vector,
    //    cached accesses; the variants of the planar formats (3 is unused) once; k_dec / k_decflat A/B on a ragged and a one-wave shape
    for (int f : {1, 2, 8})
        for (int kind = 0; kind < 3; ++kind)
            for (int k : {1, 2, 4, 5, 6, 7, 8, 11, 13, 14, 15}) {
                Case c = make(SHAPES[5], 2, f, kind == 1, kind == 2);
                c.t = tune_set(k);
                emit(c);
            }
    for (int k : {3, 9, 10, 12}) { Case c = make(SHAPES[5], 2, 2, 0, false); c.t = tune_set(k); emit(c); }
    for (int s : {11, 17})
        for (int o = 0; o < 2; ++o)
            for (int k : {5, 6, 7}) { Case c = make(SHAPES[s], 2, 2, o, false); c.t = tune_set(k); emit(c); }
    for (int s : {0, 9})                                                  // block sizes and the rules they switch off
        for (int f : {1, 2, 4})
            for (int avg = 0; avg < 2; ++avg)
                for (int k = 16; k < NTUNES; ++k) {
                    Case c = make(SHAPES[s], 2, f, 0, avg != 0);
                    c.t = tune_set(k);
                    emit(c);
                }
    for (int s : {6, 9, 12, 14})                                          // AVG on ragged shapes: variant 8 keeps whole tiles only
        for (int f : {2, 8}) {
            Case c = make(SHAPES[s], 2, f, 0, true);
            c.t.variant = 8;
            emit(c);
        }
    // 5. at launch: batches (one-frame rules, the XCD rotation of k_avg's edge blocks), 4-byte-aligned pointers, padded pitches
    for (int s : {0, 6, 17})
        for (int f : {1, 2, 8})
            for (int avg = 0; avg < 2; ++avg) emit_launches(make(SHAPES[s], 2, f, 0, avg != 0), false);
}

// One case with a variant, a batch size and pitches of its own (sweep_rules)
static void rule(Shape sh, int ch, int f, int order, bool avg, int variant = 0, int nframes = 1, int32_t ip = 0, int32_t op = 0,
                 unsigned align = 0)
{
    Case c = make(sh, ch, f, order, avg);
    c.t.variant = variant; c.nframes = nframes; c.ip = ip; c.op = op; c.align = align;
    emit(c);
}

// Shapes chosen rule by rule, one on each side of every comparison of csic_select.cpp that the named shapes above leave untouched
// (flipping any comparison or constant there must move a line of the table).  Variant 5 keeps k_dec, variant 11 k_f1x4.
static void sweep_rules()
{
    // k_dec, 128-thread blocks: one frame only; rows of whole 128-lane blocks (7680: 960 lanes, 1020 x 21940: 128 lanes of a ragged
    // row); >= 64 MB (8192 x 2730 / 2732 around it, 8192 x 2048 well below)
    for (Shape sh : {Shape{8192, 8192}, Shape{16384, 4096}, Shape{8192, 2048}, Shape{7680, 4320}, Shape{8192, 2730}, Shape{8192, 2732},
                     Shape{1020, 21940}})
        for (int nf : {1, 64}) rule(sh, 2, 2, 0, false, 5, nf);
    rule(Shape{8192, 8192}, 2, 4, 0, false, 5);
    rule(Shape{3072, 7300}, 2, 2, 0, false, 5);                          // 384 lanes: three blocks of 128, >= 64 MB
    // k_dec, block width without a hold: 257 lanes (two blocks, no divisor), 387 (3 x 129: the last divisor tried)
    for (int w : {2056, 3096}) rule(Shape{w, 64}, 2, 2, 0, false, 5, 64);
    // k_dec, block width (dec_block_x) with a lane hold of 2 (4:1:1, chroma first) and 4 (4:1:1, spatial first): rows of 270 lanes
    // (135 is no multiple of the hold; 90 lies below half a block), 125 and 126 lanes (one block), 250 / 252 lanes
    for (Shape sh : {Shape{2160, 64}, Shape{1000, 64}, Shape{1008, 64}, Shape{2000, 64}, Shape{2016, 64}})
        for (int o = 0; o < 2; ++o) rule(sh, 3, 2, o, false, 5, 64);
    // k_dec's one-wave blocks and k_decflat's `hold | Wo`: 100 lanes (50 divides, but is no multiple of a hold of 4), 126 lanes
    // (63, hold 2), 42 lanes at f = 4 (no multiple of 4), an odd output width with a hold of 2, 15 / 16 and 128 / 129 lanes
    for (int o = 0; o < 2; ++o) {
        rule(Shape{800, 64}, 3, 2, o, false);
        rule(Shape{1008, 64}, 3, 2, o, false);
        rule(Shape{672, 64}, 3, 4, o, false);
        rule(Shape{1001, 64}, 3, 2, o, false);
    }
    rule(Shape{1008, 64}, 2, 4, 1, false);                               // 63 lanes, hold 2, f = 4
    for (int f : {4, 8}) rule(Shape{60 * f, 64}, 2, f, 0, false);        // 15 lanes
    rule(Shape{752, 64}, 2, 2, 0, false);                                // 94 lanes = 2 x 47
    for (int w : {120, 128, 384, 392, 1024, 1032, 504, 512, 520})
        for (int f : {2, 4}) rule(Shape{w, 64}, 2, f, 0, false);
    // k_decflat's block size: f = 2 or output rows of >= 512 pixels take 128 threads (2044 / 2048 wide at f = 4)
    for (int w : {2044, 2048}) rule(Shape{w, 64}, 2, 4, 0, false, 6);
    // k_dec2v (variants 1 / 2): W % 8 == 0; 2 and 4 output pixels per lane
    for (int w : {1000, 1004, 2560})
        for (int v : {1, 2}) rule(Shape{w, 64}, 2, 2, 0, false, v);
    rule(Shape{1004, 64}, 2, 2, 0, false, 1, 1, 1004, 504);              // W % 8 != 0 with an output pitch that would be aligned
    // k_flatgen yields to k_generic under variant 7 only
    for (int v : {6, 7, 8}) rule(Shape{1001, 64}, 2, 2, 1, false, v);
    // only 4-byte-aligned pointers: k_f1x4 and k_dec2v give way to k_dec
    rule(Shape{1920, 1080}, 2, 1, 0, false, 11, 1, 0, 0, 4);
    rule(Shape{1920, 1080}, 2, 2, 0, false, 1, 1, 0, 0, 4);
    rule(Shape{1920, 1080}, 2, 2, 0, false, 2, 1, 0, 0, 4);
    // the quads of a hold need 3 lanes in a row (dec_fast_ok): 8 / 9 output pixels
    for (int w : {16, 18, 32, 36})
        for (int o = 0; o < 2; ++o) rule(Shape{w, 16}, 3, 2, o, false);
    // k_f1x4's block width (variant 11): 320 lanes (5 x 64), 342 (256 + rest), 250 and 255 (one partly filled block), 256, 257,
    // 192, 128, 96
    for (int w : {1280, 1368, 1000, 1020, 1024, 1028, 768, 512, 384}) rule(Shape{w, 64}, 2, 1, 0, false, 11, 64);
    // k_avg's blocks: whole waves for 320 / 384 / 448 lanes, not for 512 or 640; equal blocks for up to 8 blocks a row (1800 lanes
    // against 2100), none for one block (250); the first whole tile (4 x 2 pixels at f <= 2, 8 x 8 at f = 8)
    for (int w : {768, 1280, 1536, 1792, 2048, 2560, 7200, 8400, 1000}) rule(Shape{w, 64}, 2, 4, 0, true, 0, 64);
    for (Shape sh : {Shape{3, 8}, Shape{4, 1}, Shape{4, 2}}) rule(sh, 2, 2, 0, true);
    for (Shape sh : {Shape{7, 8}, Shape{8, 7}, Shape{8, 8}}) rule(sh, 2, 8, 0, true);
    // k_avg's XCD rotation: batched ragged frames with every count of block rows modulo 8
    for (int h = 1082; h < 1098; h += 2) rule(Shape{1922, h}, 2, 2, 0, true, 0, 64);
    rule(Shape{1026, 514}, 2, 2, 0, true);                               // 257 edge pixels: two edge blocks
    for (int h : {124, 126})                                             // one row of edge blocks: 62 + 1 and 63 + 1 block rows
        for (int nf : {2, 64}) rule(Shape{1026, h}, 2, 2, 0, true, 0, nf);
    // the flat kernels' limits where only the pitch decides: 4-row frames around pitch x f = 2^24 and an output pitch of 2^24;
    // exactly 2^30 pixels of input (4096 x 1025 at a pitch of 2^20 - 4) and of output (8192 x 2050, f = 2), and one pitch step more
    for (int f : {1, 2, 8}) {
        rule(Shape{1000, 4}, 2, f, 0, false, 0, 1, (1 << 24) / f - 4, 1000);
        rule(Shape{1000, 4}, 2, f, 0, false, 0, 1, (1 << 24) / f, 1000);
        rule(Shape{1000, 4}, 2, f, 0, false, 0, 1, 1000, (1 << 24) - 4);
        rule(Shape{1000, 4}, 2, f, 0, false, 0, 1, 1000, 1 << 24);
    }
    rule(Shape{4096, 1025}, 2, 1, 0, false, 0, 1, (1 << 20) - 4, 4096);
    rule(Shape{4096, 1025}, 2, 1, 0, false, 0, 1, 1 << 20, 4096);
    rule(Shape{8192, 2050}, 2, 2, 0, false, 0, 1, 8192, (1 << 20) - 4);
    rule(Shape{8192, 2050}, 2, 2, 0, false, 0, 1, 8192, 1 << 20);
}

// One packed frame on each side of each limit of the flat kernels: 2^30 pixels, 2^24 rows, width x f at 2^24 (pitches: sweep_rules).
static void sweep_limits()
{
    for (int f : {1, 2, 8}) {
        for (Shape s : {Shape{32768, 32768}, Shape{32768, 32769}, Shape{8, (1 << 24) - 1}, Shape{8, 1 << 24}, Shape{(1 << 24) / f - 8, 4},
                        Shape{(1 << 24) / f, 4}})
            for (int o = 0; o < (f == 1 ? 1 : 2); ++o) emit(make(s, 2, f, o, false));
    }
}

// what plan_launch refuses
static void sweep_errors()
{
    Case c = make(Shape{512, 512}, 2, 2, 0, false);
    c.nframes = 0; emit(c);
    c.nframes = 65536; emit(c);
    c.nframes = 1; c.ip = 511; emit(c);
    c.ip = 0; c.op = 255; emit(c);
    c.op = 0; c.p.out_format = CSIC_FMT_PLANAR; emit(c);
    c.p.out_format = CSIC_FMT_PLANAR_BITS; emit(c);
}

// ---- the plane units: planar and bit-plane forward, reconstruct, decode ------------------------------------------------
// The plane format travels in p.out_format: what the forward units write, what reconstruct and decode read (decode also reads
// the packed formats); `to` is the packed format those two write.
enum Unit { U_PLANAR, U_BITS, U_RECON, U_DECODE };
static const char *const UNIT_WORD[] = {"planar", "bits", "recon", "decode"};

#define REQUIRE_COVER(blocks, per_block, work) REQUIRE((uint64_t)(blocks) * (uint64_t)(per_block) >= (uint64_t)(work))

static void emit_plane(Unit u, const Case &c, int to = CSIC_FMT_ARGB8888)
{
    Geometry g;
    char head[256], name[96] = "", hash[16] = "";
    case_head(c, &g, head, sizeof head);
    ++g_cases;
    const csic_params &p = c.p;
    csic_planar_layout L;
    planar_layout(g, &p, &L);
    const int64_t n = (int64_t)g.Wo * g.Ho, out_px = (int64_t)g.W * g.H;
    const bool flat_src = p.out_format == CSIC_FMT_PLANAR || p.out_format == CSIC_FMT_PLANAR_BITS;
    PlaneLaunch l{};
    int status = CSIC_OK, kind = 0;
    bool ok = true, rows = false, tile = false;                // a row-tiled kind; k_avg's launch
    switch (u) {
    case U_PLANAR: {
        PlanarPlan pp;
        if ((status = plan_planar(p, g, c.t, c.align, c.nframes, &pp)) != CSIC_OK) break;
        l = pp; kind = pp.kind;
        planar_kernel_name(pp.kind, p, g, c.t, name, sizeof name);
        REQUIRE(pp.args.bdx == l.bdx && pp.args.bdy == l.bdy && pp.args.row_step == l.row_step);
        REQUIRE(l.bdx == (int32_t)l.block.x && l.bdy == (int32_t)l.block.y);
        if (pp.kind == PLANAR_AVG_TILE) {
            // k_avg's launch: everything check_invariants asks of FAM_AVG
            tile = true;
            LaunchPlan lp{};
            lp.id.fam = FAM_AVG; lp.id.tiles = g.f <= 2 ? 2 : 1;
            lp.grid = l.grid; lp.block = l.block; lp.args = pp.args;
            ok = check_invariants(c, g, lp) && ok;
            REQUIRE(l.T == 256);
            std::snprintf(hash, sizeof hash, " h=%08x", args_hash(pp.args));
        } else if (pp.kind == PLANAR_AVG_F1 || pp.kind == PLANAR_AVG_GEN) {
            rows = true;
            REQUIRE(l.T == 256 && l.block.x * l.block.y <= 256);
            REQUIRE_COVER(l.grid.x, l.block.x * (pp.kind == PLANAR_AVG_F1 ? 2 : 1), pp.kind == PLANAR_AVG_F1 ? g.W / 4 : g.Wo);
            if (pp.kind == PLANAR_AVG_F1) REQUIRE(g.f == 1 && g.W % 4 == 0 && g.H % g.v == 0);
        } else {
            REQUIRE_COVER(l.grid.x, (uint64_t)l.T * 4 * (pp.kind == PLANAR_STRIDED ? 1 : PLANAR_K), n);
            if (pp.kind != PLANAR_FLAT_GEN) REQUIRE(L.module_width % 4 == 0);
        }
        break;
    }
    case U_BITS: {
        BitsPlan bp;
        if ((status = plan_planar_bits(p, g, c.t, c.align, c.nframes, &bp)) != CSIC_OK) break;
        l = bp; kind = bp.kind;
        planar_bits_kernel_name(bp.kind, p, g, c.t, name, sizeof name);
        REQUIRE(l.bdx == (int32_t)l.block.x && l.bdy == 1 && l.row_step == 1);
        if (bp.kind == PBITS_F1) { REQUIRE((c.align & 15u) == 0 && L.module_width % 128 == 0 && g.f == 1); REQUIRE_COVER(l.grid.x, l.T * PBITS_K, n / 4); }
        else if (bp.kind == PBITS_STRIDED) { REQUIRE(L.module_width % 128 == 0 && !g.s_first); REQUIRE_COVER(l.grid.x, l.T * 4, n); }
        else REQUIRE_COVER(l.grid.x, l.T, (n + 7) / 8 + (L.chroma_samples + 7) / 8);
        break;
    }
    case U_RECON: {
        ReconPlan rp;
        const int K = p.out_format == CSIC_FMT_PLANAR_BITS ? RBITS_K : RECON_K;
        if ((status = plan_reconstruct(g, c.t, L.module_width, K, c.nframes, &rp)) != CSIC_OK) break;
        l = rp; kind = rp.fast;
        reconstruct_kernel_name(p.out_format, to, rp.fast, c.t, name, sizeof name);
        if (rp.fast) REQUIRE(L.module_width % 4 == 0);
        REQUIRE_COVER(l.grid.x, (uint64_t)l.T * K * 4, n);
        break;
    }
    case U_DECODE: {
        DecodePlan dp;
        if ((status = plan_decode(p, g, c.t, p.out_format, c.align, c.nframes, &dp)) != CSIC_OK) break;
        l = dp; kind = dp.kind;
        decode_kernel_name(dp, g, c.t, p.out_format, to, name, sizeof name);
        if (dp.kind == DEC_FAST) {
            REQUIRE((c.align & 15u) == 0 && g.W % 4 == 0 && out_px <= (1ll << 30));
            REQUIRE_COVER(l.grid.x, l.T * dec_pieces_per_lane(g.f), (int64_t)(g.W / 4) * g.Ho);
        } else if (dp.kind == DEC_RECON) {
            REQUIRE(g.f == 1 && flat_src && (c.nframes == 1 || out_px % 4 == 0) && (c.align & 15u) == 0);
            REQUIRE_COVER(l.grid.x, (uint64_t)l.T * (p.out_format == CSIC_FMT_PLANAR_BITS ? RBITS_K : RECON_K) * 4, n);
        } else {
            REQUIRE_COVER(l.grid.x, l.T, out_px);
        }
        break;
    }
    }
    if (status != CSIC_OK) {
        if (g_print) std::printf("%s %s -> %d\n", UNIT_WORD[u], head, status);
        return;
    }
    // every plane launch, whatever the rules are
    REQUIRE(l.T == 64 || l.T == 128 || l.T == 256);
    // (reconstruct and decode are planned once per call: z is the first batch's)
    const int nz = (u == U_RECON || u == U_DECODE) && c.nframes > 65535 ? 65535 : c.nframes;
    REQUIRE(l.grid.x >= 1 && l.grid.y >= 1 && l.grid.y <= 65535 && l.grid.z == (uint32_t)nz && l.block.z == 1);
    if (rows) REQUIRE(l.row_step == (int32_t)(l.grid.y * l.block.y));
    else if (!tile) REQUIRE(l.block.x * l.block.y == (uint32_t)l.T && l.grid.y == 1 && l.block.y == 1);
    if (u == U_RECON || u == U_DECODE) REQUIRE(l.bdx == 0 && l.bdy == 0 && l.row_step == 0);
    if (!ok) { std::fprintf(stderr, "  in: %s %s -> %s\n", UNIT_WORD[u], head, name); ++g_failed; }
    if (!g_print) return;
    std::printf("%s %s", UNIT_WORD[u], head);
    if (u == U_RECON || u == U_DECODE) std::printf(" to-%s", format_word(to));
    std::printf(" -> 0 %s g=%u,%u,%u b=%u,%u,%u a=%d,%d,%d T=%d%s", name, l.grid.x, l.grid.y, l.grid.z, l.block.x, l.block.y, l.block.z, l.bdx,
                l.bdy, l.row_step, l.T, hash);
    if (g_fields) std::printf(" k%d", kind);
    std::printf("\n");
}

static Case plane_case(Shape s, int ch, int f, int order, bool avg, int fmt, int tune = -1, int nframes = 1, unsigned align = 0)
{
    Case c = make(s, ch, f, order, avg);
    c.p.out_format = fmt;
    if (tune >= 0) c.t = tune_set(tune);
    c.nframes = nframes; c.align = align;
    return c;
}

// One case on each side of every comparison of the plane units' rules, on the smallest shapes that flip it (nothing is allocated).
// 64x40: every module width a multiple of 4; 201x27: none, and W H no multiple of 4; 66x40: W % 4 != 0 with an even output width.
static void sweep_planes()
{
    const int PL = CSIC_FMT_PLANAR, PB = CSIC_FMT_PLANAR_BITS;
    const Shape A{64, 40}, B{201, 27}, C{66, 40};
    // planar forward.  HOLD: module width % 4, factor 1 with W % 4, factors >= 2 in both order classes
    for (Shape s : {A, B, C})
        for (int f : {1, 2, 4})
            for (int o = 0; o < (f == 1 ? 1 : 2); ++o) emit_plane(U_PLANAR, plane_case(s, 2, f, o, false, PL));
    for (int ch : {0, 3}) emit_plane(U_PLANAR, plane_case(A, ch, 2, 0, false, PL));          // the other holds
    // the group count at a block's edge: 1024 groups and one position (4 blocks of 256 threads and 1), 1024 groups in 4 one-wave blocks
    for (Shape s : {Shape{4097, 1}, Shape{64, 64}}) emit_plane(U_PLANAR, plane_case(s, 2, 1, 0, false, PL));
    // AVG: whole tiles, H % v != 0, no whole tile; every factor
    for (Shape s : {A, Shape{64, 41}, Shape{3, 5}})
        for (int f : FACTORS) emit_plane(U_PLANAR, plane_case(s, 2, f, 0, true, PL));
    // the variants (9 general, 10 four positions per lane, 12 the tile body at factor 1), cached accesses, block threads
    for (int k : {9, 10, 12, 15, 16, 17, 18})
        for (int f : {1, 2})
            for (int avg = 0; avg < 2; ++avg) emit_plane(U_PLANAR, plane_case(A, 2, f, 0, avg != 0, PL, k));
    { Case c = plane_case(A, 2, 1, 0, true, PL, 12); c.t.no_nt = 1; emit_plane(U_PLANAR, c); }    // variant 12 AND cached: avg_f1 again
    // batches (k_avg's XCD rotation needs more than one frame); the table path's 4-byte-aligned frames: the same kernels as aligned
    // ones, 16-byte loads included -- the packed path drops to 4-byte kernels there
    for (int nf : {3, 65535})
        for (int avg = 0; avg < 2; ++avg)
            for (int f : {1, 2}) emit_plane(U_PLANAR, plane_case(Shape{1922, 1082}, 2, f, 0, avg != 0, PL, -1, nf));
    for (int avg = 0; avg < 2; ++avg) emit_plane(U_PLANAR, plane_case(A, 2, 1, 0, avg != 0, PL, -1, 3, 4));
    // the row-tiled kernels: block width around 256 lanes (avg_f1: 2 tiles of 4 pixels per lane; avg_gen, variant 9: a pixel), and
    // the grid-y clamp at 65535 block rows, on both sides
    for (int w : {2040, 2048, 2052, 2056}) emit_plane(U_PLANAR, plane_case(Shape{w, 8}, 2, 1, 0, true, PL));
    for (int w : {255, 256, 257}) emit_plane(U_PLANAR, plane_case(Shape{w, 8}, 2, 1, 0, true, PL, 9));
    for (int h : {65534, 65535, 65536, 70000}) {
        emit_plane(U_PLANAR, plane_case(Shape{2048, 2 * h}, 2, 1, 0, true, PL));
        emit_plane(U_PLANAR, plane_case(Shape{256, h}, 2, 1, 0, true, PL, 9));
    }
    // bit-plane forward: module width % 128 (chroma first at factor 2: the output width), factor 1, factor 2 in both order classes,
    // factor 4, AVG, variant 9, a 4-byte-aligned input, block threads, a batch
    for (Shape s : {Shape{128, 8}, Shape{132, 8}, Shape{256, 8}, Shape{264, 8}}) {
        for (int f : {1, 2, 4})
            for (int o = 0; o < (f == 1 ? 1 : 2); ++o) emit_plane(U_BITS, plane_case(s, 2, f, o, false, PB));
        emit_plane(U_BITS, plane_case(s, 2, 1, 0, true, PB));
    }
    for (int f : {1, 2}) {
        for (int k : {9, 15, 16, 17, 18}) emit_plane(U_BITS, plane_case(Shape{256, 8}, 2, f, 0, false, PB, k));
        emit_plane(U_BITS, plane_case(Shape{256, 8}, 2, f, 0, false, PB, -1, 1, 4));
        emit_plane(U_BITS, plane_case(Shape{256, 8}, 2, f, 0, false, PB, -1, 3));
        emit_plane(U_BITS, plane_case(Shape{256, 40}, 2, f, 0, false, PB));                 // several blocks of either fast kernel
    }
    // k_pbits_gen's groups of 8 samples at 4:4:4 (as many chroma samples as positions): exactly one block of them, and 2 more
    for (int w : {128, 129}) emit_plane(U_BITS, plane_case(Shape{w, 8}, 0, 1, 0, true, PB));
    // reconstruct, both sources and both outputs: module width % 4, variant 9, cached accesses, block threads, a batch
    for (int src : {PL, PB})
        for (int to : {(int)CSIC_FMT_ARGB8888, (int)CSIC_FMT_YCBCR888X}) {
            for (Shape s : {A, B, C})
                for (int f : {1, 2})
                    for (int o = 0; o < (f == 1 ? 1 : 2); ++o) emit_plane(U_RECON, plane_case(s, 2, f, o, false, src), to);
            for (int k : {9, 15, 16, 17, 18}) emit_plane(U_RECON, plane_case(A, 2, 2, 0, false, src, k), to);
            emit_plane(U_RECON, plane_case(B, 2, 1, 0, false, src, -1, 3), to);
        }
    // 1024 groups and one position; calls of more than 65535 frames go in batches: z is the first one's
    emit_plane(U_RECON, plane_case(Shape{4097, 1}, 2, 1, 0, false, PL));
    for (int nf : {65534, 65536}) {
        emit_plane(U_RECON, plane_case(A, 2, 1, 0, false, PL, -1, nf));
        emit_plane(U_DECODE, plane_case(A, 2, 2, 0, false, PL, -1, nf));
    }
    // decode from the three sources (and once from ARGB): every clause of the kind both ways -- variant 9, force-generic, no-vector,
    // 4-byte-aligned pointers; factor 1 from planes (reconstruct) against packed; W H % 4 with 1 and 3 frames; W % 4; factors 1 - 8;
    // W H on both sides of 2^30; block threads
    for (int src : {(int)CSIC_FMT_YCBCR888X, PL, PB}) {
        for (Shape s : {A, B, C, Shape{64, 41}})
            for (int f : FACTORS)
                for (int nf : {1, 3}) emit_plane(U_DECODE, plane_case(s, 2, f, 0, false, src, -1, nf));
        for (int f : {1, 2}) {
            for (int k : {9, 13, 14, 15, 16, 17, 18}) emit_plane(U_DECODE, plane_case(A, 2, f, 0, false, src, k));
            emit_plane(U_DECODE, plane_case(A, 2, f, 0, false, src, -1, 1, 4));
            emit_plane(U_DECODE, plane_case(A, 2, f, 1, false, src), CSIC_FMT_YCBCR888X);
            for (Shape s : {Shape{32768, 32768}, Shape{32768, 32769}}) emit_plane(U_DECODE, plane_case(s, 2, f, 0, false, src));
        }
    }
    emit_plane(U_DECODE, plane_case(A, 2, 2, 0, false, CSIC_FMT_ARGB8888));
}

// the whole cross product for the plane units: every knob setting, then batches and 4-byte-aligned pointers
static void sweep_planes_full()
{
    for (int s = 0; s < NSHAPES; ++s)
        for (int ch = 0; ch < 6; ++ch)
            for (int f : FACTORS)
                for (int o = 0; o < 7; ++o)
                    for (int fmt : {(int)CSIC_FMT_YCBCR888X, (int)CSIC_FMT_PLANAR, (int)CSIC_FMT_PLANAR_BITS}) {
                        const auto each = [&](Unit u, int to) {
                            for (int k = 0; k < NTUNES; ++k) emit_plane(u, plane_case(SHAPES[s], ch, f, o % 6, o == 6, fmt, k), to);
                            for (int nf : {1, 3, 65535})
                                for (unsigned al : {0u, 4u})
                                    if (nf != 1 || al) emit_plane(u, plane_case(SHAPES[s], ch, f, o % 6, o == 6, fmt, -1, nf, al), to);
                        };
                        for (int to : {(int)CSIC_FMT_ARGB8888, (int)CSIC_FMT_YCBCR888X}) each(U_DECODE, to);
                        if (fmt == CSIC_FMT_YCBCR888X) continue;
                        each(fmt == CSIC_FMT_PLANAR ? U_PLANAR : U_BITS, 0);
                        each(U_RECON, CSIC_FMT_ARGB8888);
                    }
}

int main(int argc, char **argv)
{
    bool full = false;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--full")) full = g_fields = true;
        else if (!std::strcmp(argv[i], "--check")) { full = true; g_print = false; }
        else { std::fprintf(stderr, "usage: launch_table [--full | --check]\n"); return 2; }
    }
    if (full) sweep_full(); else sweep_committed();
    sweep_rules();
    sweep_limits();
    sweep_errors();
    for (const std::string &line : g_measure) std::printf("%s\n", line.c_str());
    if (full) sweep_planes_full();
    sweep_planes();
    std::fprintf(stderr, "launch_table: %ld cases, %ld with a broken invariant\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
