// view_plan.cpp -- plan_view and check_view of csic_select.cpp without a GPU: over the cross product of scale, factor, output
// alignment, view widths 1 .. 9, origins and the tuning knobs, the program asserts
//   - grid x block covers every unit, and the lanes' units (k_view: 4 consecutive output pixels of a row, k_view_gen: one) cover every
//     output pixel exactly once -- the kernels' own index arithmetic, replayed here over the planned launch;
//   - the fast kernel is chosen exactly under its conditions (width % 4 == 0, a 16-byte aligned output, no knob for the general one);
//   - ncx / ncy are what a box can touch at most, and are reached, by brute force over the boxes of the view;
//   - check_view refuses exactly the views that leave the frame, in 64-bit arithmetic, and the scales outside the set.
// Prints "view plan ok: N launches" and exits 0, or names the first failed check and exits 1.  g++ -std=c++17, host only: links
// csic_select.cpp and csic_host.cpp.
#include <cstdio>
#include <cstring>
#include <vector>

#include "csic.h"
#include "csic_select.h"

using namespace csic;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures++ < 10) std::printf("FAILED: %s (line %d) %s\n", #c, __LINE__, ctx); } } while (0)

static char ctx[160];

static int cells_touched(int b, int s, int f) { return (b + s - 1) / f - b / f + 1; }

int main()
{
    long launches = 0;
    std::strcpy(ctx, "");
    const int W = 200, H = 150;
    for (int f : {1, 2, 4, 8}) {
        csic_params p;
        csic_params_default(&p, W, H);
        p.chroma_a = 2; p.chroma_b = 0; p.y_bits = 6; p.cb_bits = 5; p.cr_bits = 5; p.factor = f;
        Geometry g;
        if (derive_geometry(&p, &g) != CSIC_OK) { std::printf("bad case: %s\n", csic_last_error()); return 2; }
        for (int s : {1, 2, 4, 8, 16})
            for (unsigned align : {0u, 4u, 8u, 16u})
                for (int vw = 1; vw <= 9; ++vw)
                    for (int vh : {1, 3})
                        for (int x0 : {0, 1, 3, 8})
                            for (int y0 : {0, 1, 4})
                                for (int knob = 0; knob < 7; ++knob) {
                                    Tune t{};
                                    if (knob == 1) t.variant = 9;
                                    if (knob == 2) t.force_generic = 1;
                                    if (knob == 3) t.no_vec = 1;
                                    if (knob == 4) t.no_nt = 1;
                                    if (knob == 5) t.block_threads = 128;
                                    if (knob == 6) t.block_threads = 256;
                                    const csic_view v{x0, y0, vw, vh, s};
                                    std::snprintf(ctx, sizeof ctx, "[f%d s%d align%u %dx%d at (%d,%d) knob%d]", f, s, align, vw, vh, x0, y0, knob);
                                    CHECK(check_view(g, v) == CSIC_OK);
                                    for (int nframes : {1, 3, 70000}) {
                                        ViewPlan vp;
                                        CHECK(plan_view(g, t, v, align, nframes, &vp) == CSIC_OK);
                                        ++launches;
                                        const bool general = knob >= 1 && knob <= 3;
                                        const bool fast = !general && vw % 4 == 0 && align % 16 == 0;
                                        CHECK((vp.kind == VIEW_FAST) == fast);
                                        CHECK((1 << vp.ls) == s);
                                        const int per = fast ? VIEW_PX : 1;
                                        CHECK(vp.units_per_row * per == vw && vp.units == (int64_t)vp.units_per_row * vh);
                                        CHECK(vp.block.y == 1 && vp.block.z == 1 && vp.grid.y == 1 && (int)vp.block.x == vp.T);
                                        CHECK(vp.T == (knob == 5 ? 128 : knob == 6 ? 256 : fast ? 64 : 256));
                                        CHECK(vp.grid.z == (uint32_t)(nframes < 65535 ? nframes : 65535));
                                        CHECK((int64_t)vp.grid.x * vp.T >= vp.units && (int64_t)(vp.grid.x - 1) * vp.T < vp.units);
                                        // the kernels' indexing over the planned launch: lane t -> row t / U, unit t % U
                                        std::vector<int> hit((size_t)vw * vh, 0);
                                        for (int64_t lane = 0; lane < (int64_t)vp.grid.x * vp.T; ++lane) {
                                            if (lane >= vp.units) continue;
                                            const int r = (int)(lane / vp.units_per_row), u = (int)(lane % vp.units_per_row);
                                            for (int k = 0; k < per; ++k) ++hit[(size_t)r * vw + (size_t)u * per + k];
                                        }
                                        bool once = true;
                                        for (int h : hit) once = once && h == 1;
                                        CHECK(once);
                                        int mx = 0, my = 0;
                                        for (int c = 0; c < vw; ++c) mx = cells_touched(x0 + c * s, s, f) > mx ? cells_touched(x0 + c * s, s, f) : mx;
                                        for (int r = 0; r < vh; ++r) my = cells_touched(y0 + r * s, s, f) > my ? cells_touched(y0 + r * s, s, f) : my;
                                        CHECK(vp.ncx >= mx && vp.ncy >= my && vp.ncx <= mx + 1 && vp.ncy <= my + 1);
                                        if (s >= f) CHECK(vp.ncx == mx && vp.ncy == my);
                                    }
                                }
        // refusals: one pixel outside on each side, nothing to show, scales outside the set, sums that only fit 64 bits
        std::snprintf(ctx, sizeof ctx, "[refusals f%d]", f);
        const csic_view inside{8, 6, 12, 9, 16};                               // 8 + 192 = 200, 6 + 144 = 150
        CHECK(check_view(g, inside) == CSIC_OK);
        const csic_view bad[] = {{9, 6, 12, 9, 16}, {8, 7, 12, 9, 16}, {-1, 6, 12, 9, 16}, {8, -1, 12, 9, 16}, {0, 0, 201, 1, 1}, {0, 0, 1, 151, 1},
                                 {0, 0, 0, 1, 1}, {0, 0, 1, 0, 1}, {0, 0, -1, 1, 1}, {0, 0, 1, 1, 3}, {0, 0, 1, 1, 0}, {0, 0, 1, 1, 32}, {0, 0, 1, 1, -2},
                                 {0, 0, 0x7FFFFFFF, 1, 16}, {0x7FFFFFFF, 0, 0x7FFFFFFF, 1, 16}, {0, 0x7FFFFFFF, 1, 0x7FFFFFFF, 2}, {0, 0, 0x10000000, 1, 16}};
        for (const csic_view &b : bad) {
            std::snprintf(ctx, sizeof ctx, "[refusal f%d %dx%d at (%d,%d) s%d]", f, b.width, b.height, b.x0, b.y0, b.scale);
            CHECK(check_view(g, b) == CSIC_EINVAL_SIZE);
        }
        // names
        ViewPlan vp;
        char name[96];
        Tune t{};
        plan_view(g, t, csic_view{0, 0, 8, 8, 8}, 0, 1, &vp);
        view_kernel_name(vp, t, CSIC_FMT_PLANAR_BITS, CSIC_FMT_ARGB8888, name, sizeof name);
        CHECK(std::strcmp(name, "k_view<s8,bits,argb,nt>") == 0);
        t.no_nt = 1;
        view_kernel_name(vp, t, CSIC_FMT_ARGB8888, CSIC_FMT_ARGB8888, name, sizeof name);
        CHECK(std::strcmp(name, "k_view<s8,ycc,ycc,cached>") == 0);
        plan_view(g, t, csic_view{0, 0, 7, 8, 2}, 0, 1, &vp);
        view_kernel_name(vp, t, CSIC_FMT_PLANAR, CSIC_FMT_YCBCR888X, name, sizeof name);
        CHECK(std::strcmp(name, "k_view_gen<planar,ycc>") == 0);
    }
    // a view of more than 2^30 pixels takes the general kernel (32-bit byte offsets in k_view)
    {
        Geometry g{};
        g.W = 46000; g.H = 46000; g.Wo = 46000; g.Ho = 46000; g.f = 1;
        ViewPlan vp;
        Tune t{};
        std::strcpy(ctx, "[2^30]");
        plan_view(g, t, csic_view{0, 0, 40000, 30000, 1}, 0, 1, &vp);
        CHECK(vp.kind == VIEW_GEN);
        plan_view(g, t, csic_view{0, 0, 32768, 32768, 1}, 0, 1, &vp);
        CHECK(vp.kind == VIEW_FAST && vp.units == (int64_t)1 << 28);
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("view plan ok: %ld launches\n", launches);
    return 0;
}
