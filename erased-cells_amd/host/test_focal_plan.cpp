// test_focal_plan.cpp — csrc/ec_focal_plan.hpp alone, under a plain C++ compiler: the refusals of ec_focal / ec_focal_convolve, the tile
// grid, the part of the raster a workgroup stages and the LDS layout of that stage — the very functions the library's host side and
// its kernels run.  Built a second time with the address and undefined-behaviour sanitizers (test_focal_plan_san).  Needs no device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ec_focal_plan.hpp"

static int g_checks = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) {                                                                 \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

using namespace ecf;

// every cell of the raster is the output of exactly one tile; every footprint cell inside the raster is staged by that tile, and
// nothing outside the raster is: counted in a map of the raster
static void cover(uint64_t cols, uint64_t rows, uint32_t rx, uint32_t ry, uint32_t tw, uint32_t th) {
    Grid g;
    int src, dst;
    CHECK(refusal(false, 0, &src, &dst, nullptr, nullptr, nullptr, cols, rows, rx, ry, 0, tw, th, &g) == nullptr);
    CHECK(g.tiles == g.tiles_x * g.tiles_y && g.tiles_x == ceil_div(cols, tw) && g.tiles_y == ceil_div(rows, th));
    std::vector<int> owner(cols * rows, 0);
    for (uint64_t ty = 0; ty < g.tiles_y; ++ty) {
        for (uint64_t tx = 0; tx < g.tiles_x; ++tx) {
            const Tile t = tile_at(cols, rows, rx, ry, tx, ty, tw, th);
            CHECK(t.ow >= 1 && t.ow <= tw && t.oh >= 1 && t.oh <= th);
            CHECK(t.x0 + t.ow <= cols && t.y0 + t.oh <= rows);
            CHECK(t.xs + t.sw <= cols && t.ys + t.sh <= rows);               // nothing outside the raster is staged
            CHECK(t.sw <= tw + 2 * rx && t.sh <= th + 2 * ry);               // ... and the stage fits its LDS rows
            CHECK(t.xs == (t.x0 < rx ? 0 : t.x0 - rx) && t.ys == (t.y0 < ry ? 0 : t.y0 - ry));
            for (uint32_t oy = 0; oy < t.oh; ++oy) {
                for (uint32_t ox = 0; ox < t.ow; ++ox) {
                    ++owner[(t.y0 + oy) * cols + t.x0 + ox];
                    // the kernels' clip: a footprint cell is inside the raster iff its staged coordinates are inside the stage
                    for (int64_t dy = -int64_t(ry); dy <= int64_t(ry); ++dy) {
                        for (int64_t dx = -int64_t(rx); dx <= int64_t(rx); ++dx) {
                            const int64_t y = int64_t(t.y0 + oy) + dy, x = int64_t(t.x0 + ox) + dx;
                            const bool inside = y >= 0 && y < int64_t(rows) && x >= 0 && x < int64_t(cols);
                            const int32_t ly = int32_t(t.y0 - t.ys) - int32_t(ry) + int32_t(oy) + int32_t(dy + ry);
                            const int32_t lx = int32_t(t.x0 - t.xs) - int32_t(rx) + int32_t(ox) + int32_t(dx + rx);
                            CHECK((uint32_t(ly) < t.sh && uint32_t(lx) < t.sw) == inside);
                            if (inside) CHECK(t.ys + uint32_t(ly) == uint64_t(y) && t.xs + uint32_t(lx) == uint64_t(x));
                        }
                    }
                }
            }
        }
    }
    for (int k : owner) CHECK(k == 1);
}

int main() {
    const uint32_t sizes[][2] = {{64, 16}, {8, 4}, {5, 3}};
    for (const auto& s : sizes) {
        const uint32_t tw = s[0], th = s[1];
        const uint32_t radii[][2] = {{0, 0}, {1, 1}, {2, 1}, {1, 3}, {7, 7}, {7, 0}, {0, 7}};
        for (const auto& r : radii) {
            const uint64_t cs[] = {1, 2, r[0] + 1, 2 * r[0] + 1, tw - 1, tw, tw + 1, 2 * tw + 1};
            const uint64_t rs[] = {1, 2, r[1] + 1, 2 * r[1] + 1, th - 1, th, th + 1, 2 * th + 1};
            for (uint64_t c : cs)
                for (uint64_t rr : rs) cover(c, rr, r[0], r[1], tw, th);
        }
    }
    {  // the layout: every offset and pitch a multiple of 16, parts in order and disjoint, the largest well inside 64 KiB
        uint32_t largest = 0;
        for (uint32_t cell : {1u, 2u, 4u, 8u})
            for (int masked = 0; masked < 2; ++masked)
                for (int kind = 0; kind < 3; ++kind)
                    for (uint32_t rx = 0; rx <= kRadiusCap; ++rx)
                        for (uint32_t ry = 0; ry <= kRadiusCap; ++ry) {
                            const Layout l = layout_of(cell, masked != 0, kind, rx, ry, 64, 16);
                            const uint32_t hr = 16 + 2 * ry;
                            CHECK(l.cell_pitch % 16 == 0 && l.mask_pitch % 16 == 0 && l.off_mask % 16 == 0 && l.off_racc % 16 == 0 && l.off_rcnt % 16 == 0 && l.bytes % 16 == 0);
                            CHECK(l.cell_pitch >= (64 + 2 * rx) * cell && l.mask_pitch >= 64 + 2 * rx);
                            CHECK(l.off_mask == hr * l.cell_pitch);
                            CHECK(l.off_racc == l.off_mask + (masked ? hr * l.mask_pitch : 0));
                            CHECK(l.off_rcnt == l.off_racc + (kind == kConvolve ? 0 : hr * 64 * (kind == kSeparableMinMax ? cell : 8)));
                            CHECK(l.bytes >= l.off_rcnt + (kind == kConvolve || !masked ? 0 : hr * 64));
                            CHECK((64 * (kind == kSeparableMinMax ? cell : 8)) % 16 == 0);   // a row of row results keeps the slots aligned
                            if (l.bytes > largest) largest = l.bytes;
                        }
        CHECK(largest == 38400 && largest < 40 * 1024);
    }
    {  // the refusals, in the order the header lists them; pointers are only compared
        Grid g;
        int a, b, m, n;
        double w[9] = {0};
        const uint64_t big = uint64_t(1) << 40;
        CHECK(refusal(false, 0, nullptr, &b, nullptr, nullptr, nullptr, 4, 4, 1, 1, 0, 64, 16, &g));
        CHECK(refusal(false, 0, &a, nullptr, nullptr, nullptr, nullptr, 4, 4, 1, 1, 0, 64, 16, &g));
        CHECK(refusal(true, 0, &a, &b, nullptr, nullptr, nullptr, 4, 4, 1, 1, 0, 64, 16, &g));
        CHECK(!refusal(true, 99, &a, &b, w, nullptr, nullptr, 4, 4, 1, 1, 0, 64, 16, &g));   // a convolution has no op
        CHECK(refusal(false, 4, &a, &b, nullptr, nullptr, nullptr, 4, 4, 1, 1, 0, 64, 16, &g));
        CHECK(refusal(false, -1, &a, &b, nullptr, nullptr, nullptr, 4, 4, 1, 1, 0, 64, 16, &g));
        CHECK(refusal(false, 0, &a, &b, nullptr, nullptr, nullptr, 4, 4, 1, 1, 4, 64, 16, &g));
        CHECK(refusal(false, 0, &a, &b, nullptr, nullptr, nullptr, 4, 4, 1, 1, kFlagNormalize, 64, 16, &g));
        CHECK(!refusal(true, 0, &a, &b, w, nullptr, nullptr, 4, 4, 1, 1, kFlagNormalize, 64, 16, &g));
        CHECK(refusal(false, 0, &a, &b, nullptr, nullptr, nullptr, 4, 4, 8, 1, 0, 64, 16, &g));
        CHECK(refusal(false, 0, &a, &b, nullptr, nullptr, nullptr, 4, 4, 1, 0xffffffffu, 0, 64, 16, &g));
        CHECK(!refusal(false, 0, &a, &b, nullptr, nullptr, nullptr, 4, 4, 7, 7, 0, 64, 16, &g));
        CHECK(refusal(false, 0, &a, &b, nullptr, &m, nullptr, 4, 4, 1, 1, 0, 64, 16, &g));
        CHECK(refusal(false, 0, &a, &b, nullptr, nullptr, nullptr, 4, 4, 1, 1, kFlagWhole, 64, 16, &g));
        CHECK(!refusal(false, 0, &a, &b, nullptr, &m, &n, 4, 4, 1, 1, kFlagWhole, 64, 16, &g));
        CHECK(!refusal(false, 0, &a, &b, nullptr, nullptr, &n, 4, 4, 1, 1, 0, 64, 16, &g));
        CHECK(refusal(false, 0, &a, &b, nullptr, nullptr, nullptr, big, big, 1, 1, 0, 64, 16, &g));
        CHECK(refusal(false, 0, &a, &b, nullptr, nullptr, nullptr, UINT64_MAX, 2, 1, 1, 0, 64, 16, &g));
        CHECK(!refusal(false, 0, &a, &b, nullptr, nullptr, nullptr, UINT64_MAX, 0, 1, 1, 0, 64, 16, &g) && g.tiles == 0);
        CHECK(!refusal(false, 0, &a, &b, nullptr, nullptr, nullptr, 0, UINT64_MAX, 1, 1, 0, 64, 16, &g) && g.tiles == 0);
        CHECK(refusal(false, 0, &a, &a, nullptr, nullptr, nullptr, 4, 4, 1, 1, 0, 64, 16, &g));
        CHECK(refusal(false, 0, &a, &b, nullptr, &m, &m, 4, 4, 1, 1, 0, 64, 16, &g));
        // tiles: 2^31 - 1 pass, 2^31 do not, and the count never overflows on the way
        CHECK(!refusal(false, 0, &a, &b, nullptr, nullptr, nullptr, 1, 16 * kMaxTiles, 1, 1, 0, 64, 16, &g) && g.tiles == kMaxTiles);
        CHECK(refusal(false, 0, &a, &b, nullptr, nullptr, nullptr, 1, 16 * kMaxTiles + 1, 1, 1, 0, 64, 16, &g));
        CHECK(refusal(false, 0, &a, &b, nullptr, nullptr, nullptr, uint64_t(64) << 31, 1, 1, 1, 0, 64, 16, &g));
        CHECK(refusal(false, 0, &a, &b, nullptr, nullptr, nullptr, uint64_t(1) << 62, 2, 1, 1, 0, 64, 16, &g));
        CHECK(!refusal(false, 0, &a, &b, nullptr, nullptr, nullptr, 64 * 46340, 16 * 46340, 1, 1, 0, 64, 16, &g) && g.tiles == uint64_t(46340) * 46340);
        CHECK(refusal(false, 0, &a, &b, nullptr, nullptr, nullptr, 64 * 46341, 16 * 46341, 1, 1, 0, 64, 16, &g));
    }
    std::printf("%d checks passed\n", g_checks);
    return 0;
}
