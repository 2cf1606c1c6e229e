// ec_focal_plan.hpp — the arithmetic that the host side and the kernels of ec_focal / ec_focal_convolve (include/erased_cells.h) share:
// the refusals, the tile grid, the part of the raster a workgroup stages (its output tile and the halo, clipped at the raster's edges)
// and the LDS layout of that stage — and, for ec_focal_rank / ec_focal_majority, which stage the same way, their refusals (rank_refusal) and their
// layout (rank_layout_of) at the end of the file.
//
// Self-contained: no HIP include; under a plain C++ compiler the function attributes are defined away (as ec_order_key.hpp does), so
// host/test_focal_plan.cpp runs these very functions under the address and undefined-behaviour sanitizers.
//
// The tile is tw x th output cells (TW, TH of ec_focal_kernels.hpp; parameters here so that the stand-alone program can try others).
// A workgroup stages the raster cells [xs, xs + sw) x [ys, ys + sh): columns x0 - rx .. x0 + ow - 1 + rx and rows y0 - ry ..
// y0 + oh - 1 + ry cut to the raster.  Staged cell (ly, lx) is raster cell (ys + ly, xs + lx); a cell of a footprint is inside the
// raster exactly when its staged coordinates are inside [0, sh) x [0, sw), which is how the kernels clip.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EC_FOCAL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define EC_FOCAL_HD inline
#endif

namespace ecf {

constexpr uint32_t kRadiusCap = 7;              // EC_FOCAL_RADIUS_CAP
constexpr uint32_t kFlagWhole = 1, kFlagNormalize = 2;
constexpr uint64_t kMaxTiles = 0x7fffffffull;   // one workgroup per tile, a grid of at most 2^31 - 1
enum Kind { kSeparableSum = 0, kSeparableMinMax = 1, kConvolve = 2 };

struct Tile {
    uint64_t x0, y0;  // first output cell
    uint32_t ow, oh;  // output cells of the tile that exist
    uint64_t xs, ys;  // first staged cell
    uint32_t sw, sh;  // staged cells
};

EC_FOCAL_HD uint64_t ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b != 0); }

// tile (tx, ty) of a cols x rows raster, tx < ceil(cols / tw), ty < ceil(rows / th)
EC_FOCAL_HD Tile tile_at(uint64_t cols, uint64_t rows, uint32_t rx, uint32_t ry, uint64_t tx, uint64_t ty, uint32_t tw, uint32_t th) {
    Tile t;
    t.x0 = tx * tw;
    t.y0 = ty * th;
    t.ow = cols - t.x0 < tw ? uint32_t(cols - t.x0) : tw;
    t.oh = rows - t.y0 < th ? uint32_t(rows - t.y0) : th;
    t.xs = t.x0 < rx ? 0 : t.x0 - rx;
    t.ys = t.y0 < ry ? 0 : t.y0 - ry;
    const uint64_t right = cols - (t.x0 + t.ow), below = rows - (t.y0 + t.oh);  // cells of the raster behind the tile
    const uint64_t xe = t.x0 + t.ow + (right < rx ? right : rx), ye = t.y0 + t.oh + (below < ry ? below : ry);
    t.sw = uint32_t(xe - t.xs);
    t.sh = uint32_t(ye - t.ys);
    return t;
}

// The stage of one workgroup, in bytes from the start of its LDS, every offset and pitch a multiple of 16:
//   cells   (th + 2 ry) rows of cell_pitch bytes: (tw + 2 rx) cells of `cell` bytes
//   mask    (th + 2 ry) rows of mask_pitch bytes, masked launches only
//   racc    (th + 2 ry) rows of tw row results: a sum as f64 (8 bytes), a minimum or maximum as an order key of `cell` bytes — not for a
//           convolution
//   rcnt    (th + 2 ry) rows of tw row tap counts, one byte each (at most 15) — masked sums and extremes only: without a mask the count
//           of a row is what the clip leaves
struct Layout {
    uint32_t cell_pitch, mask_pitch;
    uint32_t off_mask, off_racc, off_rcnt;
    uint32_t bytes;
};

EC_FOCAL_HD uint32_t round16(uint32_t b) { return (b + 15u) & ~15u; }

EC_FOCAL_HD Layout layout_of(uint32_t cell, bool masked, int kind, uint32_t rx, uint32_t ry, uint32_t tw, uint32_t th) {
    Layout l;
    const uint32_t hr = th + 2 * ry;
    l.cell_pitch = round16((tw + 2 * rx) * cell);
    l.mask_pitch = round16(tw + 2 * rx);
    l.off_mask = hr * l.cell_pitch;
    l.off_racc = l.off_mask + (masked ? hr * l.mask_pitch : 0u);
    l.off_rcnt = l.off_racc + (kind == kConvolve ? 0u : hr * tw * (kind == kSeparableMinMax ? cell : 8u));
    l.bytes = l.off_rcnt + (kind == kConvolve || !masked ? 0u : round16(hr * tw));
    return l;
}

struct Grid {
    uint64_t tiles_x, tiles_y, tiles;
};

// The refusals every moving window ends on, behind its own: the output mask, the raster's size, the not-in-place rules and the tile
// grid.  Fills *g (zeroes before) for a call that passes; an empty raster passes with g->tiles == 0.
inline const char* raster_refusal(const void* src, const void* dst, const void* src_mask, const void* dst_mask, uint64_t cols, uint64_t rows,
                                  uint32_t flags, uint32_t tw, uint32_t th, Grid* g) {
    if (!dst_mask && (src_mask || (flags & kFlagWhole))) return "dst_mask is NULL where cells can be invalid (a source mask, or EC_FOCAL_WHOLE)";
    if (cols != 0 && rows > UINT64_MAX / cols) return "cols * rows overflows 64 bits";
    if (dst == src) return "dst == src: the operation is not in-place";
    if (dst_mask && dst_mask == src_mask) return "dst_mask == src_mask: the operation is not in-place";
    if (cols == 0 || rows == 0) return nullptr;
    g->tiles_x = ceil_div(cols, tw);
    g->tiles_y = ceil_div(rows, th);
    if (g->tiles_y > kMaxTiles / g->tiles_x) return "more than 2^31 - 1 tiles";  // tiles_x >= 1; no overflow: the product is never formed
    g->tiles = g->tiles_x * g->tiles_y;
    return nullptr;
}

// Why a call is refused (EC_ERR_ARG), or null; fills *g for a call that is not.  `op` is looked at for ec_focal (convolve false),
// `weights` for ec_focal_convolve.  An empty raster passes with g->tiles == 0.
inline const char* refusal(bool convolve, int32_t op, const void* src, const void* dst, const void* weights, const void* src_mask,
                           const void* dst_mask, uint64_t cols, uint64_t rows, uint32_t rx, uint32_t ry, uint32_t flags, uint32_t tw,
                           uint32_t th, Grid* g) {
    g->tiles_x = g->tiles_y = g->tiles = 0;
    if (!src || !dst) return "null pointer";
    if (convolve && !weights) return "null weights";
    if (!convolve && (op < 0 || op > 3)) return "the operation is not an ec_focal_op (0 .. 3)";
    if (flags & ~(kFlagWhole | kFlagNormalize)) return "unknown flag bits";
    if (!convolve && (flags & kFlagNormalize)) return "EC_FOCAL_NORMALIZE is ec_focal_convolve's";
    if (rx > kRadiusCap || ry > kRadiusCap) return "a radius above EC_FOCAL_RADIUS_CAP (7)";
    return raster_refusal(src, dst, src_mask, dst_mask, cols, rows, flags, tw, th, g);
}

// ---- ec_focal_rank / ec_focal_majority: the order statistics of a footprint (ec_focal_rank_kernels.hpp)
constexpr uint32_t kRankMaxTaps = 64;   // EC_FOCAL_RANK_MAX_TAPS
constexpr uint32_t kRankMaxDen = 65535; // EC_RANK_MAX_DEN

// Why a call of ec_focal_rank (`rank`) or ec_focal_majority is refused, or null: refusal's checks in refusal's order, the tap count
// directly behind the radius cap, and for ec_focal_rank the fraction and the method at the end.  EC_FOCAL_WHOLE is the only flag.
inline const char* rank_refusal(bool rank, const void* src, const void* dst, const void* src_mask, const void* dst_mask, uint64_t cols,
                                uint64_t rows, uint32_t rx, uint32_t ry, uint32_t num, uint32_t den, int32_t method, uint32_t flags,
                                uint32_t tw, uint32_t th, Grid* g) {
    g->tiles_x = g->tiles_y = g->tiles = 0;
    if (!src || !dst) return "null pointer";
    if (flags & ~kFlagWhole) return "unknown flag bits";
    if (rx > kRadiusCap || ry > kRadiusCap) return "a radius above EC_FOCAL_RADIUS_CAP (7)";
    if ((2 * rx + 1) * (2 * ry + 1) > kRankMaxTaps) return "more than EC_FOCAL_RANK_MAX_TAPS (64) taps in the footprint";
    if (const char* why = raster_refusal(src, dst, src_mask, dst_mask, cols, rows, flags, tw, th, g)) return why;
    if (rank) {
        if (den < 1 || den > kRankMaxDen || num > den) {
            g->tiles = 0;
            return "q = num / den needs 1 <= den <= EC_RANK_MAX_DEN (65535) and num <= den";
        }
        if (method != 0 && method != 1) {
            g->tiles = 0;
            return "the method is not an ec_rank_method (0 .. 1)";
        }
    }
    return nullptr;
}

// The stage of layout_of(kConvolve) — cells and mask bytes, no row results — and behind it the tile's results on their way from the
// lane that sorted a cell to the lane that stores its 16-byte slot: th rows of tw results of `cell` bytes (off_racc) and th rows
// of tw validity bytes (off_rcnt).
EC_FOCAL_HD Layout rank_layout_of(uint32_t cell, bool masked, uint32_t rx, uint32_t ry, uint32_t tw, uint32_t th) {
    Layout l = layout_of(cell, masked, kConvolve, rx, ry, tw, th);
    l.off_racc = l.bytes;
    l.off_rcnt = l.off_racc + th * tw * cell;
    l.bytes = l.off_rcnt + round16(th * tw);
    return l;
}

}  // namespace ecf
