// ec_window_kernels.hpp — 2-D windows of a raster resident in HBM (gfx950): cut one out (k_window_copy), cut it out at another
// size by nearest neighbour (k_window_nearest), paste a tile into one (k_window_put).  The device part of the reference's
// read_cells(window, window_size, size, e_resample_alg) (src/gdal/rasterband.rs:82-125) once the band's cells are on the device.
//
// Every kernel is a copy of cells, so it is typed by cell WIDTH only (W = 1, 2, 4, 8 bytes; a mask is the 1-byte instance), as the
// load classes of k_fused_any are.  The CONTIGUOUS side (the output of a cut, the tile of a paste) is the linear stream and takes the
// launch shape of the other streaming kernels: 256-thread workgroups, one workgroup per tile, straight-line, two fronts; each lane owns
// 16-byte slots (16 / W cells) of it, moved as four dwords at every width (1-byte cells as <16 x i8> would lose `nt`, ec_device.hpp).
// The RASTER side is addressed row by row.  A slot whose cells lie in one row of the window is ONE under-aligned 16-byte access there
// (row starts fall on every alignment; such accesses run at 92-100 % of the aligned rate, profiles/r01/unaligned_windows.md); a slot
// that straddles a row end goes cell by cell.  A paste therefore never writes a byte outside its window.
//
// Where a lane's slot sits in the window: the workgroup divides the first cell of its tile by the window width ONCE (wave-uniform);
// a lane adds its offset inside the tile and steps to its row by one compare-and-subtract when the window is at least a tile wide,
// by a 32-bit division when it is narrower (the sum then fits 32 bits).  No lane divides 64-bit numbers on the copy and paste paths.
//
// ONE TILE FRAME.  The three kernels are one body (window_move) over two SIDES, each written once: the contiguous side and the raster
// side say where a slot is one 16-byte access and walk its cells where it is not; a cut loads from the raster side and stores to the
// contiguous one, a paste the other way round, a cut at another size gathers its source through two axes instead of loading it.
// The walk over a row end (RowCursor) is the one k_window_resample uses too (ec_window_resample_kernels.hpp).  The slot itself and
// the workgroup -> tile map are every tiled kernel's: ec_tile.hpp.  Registers and first timings: profiles/window/frame.md.
#pragma once

#include "ec_tile.hpp"

namespace ecd {

constexpr int kWindowU = 4;  // 16-byte slots per lane per tile
constexpr int kWindowTileSlots = kBlock * kWindowU;  // value slots per tile; the host counts a launch's tiles by it (window_tiles, ec_window_checks.hpp)

// A window of a row-major raster and the contiguous side that faces it, in cells.
struct WindowGeom {
    uint64_t pitch;   // cells per raster row
    uint64_t origin;  // y0 * pitch + x0: the window's first cell
    uint64_t w;       // cells per row of the contiguous side
    uint64_t n;       // cells of the contiguous side (w * rows)
};

// Nearest neighbour along one axis, in integers: output index j of `out` reads source index floor((2 j + 1) * win / (2 * out)) of the
// window — the cell-centre rule (j + 0.5) * win / out evaluated exactly.  With win = q * out + r this is j * q + (q * out + (2 j + 1) * r)
// / (2 * out); from one j to the next the numerator grows by 2 r < 2 * out, so a lane divides once for its slot's first cell and steps
// the others (at most one carry each).  d0 / rem0: the state at j = 0, where a slot that runs over a row end starts again.
struct WindowAxis {
    uint64_t q, r, out, d0, rem0;
};
struct AxisPos {
    uint64_t src, rem;
};
__device__ __forceinline__ AxisPos axis_at(const WindowAxis& a, uint64_t j) {
    const uint64_t two = 2 * a.out, num = a.q * a.out + (2 * j + 1) * a.r, d = num / two;  // no overflow: checked by the host
    return AxisPos{j * a.q + d, num - d * two};
}
__device__ __forceinline__ AxisPos axis_first(const WindowAxis& a) { return AxisPos{a.d0, a.rem0}; }
__device__ __forceinline__ void axis_step(const WindowAxis& a, AxisPos& p) {
    p.src += a.q;
    p.rem += 2 * a.r;
    if (p.rem >= 2 * a.out) {
        p.rem -= 2 * a.out;
        ++p.src;
    }
}

struct RowCol {
    uint64_t row, col;
};
// (row, col) of the cell `off` cells behind (row0, col0), off < SPAN
template <uint32_t SPAN>
__device__ __forceinline__ RowCol lane_row_col(uint64_t row0, uint64_t col0, uint32_t off, uint64_t w) {
    if (w >= SPAN) {  // wave-uniform
        const uint64_t c = col0 + off;
        const bool wrap = c >= w;
        return RowCol{row0 + (wrap ? 1u : 0u), wrap ? c - w : c};
    }
    const uint32_t w32 = static_cast<uint32_t>(w), x = static_cast<uint32_t>(col0) + off, q = x / w32;
    return RowCol{row0 + q, uint64_t(x - q * w32)};
}

// The lane map of a tile, which its two sides share.  A tile is TILE_SLOTS slots of the contiguous side starting at cell `first`, which lies at
// (row0, col0) of the window; lane t owns slots t, t + 256, ... (NJ of them; the mask stream of a launch over wide cells has fewer
// slots than lanes).
template <int W, int TILE_SLOTS>
struct TileLanes {
    static constexpr int CPL = 16 / W;
    static constexpr int NJ = (TILE_SLOTS + kBlock - 1) / kBlock;
    static constexpr uint32_t SPAN = uint32_t(TILE_SLOTS) * CPL;
    uint64_t c0[NJ];   // first cell of the slot on the contiguous side
    RowCol rc[NJ];     // where it lies in the window
    bool live[NJ];     // the slot has a cell below n
    bool whole[NJ];    // all its CPL cells exist
    bool one_row[NJ];  // ... and lie in one row of the window
    __device__ __forceinline__ TileLanes(const WindowGeom& g, uint64_t first, uint64_t row0, uint64_t col0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const uint32_t s = threadIdx.x + uint32_t(j) * kBlock;
            const uint32_t off = s * CPL;
            c0[j] = first + off;
            rc[j] = lane_row_col<SPAN>(row0, col0, off, g.w);
            live[j] = (TILE_SLOTS % kBlock == 0 || s < uint32_t(TILE_SLOTS)) && c0[j] < g.n;
            whole[j] = live[j] && c0[j] + CPL <= g.n;
            one_row[j] = whole[j] && rc[j].col + CPL <= g.w;
        }
    }
};

// The row-end cursor: a walk over cells in the order of the contiguous side.  It owns the column; where the walk stands on the raster
// side is the caller's (a cell pointer for the copy and the paste, a pair of axis positions for the resampling kernels), and so is
// `row_end`, which takes that position from the last cell of a row of the window to the first cell of the next.
struct RowCursor {
    uint64_t col, w;
    template <typename E>
    __device__ __forceinline__ void next(E&& row_end) {
        if (++col == w) {
            col = 0;
            row_end();
        }
    }
};
// cell(k) for the cells of a slot that exist — cell k is cell c0 + k of the n the contiguous side has — each followed by the cursor's step
template <int CPL, typename F, typename E>
__device__ __forceinline__ void walk_slot(uint64_t c0, uint64_t n, RowCursor at, F&& cell, E&& row_end) {
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        if (c0 + k < n) {
            cell(k);
            at.next(row_end);
        }
    }
}

// The two sides of a tile as its body sees them (P: a pointer to cells, const on the side that is read).  Slot j is ONE 16-byte access
// at at(j) where vector(j) holds; else cells(j, f) calls f(k, p) for each of its cells that exists, p where cell k lies.
// The contiguous side: a slot's cells follow one another; it is whole unless it holds the last cells of the tile.
template <typename P, typename L>
struct ContiguousSide {
    P base;
    const L& t;
    uint64_t n;
    __device__ __forceinline__ bool vector(int j) const { return t.whole[j]; }
    __device__ __forceinline__ P at(int j) const { return base + t.c0[j]; }
    template <typename F>
    __device__ __forceinline__ void cells(int j, F&& f) const {
#pragma unroll
        for (int k = 0; k < L::CPL; ++k)
            if (t.c0[j] + k < n) f(k, base + t.c0[j] + k);
    }
};
// The raster side (`win`: the window's first cell): a whole slot inside one row of the window is one under-aligned access; over a
// row end the cursor takes it cell by cell, so that a paste writes nothing outside its window.
template <typename P, typename L>
struct RasterSide {
    P win;
    const L& t;
    const WindowGeom& g;
    __device__ __forceinline__ bool vector(int j) const { return t.one_row[j]; }
    __device__ __forceinline__ P at(int j) const { return win + t.rc[j].row * g.pitch + t.rc[j].col; }
    template <typename F>
    __device__ __forceinline__ void cells(int j, F&& f) const {
        P p = at(j);
        walk_slot<L::CPL>(t.c0[j], g.n, RowCursor{t.rc[j].col, g.w}, [&](int k) { f(k, p++); }, [&] { p += g.pitch - g.w; });
    }
};

// One slot of a cut at another size: contiguous[(i, j)] = raster[window cell (rows(i), cols(j))], gathered cell by cell.  The source
// row is found once per slot and stepped at a row end of the output, not per cell.  NT: the arm of the load policy.
template <int W, bool NT>
__device__ __forceinline__ void nearest_slot(u32x4& v, const typename width_cell<W>::type* win, const WindowGeom& g, uint64_t c0, RowCol rc,
                                             const WindowAxis& ax, const WindowAxis& ay) {
    using C = typename width_cell<W>::type;
    AxisPos y = axis_at(ay, rc.row), x = axis_at(ax, rc.col);
    const C* row = win + y.src * g.pitch;
    walk_slot<16 / W>(
        c0, g.n, RowCursor{rc.col, g.w},
        [&](int k) {
            C c;
            if constexpr (NT) c = ld_cell(row + x.src);
            else c = row[x.src];
            slot_put<W>(v, k, c);
            axis_step(ax, x);
        },
        [&] {
            x = axis_first(ax);
            axis_step(ay, y);
            row = win + y.src * g.pitch;
        });
}

// The tile body: the lanes' slots, zeroed, are filled from one side and stored to the other.  All 16-byte loads of the tile are
// issued in one arm of the load policy (`cacheable`: the loaded stream's bit, cache_plan, ec_runtime.hpp) before any cell-wise
// access, and every load comes before the first store.  AXES: none for the copy and the paste; the two axes of a nearest-neighbour
// cut, whose source side is gathered (nearest_slot) in the arm instead.
template <int W, bool MASK_ST, typename L, typename FROM, typename TO, typename... AXES>
__device__ __forceinline__ void window_move(const L& t, const FROM& from, const TO& to, unsigned cacheable, const AXES&... axes) {
    constexpr int NJ = L::NJ;
    constexpr bool GATHER = sizeof...(AXES) != 0;
    u32x4 v[NJ];
    policy_arms<1>(cacheable, [&](auto bits) {
        constexpr bool NT = !(decltype(bits)::value & 1u);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            v[j] = u32x4{0, 0, 0, 0};
            if constexpr (GATHER) {
                if (t.live[j]) nearest_slot<W, NT>(v[j], from.win, from.g, t.c0[j], t.rc[j], axes...);
            } else {
                if (from.vector(j)) v[j] = load_vec<NT>(reinterpret_cast<const u32x4*>(from.at(j)));
            }
        }
    });
    if constexpr (!GATHER) {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (t.live[j] && !from.vector(j)) from.cells(j, [&](int k, auto p) { slot_put<W>(v[j], k, ld_cell(p)); });
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (to.vector(j)) slot_store<MASK_ST>(v[j], to.at(j));
        else if (t.live[j]) to.cells(j, [&](int k, auto p) { st_cell(slot_get<W>(v[j], k), p); });
    }
}

enum { kWinCopy = 0, kWinPut = 1 };

// One stream of a launch, values or mask bytes, over a tile of TILE_SLOTS slots that starts at cell `first` = (row0, col0) of the
// window.  cut: contiguous[c] = raster[window cell c], at the window's size or (with axes) at another; paste: the other way round.
template <int W, int TILE_SLOTS, bool MASK_ST, int KIND, typename... AXES>
__device__ __forceinline__ void window_tile(const typename width_cell<W>::type* __restrict__ in, typename width_cell<W>::type* __restrict__ out,
                                            const WindowGeom& g, uint64_t first, uint64_t row0, uint64_t col0, unsigned cacheable,
                                            const AXES&... axes) {
    using C = typename width_cell<W>::type;
    using L = TileLanes<W, TILE_SLOTS>;
    const L t(g, first, row0, col0);
    if constexpr (KIND == kWinPut) window_move<W, MASK_ST>(t, ContiguousSide<const C*, L>{in, t, g.n}, RasterSide<C*, L>{out + g.origin, t, g}, cacheable);
    else window_move<W, MASK_ST>(t, RasterSide<const C*, L>{in + g.origin, t, g}, ContiguousSide<C*, L>{out, t, g.n}, cacheable, axes...);
}

// Launch arguments: the value stream (raster side / contiguous side) and, for MASKED launches, the mask stream over the same cells.
// `cacheable`: bit 0 = the values that are loaded, bit 1 = the mask bytes that are loaded.
struct WindowArgs {
    const void* in;
    void* out;
    const uint8_t* in_mask;
    uint8_t* out_mask;
    WindowGeom g;
    unsigned cacheable;
};

// One workgroup per tile of kWindowTileSlots value slots; the mask bytes of the SAME cells are 1 / W as many slots, with their own
// lane map (16 mask bytes per lane, as the binop's mask_and_body has), so one division serves both streams.  The axes of a
// nearest-neighbour cut come by reference to the kernel's own arguments: nothing takes their address, so they stay in registers.
template <int W, bool MASKED, int KIND, typename... AXES>
__device__ __forceinline__ void window_body(const WindowArgs& a, const AXES&... axes) {
    using C = typename width_cell<W>::type;
    constexpr int SLOTS = kWindowTileSlots, MSLOTS = SLOTS / W;
    const uint64_t first = uint64_t(two_front_tile()) * (uint64_t(SLOTS) * (16 / W));
    const uint64_t row0 = first / a.g.w, col0 = first - row0 * a.g.w;  // wave-uniform, once per workgroup
    if (first >= a.g.n) return;
    window_tile<W, SLOTS, false, KIND>(static_cast<const C*>(a.in), static_cast<C*>(a.out), a.g, first, row0, col0, a.cacheable, axes...);
    if constexpr (MASKED) window_tile<1, MSLOTS, true, KIND>(a.in_mask, a.out_mask, a.g, first, row0, col0, a.cacheable >> 1, axes...);
}

template <int W, bool MASKED>
__global__ __launch_bounds__(kBlock) void k_window_copy(WindowArgs a) { window_body<W, MASKED, kWinCopy>(a); }
template <int W, bool MASKED>
__global__ __launch_bounds__(kBlock) void k_window_put(WindowArgs a) { window_body<W, MASKED, kWinPut>(a); }
template <int W, bool MASKED>
__global__ __launch_bounds__(kBlock) void k_window_nearest(WindowArgs a, WindowAxis ax, WindowAxis ay) { window_body<W, MASKED, kWinCopy>(a, ax, ay); }

// ---- the comparison path ("unaligned_vector" = 0 and a row start that is not 16-byte aligned): one cell per lane, plain accesses.
// A workgroup takes 256 cells of one row of the contiguous side at a time.  PUT = false serves the cut at either size (the copy is
// the resampling with q = 1, r = 0 on both axes).
template <int W, bool MASKED, bool PUT>
__global__ __launch_bounds__(kBlock) void k_window_cellwise(WindowArgs a, WindowAxis ax, WindowAxis ay) {
    using C = typename width_cell<W>::type;
    const uint64_t chunks = (a.g.w + kBlock - 1) / kBlock, rows = a.g.n / a.g.w;
    for (uint64_t b = blockIdx.x; b < chunks * rows; b += gridDim.x) {
        const uint64_t row = b / chunks, col = (b - row * chunks) * kBlock + threadIdx.x;
        if (col >= a.g.w) continue;
        const uint64_t flat = row * a.g.w + col;
        if constexpr (PUT) {
            const uint64_t at = a.g.origin + row * a.g.pitch + col;
            static_cast<C*>(a.out)[at] = static_cast<const C*>(a.in)[flat];
            if constexpr (MASKED) a.out_mask[at] = a.in_mask[flat];
        } else {
            const uint64_t at = a.g.origin + axis_at(ay, row).src * a.g.pitch + axis_at(ax, col).src;
            static_cast<C*>(a.out)[flat] = static_cast<const C*>(a.in)[at];
            if constexpr (MASKED) a.out_mask[flat] = a.in_mask[at];
        }
    }
}

}  // namespace ecd
