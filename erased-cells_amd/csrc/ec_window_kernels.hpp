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
#pragma once

#include "ec_binop_kernels.hpp"

namespace ecd {

constexpr int kWindowU = 4;  // 16-byte slots per lane per tile

template <int W> struct width_cell;
template <> struct width_cell<1> { using type = uint8_t; };
template <> struct width_cell<2> { using type = uint16_t; };
template <> struct width_cell<4> { using type = uint32_t; };
template <> struct width_cell<8> { using type = uint64_t; };

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

// cell k of a slot's four dwords (k is a constant after unrolling)
template <int W>
__device__ __forceinline__ void slot_put(u32x4& v, int k, typename width_cell<W>::type c) {
    if constexpr (W == 1) v[k >> 2] |= uint32_t(c) << (8 * (k & 3));
    else if constexpr (W == 2) v[k >> 1] |= uint32_t(c) << (16 * (k & 1));
    else if constexpr (W == 4) v[k] = c;
    else {
        v[2 * k] = uint32_t(c);
        v[2 * k + 1] = uint32_t(c >> 32);
    }
}
template <int W>
__device__ __forceinline__ typename width_cell<W>::type slot_get(const u32x4& v, int k) {
    using C = typename width_cell<W>::type;
    if constexpr (W == 1) return C((v[k >> 2] >> (8 * (k & 3))) & 0xffu);
    else if constexpr (W == 2) return C((v[k >> 1] >> (16 * (k & 1))) & 0xffffu);
    else if constexpr (W == 4) return v[k];
    else return uint64_t(v[2 * k]) | (uint64_t(v[2 * k + 1]) << 32);
}

// the 16-byte store of a value stream (write-through) or of a mask stream (nt_store / mask_store, ec_device.hpp)
template <bool MASK_ST>
__device__ __forceinline__ void slot_store(u32x4 v, void* p) {
    if constexpr (MASK_ST) mask_store(v, static_cast<u32x4*>(p));
    else nt_store(v, static_cast<u32x4*>(p));
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

// What the three tile bodies share.  A tile is TILE_SLOTS slots of the contiguous side starting at cell `first`, which lies at
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

// ---- cut: contiguous[c] = raster[window cell c].  `cacheable`: the raster stream's load-policy bit (cache_plan, ec_runtime.hpp).
template <int W, int TILE_SLOTS, bool MASK_ST>
__device__ __forceinline__ void window_copy_tile(const typename width_cell<W>::type* __restrict__ src,
                                                 typename width_cell<W>::type* __restrict__ dst, const WindowGeom& g, uint64_t first,
                                                 uint64_t row0, uint64_t col0, unsigned cacheable) {
    using C = typename width_cell<W>::type;
    using L = TileLanes<W, TILE_SLOTS>;
    constexpr int CPL = L::CPL, NJ = L::NJ;
    const L t(g, first, row0, col0);
    const C* __restrict__ win = src + g.origin;
    u32x4 v[NJ];
    policy_arms<1>(cacheable, [&](auto bits) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            v[j] = u32x4{0, 0, 0, 0};
            if (t.one_row[j]) v[j] = load_vec<!(decltype(bits)::value & 1u)>(reinterpret_cast<const u32x4*>(win + t.rc[j].row * g.pitch + t.rc[j].col));
        }
    });
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (t.live[j] && !t.one_row[j]) {  // over a row end, or the last cells of the window: cell by cell
            uint64_t col = t.rc[j].col;
            const C* p = win + t.rc[j].row * g.pitch + col;
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                if (t.c0[j] + k < g.n) {
                    slot_put<W>(v[j], k, ld_cell(p));
                    ++p;
                    if (++col == g.w) {
                        col = 0;
                        p += g.pitch - g.w;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (t.whole[j]) {
            slot_store<MASK_ST>(v[j], dst + t.c0[j]);
        } else if (t.live[j]) {
#pragma unroll
            for (int k = 0; k < CPL; ++k)
                if (t.c0[j] + k < g.n) st_cell(slot_get<W>(v[j], k), dst + t.c0[j] + k);
        }
    }
}

// ---- paste: raster[window cell c] = contiguous[c].  Vector stores only inside one row of the window; nothing outside it is written.
template <int W, int TILE_SLOTS, bool MASK_ST>
__device__ __forceinline__ void window_put_tile(const typename width_cell<W>::type* __restrict__ tile,
                                                typename width_cell<W>::type* __restrict__ dst, const WindowGeom& g, uint64_t first,
                                                uint64_t row0, uint64_t col0, unsigned cacheable) {
    using C = typename width_cell<W>::type;
    using L = TileLanes<W, TILE_SLOTS>;
    constexpr int CPL = L::CPL, NJ = L::NJ;
    const L t(g, first, row0, col0);
    C* __restrict__ win = dst + g.origin;
    u32x4 v[NJ];
    policy_arms<1>(cacheable, [&](auto bits) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            v[j] = u32x4{0, 0, 0, 0};
            if (t.whole[j]) v[j] = load_vec<!(decltype(bits)::value & 1u)>(reinterpret_cast<const u32x4*>(tile + t.c0[j]));
        }
    });
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (t.live[j] && !t.whole[j]) {  // the last cells of the tile
#pragma unroll
            for (int k = 0; k < CPL; ++k)
                if (t.c0[j] + k < g.n) slot_put<W>(v[j], k, ld_cell(tile + t.c0[j] + k));
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        C* p = win + t.rc[j].row * g.pitch + t.rc[j].col;
        if (t.one_row[j]) {
            slot_store<MASK_ST>(v[j], p);
        } else if (t.live[j]) {
            uint64_t col = t.rc[j].col;
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                if (t.c0[j] + k < g.n) {
                    st_cell(slot_get<W>(v[j], k), p);
                    ++p;
                    if (++col == g.w) {
                        col = 0;
                        p += g.pitch - g.w;
                    }
                }
            }
        }
    }
}

// ---- cut and resample: contiguous[(i, j)] = raster[window cell (rows(i), cols(j))], per-cell gathers, 16-byte stores.  The source row
// is found once per slot and stepped at a row end of the output, not per cell.
template <int W, int TILE_SLOTS, bool MASK_ST>
__device__ __forceinline__ void window_nearest_tile(const typename width_cell<W>::type* __restrict__ src,
                                                    typename width_cell<W>::type* __restrict__ dst, const WindowGeom& g,
                                                    const WindowAxis& ax, const WindowAxis& ay, uint64_t first, uint64_t row0,
                                                    uint64_t col0, unsigned cacheable) {
    using C = typename width_cell<W>::type;
    using L = TileLanes<W, TILE_SLOTS>;
    constexpr int CPL = L::CPL, NJ = L::NJ;
    const L t(g, first, row0, col0);
    const C* __restrict__ win = src + g.origin;
    u32x4 v[NJ];
    policy_arms<1>(cacheable, [&](auto bits) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            v[j] = u32x4{0, 0, 0, 0};
            if (t.live[j]) {
                AxisPos y = axis_at(ay, t.rc[j].row), x = axis_at(ax, t.rc[j].col);
                uint64_t col = t.rc[j].col;
                const C* row = win + y.src * g.pitch;
#pragma unroll
                for (int k = 0; k < CPL; ++k) {
                    if (t.c0[j] + k < g.n) {
                        C c;
                        if constexpr (decltype(bits)::value & 1u) c = row[x.src];
                        else c = ld_cell(row + x.src);
                        slot_put<W>(v[j], k, c);
                        axis_step(ax, x);
                        if (++col == g.w) {
                            col = 0;
                            x = axis_first(ax);
                            axis_step(ay, y);
                            row = win + y.src * g.pitch;
                        }
                    }
                }
            }
        }
    });
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (t.whole[j]) {
            slot_store<MASK_ST>(v[j], dst + t.c0[j]);
        } else if (t.live[j]) {
#pragma unroll
            for (int k = 0; k < CPL; ++k)
                if (t.c0[j] + k < g.n) st_cell(slot_get<W>(v[j], k), dst + t.c0[j] + k);
        }
    }
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

enum { kWinCopy = 0, kWinPut = 1 };

// One workgroup per tile of kBlock * kWindowU value slots; the mask bytes of the SAME cells are 1 / W as many slots, with their own
// lane map (16 mask bytes per lane, as mask_and_body has), so one division serves both streams.
template <int W, bool MASKED, int KIND>
__device__ __forceinline__ void window_body(const WindowArgs& a, const WindowAxis* ax, const WindowAxis* ay) {
    using C = typename width_cell<W>::type;
    constexpr int SLOTS = kBlock * kWindowU, MSLOTS = SLOTS / W;
    const uint64_t first = uint64_t(two_front_tile()) * (uint64_t(SLOTS) * (16 / W));
    const uint64_t row0 = first / a.g.w, col0 = first - row0 * a.g.w;  // wave-uniform, once per workgroup
    if (first >= a.g.n) return;
    if (ax) {
        window_nearest_tile<W, SLOTS, false>(static_cast<const C*>(a.in), static_cast<C*>(a.out), a.g, *ax, *ay, first, row0, col0, a.cacheable);
        if constexpr (MASKED) window_nearest_tile<1, MSLOTS, true>(a.in_mask, a.out_mask, a.g, *ax, *ay, first, row0, col0, a.cacheable >> 1);
    } else if constexpr (KIND == kWinCopy) {
        window_copy_tile<W, SLOTS, false>(static_cast<const C*>(a.in), static_cast<C*>(a.out), a.g, first, row0, col0, a.cacheable);
        if constexpr (MASKED) window_copy_tile<1, MSLOTS, true>(a.in_mask, a.out_mask, a.g, first, row0, col0, a.cacheable >> 1);
    } else {
        window_put_tile<W, SLOTS, false>(static_cast<const C*>(a.in), static_cast<C*>(a.out), a.g, first, row0, col0, a.cacheable);
        if constexpr (MASKED) window_put_tile<1, MSLOTS, true>(a.in_mask, a.out_mask, a.g, first, row0, col0, a.cacheable >> 1);
    }
}

template <int W, bool MASKED>
__global__ __launch_bounds__(kBlock) void k_window_copy(WindowArgs a) { window_body<W, MASKED, kWinCopy>(a, nullptr, nullptr); }
template <int W, bool MASKED>
__global__ __launch_bounds__(kBlock) void k_window_put(WindowArgs a) { window_body<W, MASKED, kWinPut>(a, nullptr, nullptr); }
template <int W, bool MASKED>
__global__ __launch_bounds__(kBlock) void k_window_nearest(WindowArgs a, WindowAxis ax, WindowAxis ay) { window_body<W, MASKED, kWinCopy>(a, &ax, &ay); }

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
