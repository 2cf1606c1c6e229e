// ec_window.hip — ec_window / ec_window_put (include/erased_cells.h): the argument checks and the launches of the window kernels
// (ec_window_kernels.hpp).  Every argument check comes before any device work, so a bad call fails the same way with or without a device.
#include <hip/hip_runtime.h>

#include "ec_dispatch.hpp"
#include "ec_lattice.hpp"
#include "ec_runtime.hpp"
#include "ec_window_checks.hpp"
#include "ec_window_kernels.hpp"

namespace ecd {

// Nearest neighbour along one axis (WindowAxis, ec_window_kernels.hpp); false if the kernel's 64-bit numerator could overflow.
static bool make_axis(uint64_t win, uint64_t out, WindowAxis* a) {
    a->q = win / out;
    a->r = win % out;
    a->out = out;
    if (out > (UINT64_MAX >> 2)) return false;  // the kernel's remainder + 2 r stays below 2^64
    const unsigned __int128 worst = (unsigned __int128)(2 * out) * a->r + win;  // q * out + (2 j + 1) * r for j < out
    if (worst > UINT64_MAX) return false;
    const uint64_t num = a->q * out + a->r;
    a->d0 = num / (2 * out);
    a->rem0 = num % (2 * out);
    return true;
}

// do the row starts of both sides fall on 16-byte boundaries?  (only asked when "unaligned_vector" is off)
static bool rows_aligned(const void* raster, const WindowGeom& g, size_t cell, const void* contiguous) {
    return ((reinterpret_cast<uintptr_t>(raster) + g.origin * cell) | (g.pitch * cell) | (g.w * cell) | reinterpret_cast<uintptr_t>(contiguous)) % 16 == 0;
}

template <int W, bool MASKED>
static ec_status launch_window(int kind, const WindowArgs& args, const WindowAxis* ax, const WindowAxis* ay, bool vector, hipStream_t s) {
    WindowArgs a = args;
    // the streams of the launch are the bytes the window touches, not the raster
    const size_t bytes[2] = {a.g.n * W, MASKED ? a.g.n : 0};
    a.cacheable = cache_plan(bytes, 2);
    if (!vector) {
        const uint64_t chunks = ((a.g.w + kBlock - 1) / kBlock) * (a.g.n / a.g.w);
        const WindowAxis id_x{1, 0, a.g.w, 0, a.g.w}, id_y{1, 0, a.g.n / a.g.w, 0, a.g.n / a.g.w};
        if (kind == kWinPut) k_window_cellwise<W, MASKED, true><<<grid_capped(chunks, 8), kBlock, 0, s>>>(a, id_x, id_y);
        else k_window_cellwise<W, MASKED, false><<<grid_capped(chunks, 8), kBlock, 0, s>>>(a, ax ? *ax : id_x, ay ? *ay : id_y);
        return check_launch("window(cell-wise)");
    }
    const uint64_t tiles = window_tiles(a.g.n, W, kWindowTileSlots);
    if (const ec_status st = check_groups("window", tiles)) return st;  // a window of 256 GiB
    const unsigned grid = grid_for(tiles);
    if (ax) k_window_nearest<W, MASKED><<<grid, kBlock, 0, s>>>(a, *ax, *ay);
    else if (kind == kWinPut) k_window_put<W, MASKED><<<grid, kBlock, 0, s>>>(a);
    else k_window_copy<W, MASKED><<<grid, kBlock, 0, s>>>(a);
    return check_launch(ax ? "window(nearest)" : kind == kWinPut ? "window(put)" : "window(copy)");
}

static ec_status dispatch_window(size_t cell, bool masked, int kind, const WindowArgs& a, const WindowAxis* ax, const WindowAxis* ay, bool vector,
                                 hipStream_t s) {
    return ecl::with_cell_width(cell, [&](auto w) {
        constexpr int W = sizeof(ecl::cell_t<decltype(w)>);
        return masked ? launch_window<W, true>(kind, a, ax, ay, vector, s) : launch_window<W, false>(kind, a, ax, ay, vector, s);
    }, kTypeChecked);
}

}  // namespace ecd

using namespace ecd;

extern "C" ec_status ec_window(ec_dtype t, const void* src, const uint8_t* src_mask_or_null, uint64_t src_cols, uint64_t src_rows, uint64_t x0,
                               uint64_t y0, uint64_t win_cols, uint64_t win_rows, uint64_t out_cols, uint64_t out_rows, void* dst,
                               uint8_t* dst_mask_or_null, ec_stream stream) {
    bool nothing = false;
    ec_status st = check_cut("ec_window", t, src, src_mask_or_null, src_cols, src_rows, x0, y0, win_cols, win_rows, out_cols, out_rows, dst, dst_mask_or_null, &nothing);
    if (st != EC_OK || nothing) return st;
    const bool resample = out_cols != win_cols || out_rows != win_rows;
    WindowAxis ax, ay;
    if (resample && !(make_axis(win_cols, out_cols, &ax) && make_axis(win_rows, out_rows, &ay)))
        return set_error(EC_ERR_ARG, "ec_window: %llu x %llu -> %llu x %llu is beyond the 64-bit arithmetic of the resampling rule", (unsigned long long)win_cols,
                         (unsigned long long)win_rows, (unsigned long long)out_cols, (unsigned long long)out_rows);
    st = ensure_ready();
    if (st != EC_OK) return st;
    const size_t cell = ecl::size_of(t);
    WindowArgs a{src, dst, src_mask_or_null, dst_mask_or_null, WindowGeom{src_cols, y0 * src_cols + x0, out_cols, out_cols * out_rows}, 0};
    const WindowGeom in_rows{src_cols, a.g.origin, win_cols, 0};
    const bool vector = tuning().unaligned_vector ||
                        (rows_aligned(src, in_rows, cell, dst) && (!src_mask_or_null || rows_aligned(src_mask_or_null, in_rows, 1, dst_mask_or_null)));
    return dispatch_window(cell, src_mask_or_null != nullptr, kWinCopy, a, resample ? &ax : nullptr, resample ? &ay : nullptr, vector, static_cast<hipStream_t>(stream));
}

extern "C" ec_status ec_window_put(ec_dtype t, const void* tile, const uint8_t* tile_mask_or_null, uint64_t win_cols, uint64_t win_rows, void* dst,
                                   uint8_t* dst_mask_or_null, uint64_t dst_cols, uint64_t dst_rows, uint64_t x0, uint64_t y0, ec_stream stream) {
    ec_status st = check_window("ec_window_put", t, dst_cols, dst_rows, x0, y0, win_cols, win_rows, tile_mask_or_null, dst_mask_or_null);
    if (st != EC_OK) return st;
    if (win_cols == 0 || win_rows == 0) return EC_OK;
    if (!tile || !dst) return set_error(EC_ERR_ARG, "ec_window_put: null pointer");
    st = ensure_ready();
    if (st != EC_OK) return st;
    const size_t cell = ecl::size_of(t);
    WindowArgs a{tile, dst, tile_mask_or_null, dst_mask_or_null, WindowGeom{dst_cols, y0 * dst_cols + x0, win_cols, win_cols * win_rows}, 0};
    const bool vector = tuning().unaligned_vector ||
                        (rows_aligned(dst, a.g, cell, tile) && (!tile_mask_or_null || rows_aligned(dst_mask_or_null, a.g, 1, tile_mask_or_null)));
    return dispatch_window(cell, tile_mask_or_null != nullptr, kWinPut, a, nullptr, nullptr, vector, static_cast<hipStream_t>(stream));
}
