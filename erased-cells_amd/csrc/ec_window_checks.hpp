// ec_window_checks.hpp — the argument checks that ec_window, ec_window_put and ec_window_resample share (host code).  All of them come
// before any device work, so a bad call fails the same way with or without a device.
#pragma once

#include <stdint.h>

#include "ec_lattice.hpp"
#include "ec_runtime.hpp"

namespace ecd {

inline bool mul_overflows(uint64_t a, uint64_t b) { return a != 0 && b > UINT64_MAX / a; }

// workgroups of a tiled launch over n cells of `cell` bytes on the contiguous side: one per tile of `tile_slots` 16-byte slots
// (kWindowTileSlots, ec_window_kernels.hpp).  No sum that could overflow: n may be any 64-bit count.
inline uint64_t window_tiles(uint64_t n, size_t cell, uint64_t tile_slots) {
    const uint64_t per_slot = 16 / cell, slots = n / per_slot + (n % per_slot != 0);
    return slots / tile_slots + (slots % tile_slots != 0);
}

// the raster, the window in it and the pair of masks: what the three entry points check alike
inline ec_status check_window(const char* what, ec_dtype t, uint64_t cols, uint64_t rows, uint64_t x0, uint64_t y0, uint64_t w, uint64_t h,
                              const void* mask_a, const void* mask_b) {
    if (!ecl::valid(t)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "%s: bad dtype %d", what, int(t));
    if (mul_overflows(cols, rows))
        return set_error(EC_ERR_ARG, "%s: a raster of %llu x %llu cells overflows 64 bits", what, (unsigned long long)cols, (unsigned long long)rows);
    if (x0 > cols || w > cols - x0 || y0 > rows || h > rows - y0)
        return set_error(EC_ERR_ARG, "%s: the window (%llu, %llu) + %llu x %llu leaves the raster of %llu x %llu cells", what, (unsigned long long)x0,
                         (unsigned long long)y0, (unsigned long long)w, (unsigned long long)h, (unsigned long long)cols, (unsigned long long)rows);
    if ((mask_a == nullptr) != (mask_b == nullptr)) return set_error(EC_ERR_ARG, "%s: one mask without the other", what);
    return EC_OK;
}

// what every cut checks before it looks at its algorithm; *nothing: an empty window with an empty output (EC_OK, no launch)
inline ec_status check_cut(const char* what, ec_dtype t, const void* src, const uint8_t* src_mask, uint64_t src_cols, uint64_t src_rows, uint64_t x0,
                           uint64_t y0, uint64_t win_cols, uint64_t win_rows, uint64_t out_cols, uint64_t out_rows, const void* dst,
                           const uint8_t* dst_mask, bool* nothing) {
    ec_status st = check_window(what, t, src_cols, src_rows, x0, y0, win_cols, win_rows, src_mask, dst_mask);
    if (st != EC_OK) return st;
    const bool win_empty = win_cols == 0 || win_rows == 0, out_empty = out_cols == 0 || out_rows == 0;
    if (win_empty != out_empty)
        return set_error(EC_ERR_ARG, "%s: a window of %llu x %llu cells cannot be read at %llu x %llu", what, (unsigned long long)win_cols,
                         (unsigned long long)win_rows, (unsigned long long)out_cols, (unsigned long long)out_rows);
    *nothing = win_empty;
    if (win_empty) return EC_OK;
    if (mul_overflows(out_cols, out_rows)) return set_error(EC_ERR_ARG, "%s: an output of %llu x %llu cells overflows 64 bits", what, (unsigned long long)out_cols, (unsigned long long)out_rows);
    if (!src || !dst) return set_error(EC_ERR_ARG, "%s: null pointer", what);
    return EC_OK;
}

}  // namespace ecd
