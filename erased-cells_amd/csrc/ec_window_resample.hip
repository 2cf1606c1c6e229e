// ec_window_resample.hip — ec_window_resample (include/erased_cells.h): a window of a resident raster delivered at another size by
// average or bilinear resampling.  The argument checks (ec_window's, then the rule's own) and the launch of k_window_resample
// (ec_window_resample_kernels.hpp).  A translation unit of its own, as the binops have: its twenty kernels compile in parallel with
// ec_window.hip instead of adding to it.
#include <hip/hip_runtime.h>

#include "ec_dispatch.hpp"
#include "ec_window_checks.hpp"
#include "ec_window_resample_kernels.hpp"

namespace ecd {

typedef unsigned __int128 u128;

static uint64_t gcd_u64(uint64_t a, uint64_t b) {
    while (b) {
        const uint64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// One axis of the rule; null, or the name of what leaves 64 bits.  The kernel's products stay below the one checked here.
static const char* make_resample_axis(int32_t alg, uint64_t win, uint64_t out, ResampleAxis* a) {
    if (alg == EC_RESAMPLE_AVERAGE) {
        if ((u128)win * out > UINT64_MAX) return "win * out";
        const uint64_t g = gcd_u64(win, out);
        *a = ResampleAxis{win / g, 0, out / g, win / g, 0, win - 1, 0, 0, 0, 0};
    } else {
        if ((u128)2 * out * win + out > UINT64_MAX) return "2 * out * win + out";
        *a = ResampleAxis{2 * win, win + out, 2 * out, 2 * out, 1, win - 1, 0, 0, 0, 0};
    }
    a->q = a->num / a->den;
    a->r = a->num % a->den;
    a->c0 = a->add / a->den;
    a->f0 = a->add % a->den;
    return nullptr;
}

template <typename T, bool MASKED>
static ec_status launch_resample(const ResampleArgs& args, uint64_t win_cells, hipStream_t s) {
    constexpr size_t W = sizeof(T);
    ResampleArgs a = args;
    const size_t bytes[2] = {win_cells * W, MASKED ? win_cells : 0};  // the streams that are loaded: the window's cells and mask bytes
    a.w.cacheable = cache_plan(bytes, 2);
    return split_launch(window_tiles(a.w.g.n, W, kWindowTileSlots), "window(resample)", [&](size_t first, unsigned grid) {  // at most 2^31 - 1 tiles: checked by the caller
        a.first_tile = first;
        k_window_resample<T, MASKED><<<grid, kBlock, 0, s>>>(a);
    });
}

static ec_status dispatch_resample(ec_dtype t, const ResampleArgs& a, uint64_t win_cells, hipStream_t s) {
    const bool masked = a.w.in_mask != nullptr;
    return ecl::with_cell_type(t, [&](auto c) {
        using T = ecl::cell_t<decltype(c)>;
        return masked ? launch_resample<T, true>(a, win_cells, s) : launch_resample<T, false>(a, win_cells, s);
    }, [&] { return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_window_resample: bad dtype %d", int(t)); });
}

}  // namespace ecd

using namespace ecd;

extern "C" ec_status ec_window_resample(int32_t alg, ec_dtype t, const void* src, const uint8_t* src_mask_or_null, uint64_t src_cols,
                                        uint64_t src_rows, uint64_t x0, uint64_t y0, uint64_t win_cols, uint64_t win_rows, uint64_t out_cols,
                                        uint64_t out_rows, void* dst, uint8_t* dst_mask_or_null, ec_stream stream) {
    if (alg != EC_RESAMPLE_NEAREST && alg != EC_RESAMPLE_BILINEAR && alg != EC_RESAMPLE_AVERAGE)
        return set_error(EC_ERR_ARG, "ec_window_resample: resampling algorithm %d is not one of nearest neighbour (0), bilinear (1), average (5)", int(alg));
    if (alg == EC_RESAMPLE_NEAREST || (out_cols == win_cols && out_rows == win_rows))  // the copy, whatever the algorithm
        return ec_window(t, src, src_mask_or_null, src_cols, src_rows, x0, y0, win_cols, win_rows, out_cols, out_rows, dst, dst_mask_or_null, stream);
    bool nothing = false;
    ec_status st = check_cut("ec_window_resample", t, src, src_mask_or_null, src_cols, src_rows, x0, y0, win_cols, win_rows, out_cols, out_rows, dst, dst_mask_or_null, &nothing);
    if (st != EC_OK || nothing) return st;
    const uint64_t win[2] = {win_cols, win_rows}, out[2] = {out_cols, out_rows};
    ResampleArgs a{};
    ResampleAxis* axes[2] = {&a.ax, &a.ay};
    for (int k = 0; k < 2; ++k) {
        const char* axis = k ? "rows" : "columns";
        if (alg == EC_RESAMPLE_AVERAGE && (u128)win[k] > (u128)EC_WINDOW_MAX_REDUCTION * out[k])
            return set_error(EC_ERR_ARG, "ec_window_resample: an average of %llu %s into %llu reduces by more than %d to 1 (EC_WINDOW_MAX_REDUCTION); chain calls",
                             (unsigned long long)win[k], axis, (unsigned long long)out[k], int(EC_WINDOW_MAX_REDUCTION));
        if (const char* over = make_resample_axis(alg, win[k], out[k], axes[k]))
            return set_error(EC_ERR_ARG, "ec_window_resample: %s of %llu -> %llu %s overflows 64 bits", over, (unsigned long long)win[k],
                             (unsigned long long)out[k], axis);
    }
    if (alg == EC_RESAMPLE_BILINEAR && (u128)4 * out_cols * out_rows > UINT64_MAX)  // out_cols * out_rows fits: checked above
        return set_error(EC_ERR_ARG, "ec_window_resample: the total weight 4 * %llu * %llu of a bilinear footprint overflows 64 bits",
                         (unsigned long long)out_cols, (unsigned long long)out_rows);
    if (window_tiles(out_cols * out_rows, ecl::size_of(t), kWindowTileSlots) > 0x7fffffffu)
        return set_error(EC_ERR_ARG, "ec_window_resample: an output of %llu x %llu cells is more than 2^31 - 1 tiles", (unsigned long long)out_cols,
                         (unsigned long long)out_rows);
    st = ensure_ready();
    if (st != EC_OK) return st;
    a.w = WindowArgs{src, dst, src_mask_or_null, dst_mask_or_null, WindowGeom{src_cols, y0 * src_cols + x0, out_cols, out_cols * out_rows}, 0};
    a.cellwise_stores = !(tuning().unaligned_vector || (reinterpret_cast<uintptr_t>(dst) % 16 == 0 && reinterpret_cast<uintptr_t>(dst_mask_or_null) % 16 == 0));
    return dispatch_resample(t, a, win_cols * win_rows, static_cast<hipStream_t>(stream));
}
