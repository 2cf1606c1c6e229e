// ec_focal.hip — ec_focal and ec_focal_convolve (include/erased_cells.h): moving-window sum, mean, minimum, maximum and weighted sum
// of a resident raster.  The refusals (ecf::refusal, ec_focal_plan.hpp: before any device work and before the library asks for a
// device), the launch arguments of every moving window (focal_args: ec_focal_rank.hip calls it too) and the launches of k_focal /
// k_focal_convolve (ec_focal_kernels.hpp).  A translation unit of its own, as the windows have: its sixty kernels (ten cell types x
// masked or not x sum-mean, min-max, convolve) compile beside the others.
#include <hip/hip_runtime.h>

#include <cstring>

#include "ec_dispatch.hpp"
#include "ec_focal_kernels.hpp"
#include "ec_runtime.hpp"

namespace ecd {

// declared in ec_focal_kernels.hpp.  `lds` is the stage for cells of ecl::size_of(t) bytes — of no bytes for a bad dtype, which is
// refused here before anything reads it.
ec_status focal_args(const char* what, ec_dtype t, const void* src, const uint8_t* src_mask, uint64_t cols, uint64_t rows, uint32_t rx, uint32_t ry,
                     uint32_t op, uint32_t flags, void* dst, uint8_t* dst_mask, const ecf::Layout& lds, const ecf::Grid& g, FocalArgs* a, bool* done) {
    *done = true;
    if (!ecl::valid(t)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "%s: bad dtype %d", what, int(t));
    if (g.tiles == 0) return EC_OK;  // an empty raster
    const ec_status st = ensure_ready();
    if (st != EC_OK) return st;
    *done = false;
    *a = FocalArgs{src, dst, src_mask, dst_mask, cols, rows, uint32_t(g.tiles_x), rx, ry, op, flags, 0u, 0u, lds};
    const size_t bytes[2] = {size_t(cols * rows) * ecl::size_of(t), src_mask ? size_t(cols * rows) : 0};  // the streams that are loaded
    a->cacheable = cache_plan(bytes, 2);
    // a slot starts TW-aligned in its row, so every slot of the values and of the mask bytes is 16-byte aligned when the pointers
    // are and a row is a multiple of 16 cells
    const bool aligned = reinterpret_cast<uintptr_t>(dst) % 16 == 0 && reinterpret_cast<uintptr_t>(dst_mask) % 16 == 0 && cols % 16 == 0;
    a->cellwise_stores = !(tuning().unaligned_vector || aligned);
    return EC_OK;
}

template <typename T, int KIND>
static ec_status launch_focal(FocalArgs a, uint64_t tiles, hipStream_t s) {
    return split_launch(tiles, KIND == ecf::kSeparableSum ? "focal(sum)" : "focal(min_max)", [&](size_t first, unsigned grid) {
        a.first_tile = uint32_t(first);  // tiles <= 2^31 - 1 (ecf::refusal)
        if (a.src_mask) k_focal<T, true, KIND><<<grid, kBlock, a.lds.bytes, s>>>(a);
        else k_focal<T, false, KIND><<<grid, kBlock, a.lds.bytes, s>>>(a);
    });
}

template <typename T>
static ec_status launch_convolve(FocalArgs a, const FocalWeights& w, uint64_t tiles, hipStream_t s) {
    return split_launch(tiles, "focal(convolve)", [&](size_t first, unsigned grid) {
        a.first_tile = uint32_t(first);
        if (a.src_mask) k_focal_convolve<T, true><<<grid, kBlock, a.lds.bytes, s>>>(a, w);
        else k_focal_convolve<T, false><<<grid, kBlock, a.lds.bytes, s>>>(a, w);
    });
}

}  // namespace ecd

using namespace ecd;

extern "C" ec_dtype ec_focal_result_type(int32_t op, ec_dtype t) {
    if (op < EC_FOCAL_SUM || op > EC_FOCAL_MAX || !ecl::valid(t)) return 255;
    return op == EC_FOCAL_SUM || op == EC_FOCAL_MEAN ? ec_dtype(EC_F64) : t;
}

extern "C" ec_status ec_focal(int32_t op, ec_dtype t, const void* src, const uint8_t* src_mask_or_null, uint64_t cols, uint64_t rows, uint32_t rx,
                              uint32_t ry, uint32_t flags, void* dst, uint8_t* dst_mask_or_null, ec_stream stream) {
    ecf::Grid g;
    if (const char* why = ecf::refusal(false, op, src, dst, nullptr, src_mask_or_null, dst_mask_or_null, cols, rows, rx, ry, flags, TW, TH, &g))
        return set_error(EC_ERR_ARG, "ec_focal: %s", why);
    const bool sum = op == EC_FOCAL_SUM || op == EC_FOCAL_MEAN;
    FocalArgs a;
    bool done;
    const ecf::Layout lds = ecf::layout_of(uint32_t(ecl::size_of(t)), src_mask_or_null != nullptr, sum ? ecf::kSeparableSum : ecf::kSeparableMinMax, rx, ry, TW, TH);
    const ec_status st = focal_args("ec_focal", t, src, src_mask_or_null, cols, rows, rx, ry, uint32_t(op), flags, dst, dst_mask_or_null, lds, g, &a, &done);
    if (done) return st;
    return ecl::with_cell_type(t, [&](auto c) {
        using T = ecl::cell_t<decltype(c)>;
        return sum ? launch_focal<T, ecf::kSeparableSum>(a, g.tiles, S(stream)) : launch_focal<T, ecf::kSeparableMinMax>(a, g.tiles, S(stream));
    }, kTypeChecked);
}

extern "C" ec_status ec_focal_convolve(ec_dtype t, const void* src, const uint8_t* src_mask_or_null, uint64_t cols, uint64_t rows,
                                       const double* weights_host, uint32_t rx, uint32_t ry, uint32_t flags, void* dst, uint8_t* dst_mask_or_null,
                                       ec_stream stream) {
    ecf::Grid g;
    if (const char* why = ecf::refusal(true, 0, src, dst, weights_host, src_mask_or_null, dst_mask_or_null, cols, rows, rx, ry, flags, TW, TH, &g))
        return set_error(EC_ERR_ARG, "ec_focal_convolve: %s", why);
    FocalArgs a;
    bool done;
    const ecf::Layout lds = ecf::layout_of(uint32_t(ecl::size_of(t)), src_mask_or_null != nullptr, ecf::kConvolve, rx, ry, TW, TH);
    const ec_status st = focal_args("ec_focal_convolve", t, src, src_mask_or_null, cols, rows, rx, ry, 0u, flags, dst, dst_mask_or_null, lds, g, &a, &done);
    if (done) return st;
    FocalWeights w;
    memset(&w, 0, sizeof w);
    memcpy(w.w, weights_host, sizeof(double) * (2 * rx + 1) * (2 * ry + 1));  // read now: the caller's array may go when the call returns
    return ecl::with_cell_type(t, [&](auto c) { return launch_convolve<ecl::cell_t<decltype(c)>>(a, w, g.tiles, S(stream)); }, kTypeChecked);
}
