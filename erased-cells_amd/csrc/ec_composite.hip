// ec_composite.hip — ec_composite (include/erased_cells.h): one raster from a stack of K co-registered layers, per cell the first
// or last valid layer, the least or greatest valid cell, or the sum or mean of the valid cells.  The refusals (the stack's are ecs::*_refusal,
// ec_stack_plan.hpp; all before any device work and before the library asks for a device) and the launches of k_composite / k_composite_cellwise
// (ec_composite_kernels.hpp).  A translation unit of its own, as the moving windows have: its kernels (FIRST and LAST by cell
// width, MIN, MAX and SUM by cell type, each as a tile kernel and a cell-wise one) compile beside the others.
#include <hip/hip_runtime.h>

#include "ec_composite_kernels.hpp"
#include "ec_dispatch.hpp"
#include "ec_runtime.hpp"

namespace ecd {

// groups per tile and cells per group of the kernel that serves (op, cell width): what the tile count is checked against
static void composite_tile_shape(int op, size_t width, size_t* cpl, size_t* u) {
    *cpl = 16 / (composite_sums(op) ? sizeof(double) : width);
    *u = size_t(composite_u(composite_sums(op), width));
}

template <typename T, int OP>
static ec_status launch_composite(const CompositeArgs& a, hipStream_t s) {
    using S = CompositeShape<T, OP>;
    constexpr size_t CPL = S::CPL;
    if (tuning().unaligned_vector || ecs::stack_aligned(a, CPL, sizeof(T), sizeof(typename S::R))) {
        const size_t groups = a.n / CPL, tile = size_t(kBlock) * S::U;
        return split_launch((groups + tile - 1) / tile, "composite", [&](size_t first, unsigned grid) { k_composite<T, OP><<<grid, kBlock, 0, s>>>(a, first); });
    }
    k_composite_cellwise<T, OP><<<grid_capped((a.n + kBlock - 1) / kBlock, 8), kBlock, 0, s>>>(a);
    return check_launch("composite");
}

// FIRST and LAST move cells: typed by width.  MIN, MAX and SUM (MEAN is SUM with a flag) read them: typed by cell type.
static ec_status dispatch_composite(int op, int t, const CompositeArgs& a, hipStream_t s) {
    if (op == kCompositeFirst || op == kCompositeLast)
        return ecl::with_cell_width(ecl::size_of(t), [&](auto w) {
            using W = ecl::cell_t<decltype(w)>;
            return op == kCompositeFirst ? launch_composite<W, kCompositeFirst>(a, s) : launch_composite<W, kCompositeLast>(a, s);
        }, kTypeChecked);
    return ecl::with_cell_type(t, [&](auto c) {
        using T = ecl::cell_t<decltype(c)>;
        if (op == kCompositeMin) return launch_composite<T, kCompositeMin>(a, s);
        if (op == kCompositeMax) return launch_composite<T, kCompositeMax>(a, s);
        return launch_composite<T, kCompositeSum>(a, s);
    }, kTypeChecked);
}

}  // namespace ecd

using namespace ecd;

extern "C" ec_dtype ec_composite_result_type(int32_t op, ec_dtype t) {
    if (!valid_composite_op(op) || !ecl::valid(t)) return 255;
    return composite_sums(op) ? ec_dtype(EC_F64) : t;
}

extern "C" ec_status ec_composite(int32_t op, ec_dtype t, const void* const* layers, const uint8_t* const* masks_or_null, int32_t n_layers, size_t n,
                                  uint32_t min_count, void* dst, uint8_t* dst_mask_or_null, uint8_t* aux_or_null, ec_stream stream) {
    if (!valid_composite_op(op)) return set_error(EC_ERR_ARG, "ec_composite: operation %d is not an ec_composite_op (0..5)", int(op));
    ecs::Message why;
    if (ecs::count_refusal(why, "ec_composite", n_layers) || ecs::min_count_refusal(why, "ec_composite", min_count, n_layers))
        return set_error(EC_ERR_ARG, "%s", why);
    if (!ecl::valid(t)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_composite: bad dtype %d", int(t));
    if (n == 0) return EC_OK;
    size_t cpl, u;
    composite_tile_shape(op, ecl::size_of(t), &cpl, &u);
    const size_t tiles = (n / cpl + size_t(kBlock) * u - 1) / (size_t(kBlock) * u);
    if (ecs::pointer_refusal(why, "ec_composite", layers, masks_or_null, n_layers, n, tiles, dst, dst_mask_or_null, aux_or_null))
        return set_error(EC_ERR_ARG, "%s", why);
    const ec_status st = ensure_ready();
    if (st != EC_OK) return st;
    CompositeArgs a;
    ecs::fill(&a, layers, masks_or_null, n_layers, n, min_count, dst, dst_mask_or_null, aux_or_null);
    a.mean = op == kCompositeMean;
    return dispatch_composite(op, t, a, S(stream));
}
