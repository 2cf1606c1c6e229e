// ec_composite_rank.hip — ec_composite_rank (include/erased_cells.h): one raster from a stack of K co-registered layers, per cell
// the valid layer at position r(count) of the ascending order of (order_key(cell), k): the median and the other quantiles.  The
// refusals (the stack's are ecs::*_refusal, ec_stack_plan.hpp; all before any device work and before the library asks for a device)
// and the table r(c).  The kernels
// (ec_composite_rank_kernels.hpp: by cell type and by bucket, the stack's height rounded up to a power of two; each as a tile
// kernel and a cell-wise one) and their launches are in ec_composite_rank_c{1,2,4,8}.hip, one translation unit per cell width.
#include <hip/hip_runtime.h>

#include "ec_composite_rank_kernels.hpp"
#include "ec_dispatch.hpp"
#include "ec_runtime.hpp"

namespace ecd {

// the launches live in ec_composite_rank_c{1,2,4,8}.hip (ec_composite_rank_tu.hpp), by cell width
ec_status composite_rank_c1(int t, const CompositeRankArgs& a, hipStream_t s);
ec_status composite_rank_c2(int t, const CompositeRankArgs& a, hipStream_t s);
ec_status composite_rank_c4(int t, const CompositeRankArgs& a, hipStream_t s);
ec_status composite_rank_c8(int t, const CompositeRankArgs& a, hipStream_t s);

static ec_status dispatch_composite_rank(int t, const CompositeRankArgs& a, hipStream_t s) {
    switch (ecl::size_of(t)) {
        case 1: return composite_rank_c1(t, a, s);
        case 2: return composite_rank_c2(t, a, s);
        case 4: return composite_rank_c4(t, a, s);
        default: return composite_rank_c8(t, a, s);
    }
}

}  // namespace ecd

using namespace ecd;

extern "C" ec_status ec_composite_rank(ec_dtype t, const void* const* layers, const uint8_t* const* masks_or_null, int32_t n_layers, size_t n,
                                       uint32_t num, uint32_t den, int32_t method, uint32_t min_count, void* dst, uint8_t* dst_mask_or_null,
                                       uint8_t* aux_or_null, ec_stream stream) {
    ecs::Message why;
    if (ecs::count_refusal(why, "ec_composite_rank", n_layers)) return set_error(EC_ERR_ARG, "%s", why);
    if (!valid_rank_fraction(num, den))
        return set_error(EC_ERR_ARG, "ec_composite_rank: q = %u / %u needs 1 <= den <= EC_RANK_MAX_DEN (%u) and num <= den", num, den, kRankMaxDen);
    if (!valid_rank_method(method)) return set_error(EC_ERR_ARG, "ec_composite_rank: method %d is not an ec_rank_method (0..1)", int(method));
    if (ecs::min_count_refusal(why, "ec_composite_rank", min_count, n_layers)) return set_error(EC_ERR_ARG, "%s", why);
    if (!ecl::valid(t)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_composite_rank: bad dtype %d", int(t));
    if (n == 0) return EC_OK;
    const size_t g = size_t(rank_group(ecl::size_of(t), rank_bucket(n_layers)));
    const size_t tiles = (n / g + (n % g != 0) + size_t(kBlock) - 1) / size_t(kBlock);  // groups, the partial last one among them
    if (ecs::pointer_refusal(why, "ec_composite_rank", layers, masks_or_null, n_layers, n, tiles, dst, dst_mask_or_null, aux_or_null))
        return set_error(EC_ERR_ARG, "%s", why);
    const ec_status st = ensure_ready();
    if (st != EC_OK) return st;
    CompositeRankArgs a;
    ecs::fill(&a, layers, masks_or_null, n_layers, n, min_count, dst, dst_mask_or_null, aux_or_null);
    a.rank = rank_table(num, den, method);  // once per call: no lane divides
    return dispatch_composite_rank(t, a, S(stream));
}
