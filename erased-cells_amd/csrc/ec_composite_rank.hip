// ec_composite_rank.hip — ec_composite_rank (include/erased_cells.h): one raster from a stack of K co-registered layers, per cell
// the valid layer at position r(count) of the ascending order of (order_key(cell), k): the median and the other quantiles.  The
// refusals (before any device work and before the library asks for a device) and the table r(c).  The kernels
// (ec_composite_rank_kernels.hpp: by cell type and by bucket, the stack's height rounded up to a power of two; each as a tile
// kernel and a cell-wise one) and their launches are in ec_composite_rank_c{1,2,4,8}.hip, one translation unit per cell width.
#include <hip/hip_runtime.h>

#include <cstring>

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
    if (n_layers < 1 || n_layers > kCompositeMaxLayers)
        return set_error(EC_ERR_ARG, "ec_composite_rank: %d layers, not within 1 .. EC_COMPOSITE_MAX_LAYERS (%d)", int(n_layers), kCompositeMaxLayers);
    if (!valid_rank_fraction(num, den))
        return set_error(EC_ERR_ARG, "ec_composite_rank: q = %u / %u needs 1 <= den <= EC_RANK_MAX_DEN (%u) and num <= den", num, den, kRankMaxDen);
    if (!valid_rank_method(method)) return set_error(EC_ERR_ARG, "ec_composite_rank: method %d is not an ec_rank_method (0..1)", int(method));
    if (min_count < 1 || min_count > uint32_t(n_layers))
        return set_error(EC_ERR_ARG, "ec_composite_rank: min_count %u is not within 1 .. %d, the number of layers", min_count, int(n_layers));
    if (!ecl::valid(t)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_composite_rank: bad dtype %d", int(t));
    if (n == 0) return EC_OK;
    if (!layers || !dst) return set_error(EC_ERR_ARG, "ec_composite_rank: null pointer");
    bool masked = false;
    for (int k = 0; k < n_layers; ++k) {
        if (!layers[k]) return set_error(EC_ERR_ARG, "ec_composite_rank: layer %d is a null pointer", k);
        masked = masked || (masks_or_null && masks_or_null[k]);
    }
    if (masked && !dst_mask_or_null) return set_error(EC_ERR_ARG, "ec_composite_rank: a layer has a mask, so the result needs dst_mask");
    const size_t g = size_t(rank_group(ecl::size_of(t), rank_bucket(n_layers)));
    if ((n / g + (n % g != 0) + size_t(kBlock) - 1) / size_t(kBlock) > size_t(0x7fffffff))  // groups, the partial last one among them
        return set_error(EC_ERR_ARG, "ec_composite_rank: %zu cells are more than 2^31 - 1 tiles", n);
    for (int k = 0; k < n_layers; ++k)
        if (layers[k] == dst) return set_error(EC_ERR_ARG, "ec_composite_rank: dst is layer %d (the operation is not in-place)", k);
    for (int k = 0; k < n_layers; ++k) {
        const uint8_t* m = masks_or_null ? masks_or_null[k] : nullptr;
        if (m && (m == dst_mask_or_null || m == aux_or_null)) return set_error(EC_ERR_ARG, "ec_composite_rank: dst_mask or aux is the mask of layer %d", k);
    }
    if (dst_mask_or_null && dst_mask_or_null == dst) return set_error(EC_ERR_ARG, "ec_composite_rank: dst_mask is dst");
    if (aux_or_null && (aux_or_null == dst || aux_or_null == dst_mask_or_null)) return set_error(EC_ERR_ARG, "ec_composite_rank: aux is dst or dst_mask");
    const ec_status st = ensure_ready();
    if (st != EC_OK) return st;
    CompositeRankArgs a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < n_layers; ++k) {  // read now: the caller's arrays may go when the call returns
        a.p[k] = layers[k];
        a.m[k] = masks_or_null ? masks_or_null[k] : nullptr;
    }
    a.dst = dst;
    a.dst_mask = dst_mask_or_null;
    a.aux = aux_or_null;
    a.n = n;
    a.layers = n_layers;
    a.min_count = min_count;
    a.rank = rank_table(num, den, method);  // once per call: no lane divides
    return dispatch_composite_rank(t, a, S(stream));
}
