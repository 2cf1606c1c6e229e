// ec_focal_rank.hip — ec_focal_rank and ec_focal_majority (include/erased_cells.h): the median, the other quantiles and the mode of
// a moving window.  The refusals (ecf::rank_refusal, ec_focal_plan.hpp: before any device work and before the library asks for a
// device), the table r(c) and the launch arguments.  The kernels (ec_focal_rank_kernels.hpp: by cell type and by bucket, the
// footprint's size rounded up to a power of two) and their launches are in ec_focal_rank_c{1,2,4,8}.hip, one translation unit per
// cell width.
#include <hip/hip_runtime.h>

#include "ec_dispatch.hpp"
#include "ec_focal_rank_kernels.hpp"
#include "ec_runtime.hpp"

namespace ecd {

// the launches live in ec_focal_rank_c{1,2,4,8}.hip (ec_focal_rank_tu.hpp), by cell width
ec_status focal_rank_c1(int t, const FocalArgs& a, const RankTable& r, uint64_t tiles, hipStream_t s);
ec_status focal_rank_c2(int t, const FocalArgs& a, const RankTable& r, uint64_t tiles, hipStream_t s);
ec_status focal_rank_c4(int t, const FocalArgs& a, const RankTable& r, uint64_t tiles, hipStream_t s);
ec_status focal_rank_c8(int t, const FocalArgs& a, const RankTable& r, uint64_t tiles, hipStream_t s);

// both entry points behind their refusals: the launch arguments (focal_args, ec_focal.hip), then the launch
static ec_status focal_rank_run(const char* what, uint32_t op, ec_dtype t, const void* src, const uint8_t* src_mask, uint64_t cols, uint64_t rows,
                                uint32_t rx, uint32_t ry, const RankTable& rank, uint32_t flags, void* dst, uint8_t* dst_mask, const ecf::Grid& g,
                                hipStream_t s) {
    const size_t W = ecl::size_of(t);
    FocalArgs a;
    bool done;
    const ec_status st = focal_args(what, t, src, src_mask, cols, rows, rx, ry, op, flags, dst, dst_mask,
                                    ecf::rank_layout_of(uint32_t(W), src_mask != nullptr, rx, ry, TW, TH), g, &a, &done);
    if (done) return st;
    switch (W) {
        case 1: return focal_rank_c1(t, a, rank, g.tiles, s);
        case 2: return focal_rank_c2(t, a, rank, g.tiles, s);
        case 4: return focal_rank_c4(t, a, rank, g.tiles, s);
        default: return focal_rank_c8(t, a, rank, g.tiles, s);
    }
}

}  // namespace ecd

using namespace ecd;

extern "C" ec_status ec_focal_rank(ec_dtype t, const void* src, const uint8_t* src_mask_or_null, uint64_t cols, uint64_t rows, uint32_t rx,
                                   uint32_t ry, uint32_t num, uint32_t den, int32_t method, uint32_t flags, void* dst, uint8_t* dst_mask_or_null,
                                   ec_stream stream) {
    ecf::Grid g;
    if (const char* why = ecf::rank_refusal(true, src, dst, src_mask_or_null, dst_mask_or_null, cols, rows, rx, ry, num, den, method, flags, TW, TH, &g))
        return set_error(EC_ERR_ARG, "ec_focal_rank: %s", why);
    return focal_rank_run("ec_focal_rank", kFocalRankPick, t, src, src_mask_or_null, cols, rows, rx, ry, rank_table(num, den, method), flags, dst,
                          dst_mask_or_null, g, S(stream));  // r(c) once per call: no lane divides
}

extern "C" ec_status ec_focal_majority(ec_dtype t, const void* src, const uint8_t* src_mask_or_null, uint64_t cols, uint64_t rows, uint32_t rx,
                                       uint32_t ry, uint32_t flags, void* dst, uint8_t* dst_mask_or_null, ec_stream stream) {
    ecf::Grid g;
    if (const char* why = ecf::rank_refusal(false, src, dst, src_mask_or_null, dst_mask_or_null, cols, rows, rx, ry, 0, 1, 0, flags, TW, TH, &g))
        return set_error(EC_ERR_ARG, "ec_focal_majority: %s", why);
    return focal_rank_run("ec_focal_majority", kFocalRankMajority, t, src, src_mask_or_null, cols, rows, rx, ry, rank_table(0, 1, kRankLower), flags,
                          dst, dst_mask_or_null, g, S(stream));
}
