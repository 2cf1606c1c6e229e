// ec_focal_rank_tu.hpp — the body of ec_focal_rank_c{1,2,4,8}.hip: k_focal_rank (ec_focal_rank_kernels.hpp) for the cell types of
// EC_FOCAL_RANK_WIDTH bytes, every bucket a footprint can have, and their launches.  One translation unit per cell width, as
// ec_composite_rank_tu.hpp has and for its reason: the 64-wire networks compile slowly, and four units compile side by side.
#include <hip/hip_runtime.h>

#include "ec_dispatch.hpp"
#include "ec_focal_rank_kernels.hpp"
#include "ec_runtime.hpp"

#ifndef EC_FOCAL_RANK_WIDTH
#error "define EC_FOCAL_RANK_WIDTH (1, 2, 4 or 8) before including ec_focal_rank_tu.hpp"
#endif
#define EC_FOCAL_RANK_PASTE2(a, b) a##b
#define EC_FOCAL_RANK_PASTE(a, b) EC_FOCAL_RANK_PASTE2(a, b)

namespace ecd {

template <typename T, int KB>
static ec_status launch_focal_rank(FocalArgs a, const RankTable& r, uint64_t tiles, hipStream_t s) {
    return split_launch(tiles, a.op == kFocalRankPick ? "focal_rank" : "focal_majority", [&](size_t first, unsigned grid) {
        a.first_tile = uint32_t(first);  // tiles <= 2^31 - 1 (ecf::rank_refusal)
        k_focal_rank<T, KB><<<grid, kBlock, a.lds.bytes, s>>>(a, r);
    });
}

// focal_rank_c1 / _c2 / _c4 / _c8 (declared in ec_focal_rank.hip): the launch for a cell type of this width
ec_status EC_FOCAL_RANK_PASTE(focal_rank_c, EC_FOCAL_RANK_WIDTH)(int t, const FocalArgs& a, const RankTable& r, uint64_t tiles, hipStream_t s) {
    return ecl::with_cell_type(t, [&](auto c) -> ec_status {
        using T = ecl::cell_t<decltype(c)>;
        if constexpr (sizeof(T) == EC_FOCAL_RANK_WIDTH) {
            switch (focal_rank_bucket((2 * a.rx + 1) * (2 * a.ry + 1))) {  // an odd number of taps: never 2
                case 1: return launch_focal_rank<T, 1>(a, r, tiles, s);
                case 4: return launch_focal_rank<T, 4>(a, r, tiles, s);
                case 8: return launch_focal_rank<T, 8>(a, r, tiles, s);
                case 16: return launch_focal_rank<T, 16>(a, r, tiles, s);
                case 32: return launch_focal_rank<T, 32>(a, r, tiles, s);
                default: return launch_focal_rank<T, 64>(a, r, tiles, s);
            }
        } else {
            return kTypeChecked;
        }
    }, kTypeChecked);
}

}  // namespace ecd
