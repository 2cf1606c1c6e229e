// ec_composite_rank_tu.hpp — the body of ec_composite_rank_c{1,2,4,8}.hip: the kernels of ec_composite_rank_kernels.hpp for the cell
// types of EC_RANK_WIDTH bytes, every bucket, and their launches.  One translation unit per cell width, as the fused kernels have
// (ec_fused_any_tu.hpp): the 64-wire networks are the slowest code of the library to compile ("Order statistics of a stack"), and four units compile
// side by side.
#include <hip/hip_runtime.h>

#include "ec_composite_rank_kernels.hpp"
#include "ec_dispatch.hpp"
#include "ec_runtime.hpp"

#ifndef EC_RANK_WIDTH
#error "define EC_RANK_WIDTH (1, 2, 4 or 8) before including ec_composite_rank_tu.hpp"
#endif
#define EC_RANK_PASTE2(a, b) a##b
#define EC_RANK_PASTE(a, b) EC_RANK_PASTE2(a, b)

namespace ecd {

template <typename T, int KB>
static ec_status launch_composite_rank(const CompositeRankArgs& a, hipStream_t s) {
    constexpr size_t G = rank_group(sizeof(T), KB);
    if constexpr (G > 1) {  // a group of one cell is aligned wherever a cell is: those buckets have no cell-wise kernel
        if (!(tuning().unaligned_vector || ecs::stack_aligned(a, G, sizeof(T), sizeof(T)))) {
            k_composite_rank_cellwise<T, KB><<<grid_capped((a.n + kBlock - 1) / kBlock, 8), kBlock, 0, s>>>(a);
            return check_launch("composite_rank");
        }
    }
    const size_t groups = (a.n + G - 1) / G;  // the last one may be partial: it is guarded in the kernel
    return split_launch((groups + kBlock - 1) / kBlock, "composite_rank", [&](size_t first, unsigned grid) { k_composite_rank<T, KB><<<grid, kBlock, 0, s>>>(a, first); });
}

// composite_rank_c1 / _c2 / _c4 / _c8 (declared in ec_composite_rank.hip): the launch for a cell type of this width
ec_status EC_RANK_PASTE(composite_rank_c, EC_RANK_WIDTH)(int t, const CompositeRankArgs& a, hipStream_t s) {
    return ecl::with_cell_type(t, [&](auto c) -> ec_status {
        using T = ecl::cell_t<decltype(c)>;
        if constexpr (sizeof(T) == EC_RANK_WIDTH) {
            switch (rank_bucket(a.layers)) {
                case 1: return launch_composite_rank<T, 1>(a, s);
                case 2: return launch_composite_rank<T, 2>(a, s);
                case 4: return launch_composite_rank<T, 4>(a, s);
                case 8: return launch_composite_rank<T, 8>(a, s);
                case 16: return launch_composite_rank<T, 16>(a, s);
                case 32: return launch_composite_rank<T, 32>(a, s);
                default: return launch_composite_rank<T, 64>(a, s);
            }
        } else {
            return kTypeChecked;
        }
    }, kTypeChecked);
}

}  // namespace ecd
