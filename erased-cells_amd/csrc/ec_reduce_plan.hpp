// ec_reduce_plan.hpp — what the host decides for one launch of a reduction (ec_reduce_kernels.hpp), in plain C++: nothing from
// HIP or from this library, so that host/test_reduce_plan.cpp can hold it against the launchers' formulas it replaced.
//
// The launchers — launch_reduction (ec_reduce_launch.hpp) for min/max and the band statistics, first_diff_w and
// ec_mask_counts_device (ec_abi.hip) — pass what they know — where the streams start, the cell size and count, the launch
// shape, the device's CU count, the knobs, the load policy of cache_plan() — and keep what is theirs: the kernel per shape, the
// residency probe, the one-launch rule of the counts, the finalize launch.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace ecd {

constexpr int kReduceU = 8;   // 16-byte loads in flight per lane of a reduction tile (ec_reduce_kernels.hpp)
constexpr int kMaxReduceBlocks = 4096;  // the finalize kernels read no more partials

// A launch shape: the vector kernel, and the cell-wise kernel that serves pointers the vector kernel may not take.
struct ReduceShape {
    int block, u;   // threads per workgroup, 16-byte loads in flight per lane
    int per_cu;     // workgroups per CU: as many as are resident at once, so the grid runs as ONE round
    int cellwise_block, cellwise_per_cu;
};

struct ReducePlan {
    bool aligned;          // the vector kernel runs (false: the cell-wise one)
    unsigned head;         // leading cells peeled by workgroup 0
    unsigned grid;         // workgroups; 0 = nothing to scan (n == 0)
    unsigned head_policy;  // head | load policy << 8, the kernels' `head` argument
    bool single;           // one workgroup: its fold is the result, a kernel that can write it itself skips the finalize launch
};

// Workgroups a reduction launches at most: `per_cu` per CU unless the "reduce_bpc" knob (> 0) overrides it; never more than
// the finalize kernels read.
inline size_t reduce_cap(int cus, int per_cu, int reduce_bpc) {
    const long cap = long(cus) * (reduce_bpc > 0 ? reduce_bpc : per_cu);
    return static_cast<size_t>(cap < kMaxReduceBlocks ? cap : kMaxReduceBlocks);
}

// Leading cells a reduction peels so that its 16-byte loads start 16-byte aligned (0 when the window is shorter).
// `residue` = the first cell's address mod 16.
inline unsigned reduce_head(unsigned residue, size_t cell_size, size_t n, bool unaligned_vector) {
    if (!unaligned_vector) return 0;
    const size_t h = ((16 - residue) % 16) / cell_size;
    return h <= n ? static_cast<unsigned>(h) : 0u;
}

// residue0: stream 0's first cell mod 16; residue1: the second stream's (mask, other buffer) start mod the alignment the vector
// kernel wants of it, 0 without one.  The vector kernels' loads are declared under-aligned (ec_device.hpp), so any residue
// will do unless the "unaligned_vector" knob is off.  `policy`: cache_plan()'s bits for the launch's streams.
inline ReducePlan reduce_plan(unsigned residue0, unsigned residue1, size_t cell_size, size_t n, const ReduceShape& shape, int cus,
                              int reduce_bpc, bool unaligned_vector, unsigned policy) {
    ReducePlan pl{};
    pl.aligned = unaligned_vector || (residue0 == 0 && residue1 == 0);
    if (n == 0) return pl;
    pl.head = pl.aligned ? reduce_head(residue0, cell_size, n, unaligned_vector) : 0u;
    // what one workgroup takes per round: a tile of 16-byte groups, or one cell per thread
    const size_t work = pl.aligned ? (n - pl.head) / (16 / cell_size) : n;
    const size_t per_round = pl.aligned ? size_t(shape.block) * size_t(shape.u) : size_t(shape.cellwise_block);
    size_t tiles = (work + per_round - 1) / per_round;
    if (tiles < 1) tiles = 1;
    const size_t cap = reduce_cap(cus, pl.aligned ? shape.per_cu : shape.cellwise_per_cu, reduce_bpc);
    pl.grid = static_cast<unsigned>(tiles < cap ? tiles : cap);
    pl.head_policy = pl.head | (policy << 8);
    pl.single = pl.grid == 1;
    return pl;
}

}  // namespace ecd
