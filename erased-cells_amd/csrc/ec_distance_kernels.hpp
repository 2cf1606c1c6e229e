// ec_distance_kernels.hpp — the two gfx950 kernels of ec_distance (include/erased_cells.h) around the line scans of
// ec_distance_line.hpp.  One wave per workgroup in both: a lane owns a line, and the only exchange between lanes is the
// transposition of a tile through LDS.
//
//   k_distance_columns   lane l of workgroup b owns column b * kDistLines + l.  Adjacent lanes own adjacent columns, so the mask
//                        bytes a wave loads for a row and the g cells it stores are consecutive: 64 and 128 bytes a row.
//   k_distance_rows      lane l of workgroup b owns row b * kDistLines + l.  g comes in and the results go out as tiles of
//                        kDistLines rows by kDistTile columns: the wave reads and writes them row by row (lanes along a row:
//                        coalesced), a lane walks its own row of the tile in LDS.  The pitches (ec_distance_line.hpp) keep the
//                        column-wise LDS accesses on distinct banks.  No lane issues a global access with a stride of cols cells
//                        but the single g cell a pop looks up.  max_sq, the square root and the mask byte are applied where the
//                        result tile is written.
//
// No atomics, no inline assembly, no private memory: the chunk arrays of the column sweeps are unrolled into registers.
#pragma once

#include <hip/hip_runtime.h>

#include "ec_distance_line.hpp"

namespace ecd {

__global__ __launch_bounds__(kDistLines) void k_distance_columns(const uint8_t* __restrict__ mask, uint32_t cols, uint32_t rows,
                                                                  uint16_t* __restrict__ g) {
    const uint32_t x = blockIdx.x * uint32_t(kDistLines) + threadIdx.x;
    if (x >= cols) return;
    distance_column_down(mask + x, cols, rows, g + x, cols);
    distance_column_up(g + x, cols, rows);
}

// OUT: uint32_t (d2) or double (its square root); VALUES / MASKOUT: dst / dst_mask is given
template <typename OUT, bool VALUES, bool MASKOUT>
__global__ __launch_bounds__(kDistLines) void k_distance_rows(const uint16_t* __restrict__ g, uint32_t cols, uint32_t rows, uint32_t max_sq,
                                                               uint16_t* __restrict__ stack_s, uint16_t* __restrict__ stack_t,
                                                               OUT* __restrict__ dst, uint8_t* __restrict__ dst_mask) {
    __shared__ uint16_t tile_g[kDistLines * kDistGPitch];
    __shared__ uint32_t tile_d[kDistLines * kDistDPitch];
    const uint32_t lane = threadIdx.x;
    const uint32_t y0 = blockIdx.x * uint32_t(kDistLines);
    const uint32_t y = y0 + lane;
    const bool owns = y < rows;
    const uint32_t tile_rows = rows - y0 < uint32_t(kDistLines) ? rows - y0 : uint32_t(kDistLines);
    const size_t wave_stack = size_t(blockIdx.x) * size_t(kDistLines) * size_t(cols) + lane;
    uint16_t* S = stack_s + wave_stack;
    uint16_t* T = stack_t + wave_stack;
    const uint16_t* grow = g + size_t(owns ? y : y0) * cols;  // this lane's row of g: what a pop looks g(s) up in
    const uint32_t tiles = (cols + uint32_t(kDistTile) - 1) / uint32_t(kDistTile);
    DistEnvelope e;

    for (uint32_t tx = 0; tx < tiles; ++tx) {
        const uint32_t x0 = tx * uint32_t(kDistTile);
        const uint32_t n = cols - x0 < uint32_t(kDistTile) ? cols - x0 : uint32_t(kDistTile);
        if (lane < n) {
#pragma unroll 8
            for (uint32_t r = 0; r < tile_rows; ++r) tile_g[r * kDistGPitch + lane] = g[size_t(y0 + r) * cols + x0 + lane];
        }
        __syncthreads();
        if (owns) distance_row_forward(e, tile_g + lane * kDistGPitch, 1, x0, n, cols, S, T, kDistLines, grow, 1);
        __syncthreads();
    }

    for (uint32_t tx = tiles; tx-- > 0;) {
        const uint32_t x0 = tx * uint32_t(kDistTile);
        const uint32_t n = cols - x0 < uint32_t(kDistTile) ? cols - x0 : uint32_t(kDistTile);
        if (owns) distance_row_backward(e, x0, n, tile_d + lane * kDistDPitch, 1, S, T, kDistLines, grow, 1);
        __syncthreads();
        if (lane < n) {
            for (uint32_t r = 0; r < tile_rows; ++r) {
                const uint32_t d2 = tile_d[r * kDistDPitch + lane];
                const bool ok = dist_valid(d2, max_sq);
                const size_t at = size_t(y0 + r) * cols + x0 + lane;
                if constexpr (VALUES) {
                    if constexpr (sizeof(OUT) == 8) dst[at] = ok ? __dsqrt_rn(double(d2)) : 0.0;
                    else dst[at] = ok ? d2 : 0u;
                }
                if constexpr (MASKOUT) dst_mask[at] = ok ? uint8_t(1) : uint8_t(0);
            }
        }
        __syncthreads();
    }
}

}  // namespace ecd
