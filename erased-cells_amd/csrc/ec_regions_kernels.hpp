// ec_regions_kernels.hpp — the gfx950 kernels of ec_regions (include/erased_cells.h) around the per-cell functions of
// ec_regions_cell.hpp.  The phases are separated by kernel boundaries; only k_regions_seams has workgroups meet.
//
//   k_regions_tiles<W>    one workgroup per tile of kRegTileW x kRegTileH cells: a union-find over the tile in LDS (workgroup-scope
//                         atomics on a u32 per cell), then parent[i] = the global index of the tile-local root; count[i] = 0.
//   k_regions_seams<W>    one wave per tile, a lane per cell of the tile's last row and last column: reg_seam_unite.  EVERY access
//                         to parent[] here is an agent-scope __hip_atomic_* (a relaxed load, a fetch_min): the XCDs' L2s and the
//                         CUs' L1s are not coherent within a launch, and reg_unite needs nothing of a load but that it returns a
//                         value parent[i] once had (a relaxed load, a fetch_min — the path compression of reg_find is one too).  No wait, flag or ticket
//                         between workgroups.
//   k_regions_flatten     parent[i] = the root, with plain loads (a new launch: the seams' atomics are in memory).  A lane stores
//                         only its own entry, and the root it stores is where every chain through i ends anyway, so a lane that
//                         reads the entry sees the old value or the new and reaches the same root.  With a sieve the sizes are
//                         counted at count[root], one add per run of equal roots in a wave.
//   k_regions_sums        per block of kRegScanCells cells, the number of kept roots.
//   k_regions_scan        ONE workgroup: the exclusive scan of the block sums in place; K by one store.
//   k_regions_number      dense numbering: count[root] = its number for a kept root, 0 for a dropped one.
//   k_regions_store       labels (write-through, st_cell / nt_store) and mask bytes (mask_store), four cells a lane.
//
// Reduce-then-scan in three launches, no single-pass look-back: no workgroup ever waits for another.  No inline assembly but the
// library's value store, no private memory.
#pragma once

#include <hip/hip_runtime.h>

#include "ec_device.hpp"
#include "ec_regions_cell.hpp"

namespace ecd {

struct RegLdsWords {  // the tile's union-find: workgroup scope is all an LDS word needs
    uint32_t* w;
    __device__ __forceinline__ uint32_t load(uint32_t i) { return __hip_atomic_load(w + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ uint32_t fetch_min(uint32_t i, uint32_t v) {
        return __hip_atomic_fetch_min(w + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ void lower(uint32_t i, uint32_t v) { fetch_min(i, v); }
};
struct RegAgentWords {  // the seams: every access an agent-scope atomic
    uint32_t* w;
    __device__ __forceinline__ uint32_t load(uint32_t i) { return __hip_atomic_load(w + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint32_t fetch_min(uint32_t i, uint32_t v) {
        return __hip_atomic_fetch_min(w + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void lower(uint32_t i, uint32_t v) { fetch_min(i, v); }
};
struct RegPlainWords {  // after the seams: nothing is lowered any more
    const uint32_t* w;
    __device__ __forceinline__ uint32_t load(uint32_t i) { return w[i]; }
    __device__ __forceinline__ void lower(uint32_t, uint32_t) {}  // the flatten kernel stores a lane's own entry, once, itself
};

template <typename W>
__global__ __launch_bounds__(kRegThreads) void k_regions_tiles(RegRaster<W> r, uint32_t tiles_x, bool eight, uint32_t* __restrict__ parent,
                                                                uint32_t* __restrict__ count) {
    __shared__ uint32_t words[kRegTileW * kRegTileH];
    constexpr int kPer = kRegTileW * kRegTileH / kRegThreads;
    const uint32_t x0 = (blockIdx.x % tiles_x) * uint32_t(kRegTileW), y0 = (blockIdx.x / tiles_x) * uint32_t(kRegTileH);
    RegLdsWords lds{words};
    uint32_t loads = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) words[threadIdx.x + k * kRegThreads] = threadIdx.x + k * kRegThreads;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const uint32_t li = threadIdx.x + k * kRegThreads, x = x0 + li % kRegTileW, y = y0 + li / kRegTileW;
        if (x >= r.cols || y >= r.rows) continue;
        const uint32_t links = reg_tile_links(r, y, x, kRegTileW, kRegTileH, eight);
        if (links & kRegLinkW) reg_unite(lds, li, li - 1, loads);
        if (links & kRegLinkN) reg_unite(lds, li, li - kRegTileW, loads);
        if (links & kRegLinkNW) reg_unite(lds, li, li - kRegTileW - 1, loads);
        if (links & kRegLinkNE) reg_unite(lds, li, li - kRegTileW + 1, loads);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const uint32_t li = threadIdx.x + k * kRegThreads, x = x0 + li % kRegTileW, y = y0 + li / kRegTileW;
        if (x >= r.cols || y >= r.rows) continue;
        const uint32_t root = reg_find(lds, li, loads);  // the tile's order of cells is the raster's: the least local is the least global
        const uint32_t i = y * r.cols + x;
        parent[i] = (y0 + root / kRegTileW) * r.cols + x0 + root % kRegTileW;
        if (count) count[i] = 0;
    }
}

template <typename W>
__global__ __launch_bounds__(kRegSeamLanes) void k_regions_seams(RegRaster<W> r, uint32_t tiles_x, bool eight, uint32_t* parent) {
    const uint32_t lane = threadIdx.x;
    if (lane >= uint32_t(kRegTileW + kRegTileH - 1)) return;
    // lanes 0 .. kRegTileW - 1: the last row; the rest: the last column above it
    const uint32_t lx = lane < uint32_t(kRegTileW) ? lane : uint32_t(kRegTileW - 1);
    const uint32_t ly = lane < uint32_t(kRegTileW) ? uint32_t(kRegTileH - 1) : lane - uint32_t(kRegTileW);
    const uint32_t x = (blockIdx.x % tiles_x) * uint32_t(kRegTileW) + lx, y = (blockIdx.x / tiles_x) * uint32_t(kRegTileH) + ly;
    if (x >= r.cols || y >= r.rows) return;
    RegAgentWords words{parent};
    uint32_t loads = 0;
    reg_seam_unite(words, r, y, x, kRegTileW, kRegTileH, eight, loads);
}

__global__ __launch_bounds__(kRegThreads) void k_regions_flatten(const uint8_t* __restrict__ mask, uint32_t n, uint32_t* parent, uint32_t* count) {
    const uint32_t i = blockIdx.x * uint32_t(kRegThreads) + threadIdx.x;
    const bool valid = i < n && (!mask || mask[i] != 0);
    uint32_t root = 0xFFFFFFFFu, loads = 0;
    if (valid) {
        RegPlainWords words{parent};
        root = reg_find(words, i, loads);
        if (root != i) parent[i] = root;
    }
    if (!count) return;
    // one add per distinct root of the wave: the lanes that share the first waiting lane's root leave together
    bool waiting = valid;
    for (;;) {
        const uint64_t left = __builtin_amdgcn_ballot_w64(waiting);
        if (left == 0) break;
        const uint32_t first = __builtin_amdgcn_readlane(root, __builtin_ctzll(left));
        const uint64_t same = __builtin_amdgcn_ballot_w64(waiting && root == first);
        if (waiting && root == first) {
            if ((same & ((1ull << (threadIdx.x % 64u)) - 1ull)) == 0) atomicAdd(count + first, uint32_t(__builtin_popcountll(same)));
            waiting = false;
        }
    }
}

// is cell i a root of a kept region
__device__ __forceinline__ bool reg_kept_root(const uint8_t* mask, const uint32_t* parent, const uint32_t* count, uint32_t i, uint32_t need) {
    if (mask && mask[i] == 0) return false;
    if (parent[i] != i) return false;
    return need <= 1 || count[i] >= need;
}

// the kept roots among this lane's kRegScanCells / kRegThreads consecutive cells, as bits
__device__ __forceinline__ uint32_t reg_lane_roots(const uint8_t* mask, const uint32_t* parent, const uint32_t* count, uint32_t n, uint32_t need,
                                                   uint32_t first) {
    constexpr int kPer = kRegScanCells / kRegThreads;
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k)
        if (first + k < n && reg_kept_root(mask, parent, count, first + k, need)) bits |= 1u << k;
    return bits;
}

// the inclusive scan of one value per lane over the workgroup; scratch: kRegThreads words
__device__ __forceinline__ uint32_t reg_block_scan(uint32_t v, uint32_t* scratch) {
    scratch[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = 1; d < uint32_t(kRegThreads); d <<= 1) {
        const uint32_t add = threadIdx.x >= d ? scratch[threadIdx.x - d] : 0u;
        __syncthreads();
        scratch[threadIdx.x] += add;
        __syncthreads();
    }
    return scratch[threadIdx.x];
}

__global__ __launch_bounds__(kRegThreads) void k_regions_sums(const uint8_t* __restrict__ mask, const uint32_t* __restrict__ parent,
                                                               const uint32_t* __restrict__ count, uint32_t n, uint32_t need,
                                                               uint32_t* __restrict__ sums) {
    __shared__ uint32_t scratch[kRegThreads];
    const uint32_t first = blockIdx.x * uint32_t(kRegScanCells) + threadIdx.x * uint32_t(kRegScanCells / kRegThreads);
    const uint32_t total = reg_block_scan(uint32_t(__builtin_popcount(reg_lane_roots(mask, parent, count, n, need, first))), scratch);
    if (threadIdx.x == kRegThreads - 1) sums[blockIdx.x] = total;
}

// one workgroup; a lane scans a run of consecutive sums, the runs are scanned across the lanes
__global__ __launch_bounds__(kRegThreads) void k_regions_scan(uint32_t* __restrict__ sums, uint32_t blocks, uint64_t* __restrict__ n_regions) {
    __shared__ uint32_t scratch[kRegThreads];
    const uint32_t per = (blocks + uint32_t(kRegThreads) - 1) / uint32_t(kRegThreads);
    const uint32_t lo = threadIdx.x * per < blocks ? threadIdx.x * per : blocks, hi = lo + per < blocks ? lo + per : blocks;
    uint32_t mine = 0;
    for (uint32_t b = lo; b < hi; ++b) mine += sums[b];
    const uint32_t upto = reg_block_scan(mine, scratch);
    uint32_t run = upto - mine;
    for (uint32_t b = lo; b < hi; ++b) {
        const uint32_t s = sums[b];
        sums[b] = run;
        run += s;
    }
    if (threadIdx.x == kRegThreads - 1 && n_regions) *n_regions = uint64_t(upto);
}

__global__ __launch_bounds__(kRegThreads) void k_regions_number(const uint8_t* __restrict__ mask, const uint32_t* __restrict__ parent, uint32_t* count,
                                                                 uint32_t n, uint32_t need, const uint32_t* __restrict__ sums) {
    __shared__ uint32_t scratch[kRegThreads];
    constexpr int kPer = kRegScanCells / kRegThreads;
    const uint32_t first = blockIdx.x * uint32_t(kRegScanCells) + threadIdx.x * uint32_t(kPer);
    const uint32_t bits = reg_lane_roots(mask, parent, count, n, need, first);
    const uint32_t mine = uint32_t(__builtin_popcount(bits));
    uint32_t number = sums[blockIdx.x] + reg_block_scan(mine, scratch) - mine;  // kept roots before this lane's cells
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        if (first + k >= n || parent[first + k] != first + k) continue;  // a lane writes only at its own cells that are roots
        count[first + k] = (bits >> k) & 1u ? ++number : 0u;
    }
}

template <bool VALUES, bool MASKOUT>
__global__ __launch_bounds__(kRegThreads) void k_regions_store(const uint8_t* __restrict__ mask, const uint32_t* __restrict__ parent,
                                                                const uint32_t* __restrict__ count, uint32_t n, bool dense, uint32_t need,
                                                                int32_t* __restrict__ dst, uint8_t* __restrict__ dst_mask) {
    const uint32_t first = (blockIdx.x * uint32_t(kRegThreads) + threadIdx.x) * 4u;
    if (first >= n) return;
    const bool sized = dense || need > 1;  // else count[] holds nothing
    if (first + 4u <= n) {
        const vec<uint32_t, 4> up = *reinterpret_cast<const vec<uint32_t, 4>*>(parent + first);
        const uint32_t valid = mask ? plain_load(reinterpret_cast<const uint32_t*>(mask + first)) : 0x01010101u;
        vec<uint32_t, 4> label;
        uint32_t bytes = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool ok = ((valid >> (8 * k)) & 0xFFu) != 0;
            label[k] = reg_label(ok, up[k], ok && sized ? count[up[k]] : 0u, dense, need);
            bytes |= (label[k] != 0 ? 1u : 0u) << (8 * k);
        }
        if constexpr (VALUES) nt_store(label, reinterpret_cast<vec<uint32_t, 4>*>(dst + first));
        if constexpr (MASKOUT) mask_store(bytes, reinterpret_cast<uint32_t*>(dst_mask + first));
        return;
    }
    for (uint32_t i = first; i < n; ++i) {
        const bool ok = !mask || mask[i] != 0;
        const uint32_t up = parent[i];
        const uint32_t label = reg_label(ok, up, ok && sized ? count[up] : 0u, dense, need);
        if constexpr (VALUES) st_cell(int32_t(label), dst + i);
        if constexpr (MASKOUT) mask_store(uint8_t(label != 0), dst_mask + i);
    }
}

}  // namespace ecd
