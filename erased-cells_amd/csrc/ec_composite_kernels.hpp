// ec_composite_kernels.hpp — ec_composite (include/erased_cells.h) on gfx950: one pass over a stack of K layers, K a run-time
// number.  Not a k_map Fn: k_map loads every input of a group at once, here the layers are walked in batches.
//
// The K layer pointers and the K mask pointers travel in the kernel's arguments (CompositeArgs, by value) and are read with a
// wave-uniform index, so they come in by scalar loads; nothing is uploaded and no lane holds a pointer table.  One workgroup
// per tile of kBlock x U groups, straight-line; a group is CPL = 16 / max(cell bytes, result cell bytes) cells, so the widest
// stream moves 16 bytes per lane per access.  Per tile the layers go in batches of kCompositeBatch: the batch's value loads and the
// mask loads of a batch are issued together, then folded into the per-cell state (ec_composite_cell.hpp) in ascending k.  A layer
// without a mask is a wave-uniform branch, never a load.  The layers past the last whole batch go one at a time.
//
// Every value and mask load is `nt` (a stack is read once and rarely fits the Infinity Cache: no policy arms); 1-byte streams
// travel as words (cells<T, N> / load_cells); values leave with nt_store / st_cell, mask and aux bytes with mask_store.
// Pointers may sit at any cell offset (under-aligned accesses, ec_device.hpp); the cell-wise kernel runs only when the
// "unaligned_vector" knob is off and a pointer is not aligned to its group.  Ragged tails are guarded in the last tile, the
// cells past the last group go through composite_cell — the same per-cell functions either way.
#pragma once

#include "ec_composite_cell.hpp"
#include "ec_map_kernels.hpp"
#include "ec_stack_plan.hpp"

namespace ecd {

constexpr int kCompositeBatch = 4;  // layers whose loads are in flight together

struct CompositeArgs : ecs::StackArgs {  // the stack (ec_stack_plan.hpp), then this family's own
    uint32_t mean;
};
static_assert(ecs::kMaxLayers == kCompositeMaxLayers && sizeof(CompositeArgs) == 1072 && offsetof(CompositeArgs, mean) == sizeof(ecs::StackArgs),
              "the kernels read the block at constant offsets: its layout is part of them");

// groups per lane per tile: the host's tile count and the kernels agree through this
constexpr int composite_u(bool sums, size_t cell_bytes) { return sums ? 2 : cell_bytes == 1 ? 1 : 2; }

template <typename T, int OP>
struct CompositeShape {
    using R = typename composite_result<T, OP>::type;
    static constexpr int CPL = 16 / max_of<sizeof(T), sizeof(R)>::value;
    static constexpr int U = composite_u(composite_sums(OP), sizeof(T));
};

// NB layers from k0 on, folded into the states of U groups (group j of the lane is g0 + j * kBlock)
template <typename T, int OP, int U, int NB>
__device__ __forceinline__ void composite_batch(const CompositeArgs& a, int k0, size_t g0,
                                                composite_state<T, OP> (&st)[U][CompositeShape<T, OP>::CPL]) {
    constexpr int CPL = CompositeShape<T, OP>::CPL;
    cells<T, CPL> v[NB][U];
    cells<uint8_t, CPL> mk[NB][U];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const T* p = static_cast<const T*>(a.p[k0 + b]);
        const uint8_t* m = a.m[k0 + b];
#pragma unroll
        for (int j = 0; j < U; ++j) v[b][j] = load_cells<true, T, CPL>(p + (g0 + size_t(j) * kBlock) * CPL);
        if (m) {
#pragma unroll
            for (int j = 0; j < U; ++j) mk[b][j] = load_cells<true, uint8_t, CPL>(m + (g0 + size_t(j) * kBlock) * CPL);
        } else {
#pragma unroll
            for (int j = 0; j < U; ++j) mk[b][j].v = typename cells<uint8_t, CPL>::rep(0x01010101u);
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < U; ++j)
#pragma unroll
            for (int c = 0; c < CPL; ++c) composite_step<T, OP>(st[j][c], v[b][j][c], mk[b][j][c] != 0, uint32_t(k0 + b));
}

// U groups of one lane through every layer, then their stores
template <typename T, int OP, int U>
__device__ __forceinline__ void composite_groups(const CompositeArgs& a, size_t g0) {
    using S = CompositeShape<T, OP>;
    using R = typename S::R;
    constexpr int CPL = S::CPL;
    using RV = vec<R, CPL>;
    using MV = vec<uint8_t, CPL>;
    composite_state<T, OP> st[U][CPL];
#pragma unroll
    for (int j = 0; j < U; ++j)
#pragma unroll
        for (int c = 0; c < CPL; ++c) st[j][c] = composite_init<T, OP>();
    int k = 0;
    for (; k + kCompositeBatch <= a.layers; k += kCompositeBatch) composite_batch<T, OP, U, kCompositeBatch>(a, k, g0, st);
    for (; k < a.layers; ++k) composite_batch<T, OP, U, 1>(a, k, g0, st);
#pragma unroll
    for (int j = 0; j < U; ++j) {
        const size_t g = g0 + size_t(j) * kBlock;
        RV r;
        MV mo, ao;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            uint8_t mb, ab;
            r[c] = composite_finish<T, OP>(st[j][c], a.min_count, a.mean != 0, &mb, &ab);
            mo[c] = mb;
            ao[c] = ab;
        }
        nt_store(r, reinterpret_cast<RV*>(a.dst) + g);
        if (a.dst_mask) mask_store(mo, reinterpret_cast<MV*>(a.dst_mask) + g);
        if (a.aux) mask_store(ao, reinterpret_cast<MV*>(a.aux) + g);
    }
}

// one cell, any alignment
template <typename T, int OP>
__device__ __forceinline__ void composite_cell(const CompositeArgs& a, size_t i) {
    using R = typename CompositeShape<T, OP>::R;
    composite_state<T, OP> s = composite_init<T, OP>();
    for (int k = 0; k < a.layers; ++k) {
        const uint8_t* m = a.m[k];
        const T v = ld_cell(static_cast<const T*>(a.p[k]) + i);  // unconditional, as in MaskSelectFn
        uint8_t mb = 1;
        if (m) mb = ld_cell(m + i);
        composite_step<T, OP>(s, v, mb != 0, uint32_t(k));
    }
    uint8_t mb, ab;
    const R r = composite_finish<T, OP>(s, a.min_count, a.mean != 0, &mb, &ab);
    st_cell<R>(r, static_cast<R*>(a.dst) + i);
    if (a.dst_mask) st_cell<uint8_t>(mb, a.dst_mask + i);
    if (a.aux) st_cell<uint8_t>(ab, a.aux + i);
}

template <typename T, int OP>
__global__ __launch_bounds__(kBlock) void k_composite(const CompositeArgs a, const size_t first_tile) {
    constexpr int U = CompositeShape<T, OP>::U;
    constexpr size_t CPL = CompositeShape<T, OP>::CPL;
    constexpr size_t TILE = size_t(kBlock) * U;
    const size_t ngroups = a.n / CPL;
    const size_t tile = two_front_tile(first_tile);  // one workgroup per tile, straight-line
    const size_t base = tile * TILE + threadIdx.x;
    if (tile * TILE + TILE <= ngroups) {
        composite_groups<T, OP, U>(a, base);
    } else {
#pragma unroll 1
        for (int j = 0; j < U; ++j) {
            const size_t g = base + size_t(j) * kBlock;
            if (g < ngroups) composite_groups<T, OP, 1>(a, g);
        }
    }
    if (first_group(first_tile))
        for (size_t i = ngroups * CPL + threadIdx.x; i < a.n; i += kBlock) composite_cell<T, OP>(a, i);
}

template <typename T, int OP>
__global__ __launch_bounds__(kBlock) void k_composite_cellwise(const CompositeArgs a) {
    const size_t stride = size_t(gridDim.x) * kBlock;
    for (size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x; i < a.n; i += stride) composite_cell<T, OP>(a, i);
}

}  // namespace ecd
