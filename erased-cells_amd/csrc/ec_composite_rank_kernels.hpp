// ec_composite_rank_kernels.hpp — ec_composite_rank (include/erased_cells.h) on gfx950: the stack of K layers is read once, a
// cell's K words (ec_composite_rank_cell.hpp) are all in registers at once, sorted by a fixed network and the position r(count)
// taken by a select chain.  No LDS, no memory-resident array: every index into the words is a constant.
//
// The frame is k_composite's: the K layer pointers and the K mask pointers travel in the kernel's arguments (CompositeRankArgs, by
// value) and are read with constant indices, so they come in by scalar loads; so does the table r(c), 65 words the host computed
// from (num, den, method) — no lane divides.  A kernel is instantiated per cell type and per BUCKET KB, the stack's height rounded up
// to a power of two (1 .. 64); layers b >= K are a wave-uniform branch that makes sentinels, never a load.
//
// One workgroup per tile of kBlock groups, straight-line; a group is G cells of one lane, G = rank_group(cell bytes, KB): as many as
// keep G x KB words within 64 registers, at most 16 bytes.  Every value and mask load is `nt`; 1-byte streams travel as words (cells<T, N> / load_cells);
// values leave with nt_store / st_cell, mask and aux bytes with mask_store.  Pointers may sit at any cell offset (under-aligned
// accesses, ec_device.hpp); the cell-wise kernel runs only when the "unaligned_vector" knob is off and a pointer is not aligned
// to its group.  The last group, when it is partial, loads and stores cell by cell under a guard and goes through the same sort.
#pragma once

#include "ec_composite_rank_cell.hpp"
#include "ec_map_kernels.hpp"
#include "ec_stack_plan.hpp"

namespace ecd {

struct CompositeRankArgs : ecs::StackArgs {  // the stack (ec_stack_plan.hpp), then this family's own
    RankTable rank;  // r(c), c = 1 .. 64
};
static_assert(ecs::kMaxLayers == kCompositeMaxLayers && sizeof(CompositeRankArgs) == 1328 && offsetof(CompositeRankArgs, rank) == sizeof(ecs::StackArgs),
              "the kernels read the block at constant offsets: its layout is part of them");

// registers one word takes
constexpr int rank_word_regs(size_t cell_bytes) { return cell_bytes <= 2 ? 1 : cell_bytes == 4 ? 2 : 3; }
// cells per lane per group: a power of two, at most 16 bytes of cells, G x KB words within 64 registers — but four cells of one or
// two bytes at 32 layers, which ran 1.8 times faster than two (both from the A/B of DESIGN §5).  The host's tile count and the
// kernels agree through this.
constexpr int rank_group(size_t cell_bytes, int kb) {
    int g = 16 / int(cell_bytes);
    while (g > 1 && g * kb * rank_word_regs(cell_bytes) > 64) g /= 2;
    return cell_bytes <= 2 && kb == 32 ? 4 : g;
}

// G cells of one stream as one access returns them: a whole group of cells (1-byte cells as words, ec_device.hpp), or one cell
template <typename T, int G>
struct rank_cells {
    cells<T, G> x;
    __device__ __forceinline__ T operator[](int c) const { return x[c]; }
    static __device__ __forceinline__ rank_cells load(const T* first) { return rank_cells{load_cells<true, T, G>(first)}; }
};
template <typename T>
struct rank_cells<T, 1> {
    T x;
    __device__ __forceinline__ T operator[](int) const { return x; }
    static __device__ __forceinline__ rank_cells load(const T* first) { return rank_cells{ld_cell(first)}; }
};

// the G cells from `first` on through every layer, then their stores.  WHOLE: all G lie below n.
template <typename T, int KB, int G>
__device__ __forceinline__ void rank_group_run(const CompositeRankArgs& a, size_t first) {
    using W = typename rank_word<T>::type;
    const bool whole = first + G <= a.n;
    // What the two arms hand on is never a byte: 1-byte cells and mask bytes that crossed the join were gathered back into
    // <N x i8> vector loads, which lose `nt` when they are legalised (ec_device.hpp, cells<>; tools/isa_audit.py found the mask loads
    // of the 8-cell groups without it).  Two forms, each the faster one where it is used: 1- and 2-byte cells become
    // their words inside the arm that loaded them; wider cells are held as loaded, with their validity as a flag word, and become
    // words behind the join.
    W w[G][KB];
    uint32_t count[G];  // at most KB <= 64 flags each: the table's index is bounded by construction
#pragma unroll
    for (int c = 0; c < G; ++c) count[c] = 0;
    if constexpr (sizeof(T) <= 2) {
        if (whole) {
#pragma unroll
            for (int b = 0; b < KB; ++b) {
                if (b < a.layers) {
                    const rank_cells<T, G> x = rank_cells<T, G>::load(static_cast<const T*>(a.p[b]) + first);
                    const uint8_t* m = a.m[b];
                    if (m) {
                        const rank_cells<uint8_t, G> mx = rank_cells<uint8_t, G>::load(m + first);
#pragma unroll
                        for (int c = 0; c < G; ++c) {
                            const bool valid = mx[c] != 0;
                            w[c][b] = rank_word<T>::make(x[c], valid, uint32_t(b));
                            count[c] += valid ? 1u : 0u;
                        }
                    } else {
#pragma unroll
                        for (int c = 0; c < G; ++c) {
                            w[c][b] = rank_word<T>::make(x[c], true, uint32_t(b));
                            count[c] += 1u;
                        }
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < G; ++c) w[c][b] = rank_word<T>::make(T(0), false, uint32_t(b));
                }
            }
        } else {
#pragma unroll
            for (int b = 0; b < KB; ++b) {
#pragma unroll
                for (int c = 0; c < G; ++c) w[c][b] = rank_word<T>::make(T(0), false, uint32_t(b));
                if (b < a.layers) {
                    const T* p = static_cast<const T*>(a.p[b]);
                    const uint8_t* m = a.m[b];
#pragma unroll
                    for (int c = 0; c < G; ++c) {
                        if (first + c < a.n) {
                            const T x = ld_cell(p + first + c);  // unconditional within the guard, as in composite_cell
                            uint8_t mb = 1;
                            if (m) mb = ld_cell(m + first + c);
                            w[c][b] = rank_word<T>::make(x, mb != 0, uint32_t(b));
                            count[c] += mb != 0 ? 1u : 0u;
                        }
                    }
                }
            }
        }
    } else {
        T v[KB][G];
        uint32_t ok[KB][G];
        if (whole) {
#pragma unroll
            for (int b = 0; b < KB; ++b) {
                if (b < a.layers) {
                    const rank_cells<T, G> x = rank_cells<T, G>::load(static_cast<const T*>(a.p[b]) + first);
#pragma unroll
                    for (int c = 0; c < G; ++c) v[b][c] = x[c];
                    const uint8_t* m = a.m[b];
                    if (m) {
                        const rank_cells<uint8_t, G> mx = rank_cells<uint8_t, G>::load(m + first);
#pragma unroll
                        for (int c = 0; c < G; ++c) ok[b][c] = mx[c] != 0 ? 1u : 0u;
                    } else {
#pragma unroll
                        for (int c = 0; c < G; ++c) ok[b][c] = 1u;
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < G; ++c) v[b][c] = T(0), ok[b][c] = 0u;
                }
            }
        } else {
#pragma unroll
            for (int b = 0; b < KB; ++b) {
#pragma unroll
                for (int c = 0; c < G; ++c) v[b][c] = T(0), ok[b][c] = 0u;
                if (b < a.layers) {
                    const T* p = static_cast<const T*>(a.p[b]);
                    const uint8_t* m = a.m[b];
#pragma unroll
                    for (int c = 0; c < G; ++c) {
                        if (first + c < a.n) {
                            v[b][c] = ld_cell(p + first + c);  // unconditional within the guard, as in composite_cell
                            uint8_t mb = 1;
                            if (m) mb = ld_cell(m + first + c);
                            ok[b][c] = mb != 0 ? 1u : 0u;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < G; ++c)
#pragma unroll
            for (int b = 0; b < KB; ++b) {
                w[c][b] = rank_word<T>::make(v[b][c], ok[b][c] != 0, uint32_t(b));
                count[c] += ok[b][c];
            }
    }
    T out[G];
    uint8_t mo[G], ao[G];
#pragma unroll
    for (int c = 0; c < G; ++c) out[c] = rank_cell<T, KB>(w[c], count[c], a.rank.r, a.min_count, &mo[c], &ao[c]);
    if (whole) {
        if constexpr (G == 1) {
            st_cell<T>(out[0], static_cast<T*>(a.dst) + first);
            if (a.dst_mask) st_cell<uint8_t>(mo[0], a.dst_mask + first);
            if (a.aux) st_cell<uint8_t>(ao[0], a.aux + first);
        } else {
            using RV = vec<T, G>;
            using MV = vec<uint8_t, G>;
            RV r;
            MV mv, av;
#pragma unroll
            for (int c = 0; c < G; ++c) r[c] = out[c], mv[c] = mo[c], av[c] = ao[c];
            nt_store(r, reinterpret_cast<RV*>(static_cast<T*>(a.dst) + first));
            if (a.dst_mask) mask_store(mv, reinterpret_cast<MV*>(a.dst_mask + first));
            if (a.aux) mask_store(av, reinterpret_cast<MV*>(a.aux + first));
        }
    } else {
#pragma unroll
        for (int c = 0; c < G; ++c) {
            if (first + c < a.n) {
                st_cell<T>(out[c], static_cast<T*>(a.dst) + first + c);
                if (a.dst_mask) st_cell<uint8_t>(mo[c], a.dst_mask + first + c);
                if (a.aux) st_cell<uint8_t>(ao[c], a.aux + first + c);
            }
        }
    }
}

template <typename T, int KB>
__global__ __launch_bounds__(kBlock) void k_composite_rank(const CompositeRankArgs a, const size_t first_tile) {
    constexpr size_t G = rank_group(sizeof(T), KB);
    const size_t first = (two_front_tile(first_tile) * kBlock + threadIdx.x) * G;  // one workgroup per tile, straight-line
    if (first < a.n) rank_group_run<T, KB, int(G)>(a, first);
}

template <typename T, int KB>
__global__ __launch_bounds__(kBlock) void k_composite_rank_cellwise(const CompositeRankArgs a) {
    const size_t stride = size_t(gridDim.x) * kBlock;
    for (size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x; i < a.n; i += stride) rank_group_run<T, KB, 1>(a, i);
}

}  // namespace ecd
