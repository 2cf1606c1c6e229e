// ec_reclass_kernels.hpp — a raster classified by break values (gfx950): the device side of ec_reclass
// (include/erased_cells.h).  The frame is k_zonal_broadcast's — the k_map tile (ec_map_kernels.hpp: one workgroup per tile of
// U groups per lane, two fronts, the ragged tail by workgroup 0, a cell-wise twin) behind an LDS prologue.
//
// The record (ec_reclass_table, built on the host: ec_reclass_plan.hpp) holds thresholds in the order keys of T, so a cell's
// class is c = #{ j < n_reached : thr[j] <= order_key<T>(x) }: the kernels know neither the breaks' type nor `right` and are
// typed by (T, W = the unsigned word of the output's width) only.
//
// The prologue.  Thread i of the 256 stages slot i of the record: threshold i (a key of a type of at most 4 bytes as int32 —
// u32 biased by 2^31, which keeps the order — else int64; slots from n_reached on are 0 and never decide), class value i as
// a W, validity byte i.  n_reached is clamped to 0 .. 255 whatever the record says; nothing else of it is an index.
//   1-byte T   a second step: thread i classifies THE cell whose byte is i and leaves out_lut[i] / valid_lut[i].  The
//              streaming part is then one LDS read per cell (indexed by the cell's UNSIGNED byte) and no search.
//   wider T    a branch-free upper bound per cell: ceil(log2(n_reached + 1)) steps, the same for every lane (a scalar trip
//              count), no divergent exit; the cells of a lane's group step together, so their LDS reads are independent.
// LDS: 1.3 - 4.3 KiB (1-byte T: up to 5.5 KiB), far from what bounds occupancy.
//
// Loads and stores as in every map kernel: the value operand takes the launch's load policy (cache_plan -> policy_arms), mask
// bytes and the record load nt, every load is unconditional — a masked-out cell is loaded, classified and not used, so what it
// holds leaves no trace — values leave with nt_store / st_cell, mask bytes with mask_store.  The mask OUTPUT is a launch-uniform
// branch, not a template parameter: it halves the instantiations (10 T x 4 W x 2 mask-in x 2 kernels).
#pragma once

#include <type_traits>

#include "ec_map_kernels.hpp"
#include "ec_reclass_plan.hpp"

namespace ecd {

static_assert(ecr::kBlock == kBlock && ecr::kSlots == kBlock, "one thread per slot of the record");

template <typename T>
using reclass_key_t = std::conditional_t<sizeof(T) == 8, int64_t, int32_t>;

// an order key of T (ec_order_key.hpp) as the key the kernels compare
template <typename T>
__device__ __forceinline__ reclass_key_t<T> reclass_key(int64_t k) {
    if constexpr (sizeof(T) == 8) return k;
    else if constexpr (sizeof(T) == 4 && !is_fp<T>::value && T(-1) > T(0)) return static_cast<int32_t>(static_cast<uint32_t>(k) ^ 0x80000000u);  // u32
    else return static_cast<int32_t>(k);
}

template <typename T, typename W>
struct ReclassLds {
    reclass_key_t<T> thr[ecr::kSlots];
    W vals[ecr::kSlots];
    W out_lut[sizeof(T) == 1 ? ecr::kSlots : 1];
    uint8_t valid[ecr::kSlots];
    uint8_t valid_lut[sizeof(T) == 1 ? ecr::kSlots : 1];
};

// c = #{ j < nr : thr[j] <= key[k] } for the N cells of a group; nr <= 255, so no index passes 254
template <typename K, int N>
__device__ __forceinline__ void reclass_search(const K* thr, int nr, int steps, const K (&key)[N], int (&c)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) c[k] = 0;
    for (int step = (1 << steps) >> 1; step != 0; step >>= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const int idx = c[k] + step - 1;
            const K t = thr[idx];
            c[k] += (idx < nr && t <= key[k]) ? step : 0;
        }
    }
}

template <typename T>
struct one_cell {
    T v;
    __device__ __forceinline__ T operator[](int) const { return v; }
};

template <typename T, typename W, bool MASKED>
struct Reclass {
    using K = reclass_key_t<T>;
    ReclassLds<T, W>& s;
    int nr, steps;
    W nd;
    bool maskout;

    // the prologue; every thread of the workgroup calls it
    __device__ __forceinline__ Reclass(ReclassLds<T, W>& lds, const ec_reclass_table* __restrict__ tab, bool maskout_) : s(lds), maskout(maskout_) {
        const int i = threadIdx.x;
        int n = __builtin_amdgcn_readfirstlane(ld_cell(&tab->n_reached));
        n = n < 0 ? 0 : n > ecr::kMaxBreaks ? ecr::kMaxBreaks : n;
        nr = n;
        steps = n == 0 ? 0 : 32 - __builtin_clz(static_cast<unsigned>(n));  // the bit width of n: ceil(log2(n + 1))
        const int64_t t = ld_cell(&tab->thr[i < ecr::kMaxBreaks ? i : ecr::kMaxBreaks - 1]);
        s.thr[i] = i < n ? reclass_key<T>(t) : K(0);
        s.vals[i] = static_cast<W>(ld_cell(&tab->value_bits[i]));
        s.valid[i] = ld_cell(&tab->valid[i]) != 0;
        nd = static_cast<W>(ld_cell(&tab->nodata_bits));
        __syncthreads();
        if constexpr (sizeof(T) == 1) {
            const K key[1] = {reclass_key<T>(order_key<T>(static_cast<T>(static_cast<uint8_t>(i))))};
            int c[1];
            reclass_search<K, 1>(s.thr, nr, steps, key, c);
            s.out_lut[i] = s.vals[c[0]];
            s.valid_lut[i] = s.valid[c[0]];
            __syncthreads();
        }
    }

    // X, M: N cells and their mask bytes behind operator[] (cells<T, N>, one_cell<T>)
    template <int N, typename X, typename M>
    __device__ __forceinline__ void classify(const X& x, const M& m, W (&o)[N], uint8_t (&ok)[N]) const {
        if constexpr (sizeof(T) == 1) {
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const int b = static_cast<uint8_t>(x[k]);
                o[k] = s.out_lut[b];
                ok[k] = maskout ? s.valid_lut[b] : uint8_t(1);
            }
        } else {
            K key[N];
            int c[N];
#pragma unroll
            for (int k = 0; k < N; ++k) key[k] = reclass_key<T>(order_key<T>(x[k]));
            reclass_search<K, N>(s.thr, nr, steps, key, c);
#pragma unroll
            for (int k = 0; k < N; ++k) {
                o[k] = s.vals[c[k]];
                ok[k] = maskout ? s.valid[c[k]] : uint8_t(1);
            }
        }
        if constexpr (MASKED) {
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const bool in = m[k] != 0;
                o[k] = in ? o[k] : nd;
                ok[k] = in ? ok[k] : uint8_t(0);
            }
        }
    }

    // one cell, any alignment
    __device__ __forceinline__ void cell(const T* __restrict__ src, const uint8_t* __restrict__ mask, W* __restrict__ dst, uint8_t* __restrict__ dst_mask,
                                         size_t i) const {
        const one_cell<T> x{ld_cell(src + i)};
        one_cell<uint8_t> m{1};
        if constexpr (MASKED) m.v = ld_cell(mask + i);
        W o[1];
        uint8_t ok[1];
        classify<1>(x, m, o, ok);
        st_cell<W>(o[0], dst + i);
        if (maskout) st_cell<uint8_t>(ok[0], dst_mask + i);
    }
};

template <typename T, typename W, bool MASKED, int U>
__global__ __launch_bounds__(kBlock) void k_reclass(const T* __restrict__ src, const uint8_t* __restrict__ mask,
                                                    const ec_reclass_table* __restrict__ tab, W* __restrict__ dst, uint8_t* __restrict__ dst_mask,
                                                    size_t n, unsigned cacheable, size_t first_tile) {
    __shared__ ReclassLds<T, W> lds;
    const Reclass<T, W, MASKED> rc(lds, tab, dst_mask != nullptr);
    constexpr int CPL = 16 / max_of<sizeof(T), sizeof(W)>::value;
    using DV = vec<W, CPL>;
    using MV = vec<uint8_t, CPL>;
    const size_t ngroups = n / CPL;
    constexpr size_t TILE = size_t(kBlock) * U;
    const size_t tile = two_front_tile(first_tile);
    const size_t base = tile * TILE + threadIdx.x;
    auto store = [&](size_t g, const cells<T, CPL>& x, const cells<uint8_t, CPL>& m) {
        W o[CPL];
        uint8_t ok[CPL];
        rc.template classify<CPL>(x, m, o, ok);
        DV ov;
        MV mv;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            ov[k] = o[k];
            mv[k] = ok[k];
        }
        nt_store(ov, reinterpret_cast<DV*>(dst) + g);
        if (rc.maskout) mask_store(mv, reinterpret_cast<MV*>(dst_mask) + g);
    };
    if (tile * TILE + TILE <= ngroups) {
        cells<T, CPL> x[U];
        cells<uint8_t, CPL> m[U] = {};
        policy_arms<1>(cacheable, [&](auto bits) {
            constexpr unsigned B = decltype(bits)::value;
#pragma unroll
            for (int j = 0; j < U; ++j) x[j] = load_cells<!(B & 1u), T, CPL>(src + (base + size_t(j) * kBlock) * CPL);
        });
        if constexpr (MASKED) {
#pragma unroll
            for (int j = 0; j < U; ++j) m[j] = load_cells<true, uint8_t, CPL>(mask + (base + size_t(j) * kBlock) * CPL);
        }
#pragma unroll
        for (int j = 0; j < U; ++j) store(base + size_t(j) * kBlock, x[j], m[j]);
    } else {
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const size_t g = base + size_t(j) * kBlock;
            if (g >= ngroups) continue;
            const cells<T, CPL> x = load_cells<true, T, CPL>(src + g * CPL);
            cells<uint8_t, CPL> m = {};
            if constexpr (MASKED) m = load_cells<true, uint8_t, CPL>(mask + g * CPL);
            store(g, x, m);
        }
    }
    if (first_group(first_tile))
        for (size_t i = ngroups * CPL + threadIdx.x; i < n; i += kBlock) rc.cell(src, mask, dst, dst_mask, i);
}

template <typename T, typename W, bool MASKED>
__global__ __launch_bounds__(kBlock) void k_reclass_cellwise(const T* __restrict__ src, const uint8_t* __restrict__ mask,
                                                             const ec_reclass_table* __restrict__ tab, W* __restrict__ dst,
                                                             uint8_t* __restrict__ dst_mask, size_t n) {
    __shared__ ReclassLds<T, W> lds;
    const Reclass<T, W, MASKED> rc(lds, tab, dst_mask != nullptr);
    const size_t stride = size_t(gridDim.x) * kBlock;
    for (size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) rc.cell(src, mask, dst, dst_mask, i);
}

}  // namespace ecd
