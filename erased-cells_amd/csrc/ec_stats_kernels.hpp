// ec_stats_kernels.hpp — count, min, max and the first two moments of a buffer in one pass (gfx950): the device side of
// ec_stats_device (include/erased_cells.h).  The reference has min_max only (BufferOps::min_max, src/buffer.rs:169-173;
// masked: src/masked/masked_buffer.rs:208-217); its test of NDVI against GDAL's band statistics
// (src/gdal/rasterband.rs:151-156) is what these kernels serve.
//
// The frame is the reductions' (ec_reduce_kernels.hpp, ec_reduce_plan.hpp): the launch shape of reduce_plan(), a read-only
// stream at 16 B per lane with U loads in flight, the peeled head and the ragged tail folded cell by cell by workgroup 0,
// one barrier per workgroup through block_fold over a Moments partial, partials in the stream's scratch, one finalize
// workgroup over block_fold (k_stats_finalize) — or, with a one-workgroup grid, the record written by that workgroup itself.  The
// launch sequence is launch_reduction's (ec_reduce_launch.hpp), which ec_stats.hip describes these kernels to.  The min/max
// part is MinMaxLanes (ec_reduce_kernels.hpp), the accumulator of k_min_max_partials, ByteFold included.  What is new is the moments:
//   kind 0 (1-, 2-, 4-byte integers)  exact: the count, the sum in int64, the sum of squares in 128 bits.
//   kind 1 (u64, i64, f32, f64)       d = to_f64(x) - pivot; s1 += d; s2 = fma(d, d, s2), one accumulator pair per slot of the
//                                     16-byte group, combined in slot order.  No atomics anywhere: the record is a pure
//                                     function of the cells and the launch plan.
// A cell that the mask hides is replaced by a select (never multiplied by 0), so a hidden NaN or Inf stays out of the sums.
// Mask bytes are 0 or 1 (`Vec<bool>` images, src/masked/mask.rs:10-12), as everywhere in this library.
//
// Overflow.  Accepted n (stats_max_cells, ec_stats_fold.hpp): 2^32 cells of 1 or 2 bytes, 2^31 of 4 bytes.  The smallest
// grid the plan can produce is ONE workgroup (a device of one CU with reduce_bpc = 1, or any short buffer), so the bounds
// below take a lane's share as n / BLOCK (vector kernel, BLOCK = 512) or n / kBlock (cell-wise kernel, 256), plus the head
// and tail cells: at most 2^24 + 32 cells per lane of 1 or 2 bytes, 2^23 + 32 of 4 bytes.  Each accumulator's bound stands
// beside it.  Across lanes and workgroups FoldMoments adds the count and the sum in 64 bits and the squares in 128; the
// totals are bounded by n * max|x| < 2^63 and n * max(x^2) < 2^96, whatever the grid.
#pragma once

#include "ec_lattice.hpp"
#include "ec_reduce_kernels.hpp"
#include "erased_cells.h"

namespace ecd {

template <typename T> struct StatsKind { static constexpr int value = (is_fp<T>::value || sizeof(T) == 8) ? 1 : 0; };

// Combines two partials.  KIND 0: a = sum (int64, two's complement), b / c = low / high word of the sum of squares.
// KIND 1: a, b = the bits of s1, s2.  IEEE addition is commutative, so both lanes of a shuffle pair compute the same bits
// and the wave's fold is one value whichever lane is read.
template <int KIND>
struct FoldMoments {
    __device__ __forceinline__ Moments operator()(const Moments& x, const Moments& y) const {
        Moments r;
        r.count = x.count + y.count;
        r.kmin = y.kmin < x.kmin ? y.kmin : x.kmin;
        r.kmax = y.kmax > x.kmax ? y.kmax : x.kmax;
        if constexpr (KIND == 0) {
            r.a = x.a + y.a;
            r.b = x.b + y.b;
            r.c = x.c + y.c + (r.b < x.b ? 1u : 0u);
        } else {
            r.a = f64_bits(bits_f64(x.a) + bits_f64(y.a));
            r.b = f64_bits(bits_f64(x.b) + bits_f64(y.b));
            r.c = 0;
        }
        return r;
    }
};

// The identity of FoldMoments for cell type T: nothing counted, the sentinels (T::MAX, T::MIN) of src/buffer.rs:170.
template <typename T>
__device__ __forceinline__ Moments moments_identity() {
    Moments r;
    r.count = 0;
    r.kmin = order_key<T>(Limits<T>::hi);
    r.kmax = order_key<T>(Limits<T>::lo);
    r.a = r.b = r.c = 0;  // +0.0 for kind 1
    return r;
}

// The pivot of a kind-1 scan: to_f64 of the buffer's first cell (src/value.rs:145-156) if finite, else 0.0 — whatever the
// mask says about that cell.  One address for the whole launch: a plain (cached) load that every lane shares.
template <typename T>
__device__ __forceinline__ double stats_pivot(const T* first_cell) {
    if constexpr (StatsKind<T>::value == 0) {
        return 0.0;
    } else {
        const double c = static_cast<double>(*first_cell);
        return __builtin_isfinite(c) ? c : 0.0;
    }
}

template <typename T>
__device__ __forceinline__ void write_record(ec_moments* __restrict__ out, const Moments& r, double pivot) {
    out->count = r.count;
    out->keys2[0] = ~r.kmin;
    out->keys2[1] = r.kmax;
    out->kind = StatsKind<T>::value;
    out->dtype = ecl::dtype_of<T>::value;
    if constexpr (StatsKind<T>::value == 0) {
        out->u.i.sum = static_cast<int64_t>(r.a);
        out->u.i.sq_lo = r.b;
        out->u.i.sq_hi = r.c;
    } else {
        out->u.f.pivot = pivot;
        out->u.f.s1 = bits_f64(r.a);
        out->u.f.s2 = bits_f64(r.b);
    }
    out->reserved = 0;
}

// One lane's running record, cell by cell: the head, the tail, the cell-wise kernel — and what the vector kernel's tile
// accumulators are flushed into.
template <typename T, bool MASKED>
struct CellMoments {
    using A = typename AccT<T>::type;
    static constexpr int KIND = StatsKind<T>::value;
    MinMaxLanes<T, MASKED> mm;  // the vector kernel folds its groups into it as well
    uint64_t cnt;    // <= 2^24 + 32 per lane
    int64_t sum;     // kind 0: |sum| <= (2^24 + 32) * 2^16 < 2^41 (1, 2 bytes); <= (2^23 + 32) * 2^32 < 2^56 (4 bytes)
    uint64_t sq_lo;  // kind 0: 1, 2 bytes: <= (2^24 + 32) * 2^32 < 2^57, never carries; 4 bytes: carries into sq_hi
    uint32_t sq_hi;  // kind 0: one carry per cell at most: <= 2^23 + 32 < 2^32
    double s1, s2;   // kind 1

    __device__ __forceinline__ void init() {
        mm.init();
        cnt = 0;
        sum = 0;
        sq_lo = 0;
        sq_hi = 0;
        s1 = s2 = 0.0;
    }
    __device__ __forceinline__ void add(T x, double pivot) {
        mm.fold_cell(x);
        ++cnt;
        if constexpr (KIND == 0) {
            const int64_t w = static_cast<int64_t>(x);
            const uint64_t q = static_cast<uint64_t>(w) * static_cast<uint64_t>(w);  // x * x mod 2^64 = x * x: at most 2^64 - 2^33 + 1
            sum += w;
            sq_lo += q;
            sq_hi += sq_lo < q ? 1u : 0u;
        } else {
            const double d = static_cast<double>(x) - pivot;
            s1 += d;
            s2 = __builtin_fma(d, d, s2);
        }
    }
    __device__ __forceinline__ Moments partial() const {
        Moments r;
        r.count = cnt;
        r.kmin = acc_to_i64<A>(mm.amin);
        r.kmax = acc_to_i64<A>(mm.amax);
        if constexpr (KIND == 0) {
            r.a = static_cast<uint64_t>(sum);
            r.b = sq_lo;
            r.c = sq_hi;
        } else {
            r.a = f64_bits(s1);
            r.b = f64_bits(s2);
            r.c = 0;
        }
        return r;
    }
};

// true cells among the mask bytes of one dword (bytes are 0 / 1): v_dot4_u32_u8 against ones
__device__ __forceinline__ uint32_t mask_word_count(uint32_t m, uint32_t acc) { return __builtin_amdgcn_udot4(m, 0x01010101u, acc, false); }

// partials[b] = the Moments of workgroup b.  Arguments as k_min_max_partials: `head` = peeled cells | load policy << 8;
// record_if_single != nullptr (one-workgroup grid): this workgroup's fold IS the result and it writes the record.
template <typename T, bool MASKED, int U, int BLOCK = kRBlock>
__global__ __launch_bounds__(BLOCK) void k_stats_partials(const T* __restrict__ p, const uint8_t* __restrict__ mask, size_t n,
                                                           Moments* __restrict__ partials, unsigned head,
                                                           ec_moments* __restrict__ record_if_single) {
    constexpr int KIND = StatsKind<T>::value;
    const double pivot = stats_pivot<T>(p);  // the FIRST cell of the buffer, before the peel moves p
    const unsigned cacheable = head >> 8;
    head &= 0xffu;
    p += head;
    if constexpr (MASKED) mask += head;
    n -= head;
    using A = typename AccT<T>::type;
    constexpr int CPL = 16 / sizeof(T);
    using TV = cells<T, CPL>;
    using MV = cells<uint8_t, CPL>;
    constexpr bool BYTES = sizeof(T) == 1;
    constexpr bool SIGNED = !is_fp<T>::value && T(-1) < T(0);
    const A hi0 = acc_key<T>(Limits<T>::hi), lo0 = acc_key<T>(Limits<T>::lo);
    CellMoments<T, MASKED> acc;  // the lane's record; its min/max lanes (acc.mm) take the groups of the tile loop too
    acc.init();
    double s1[CPL], s2[CPL];  // kind 1: one pair per slot of the 16-byte group
#pragma unroll
    for (int k = 0; k < CPL; ++k) s1[k] = s2[k] = 0.0;
    // Tile accumulators of the 1- and 2-byte paths, flushed into `acc` after every tile.  One tile is U * 16 = 128 bytes per lane:
    //   t_cnt  <= 128
    //   t_sum  1 byte: <= 128 * 255 < 2^15 (signed: |.| <= 128 * 128 = 2^14); 2 bytes: <= 64 * 65535 < 2^22 (signed: <= 2^21)
    //   t_sq   1 byte: <= 128 * 255^2 < 2^23 (signed: <= 128 * 2^14 = 2^21); unused for 2 bytes
    uint32_t t_cnt = 0, t_sum = 0, t_sq = 0;

    const size_t ngroups = n / CPL;
    constexpr size_t TILE = size_t(BLOCK) * U;
    const size_t ntiles = (ngroups + TILE - 1) / TILE;
    auto fold = [&](const TV& x, const MV& m) {
        if constexpr (BYTES) {
            acc.mm.fold_group(x, m);
            // four cells per instruction: v_dot4 against ones for the sum, against itself for the squares
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t xw = x.v[k];
                if constexpr (MASKED) {
                    xw &= m.v[k] * 0xFFu;  // 0 / 1 bytes -> 0x00 / 0xFF: a hidden cell becomes 0 and adds nothing
                    t_cnt = mask_word_count(m.v[k], t_cnt);
                }
                if constexpr (SIGNED) {
                    t_sum = static_cast<uint32_t>(__builtin_amdgcn_sdot4(static_cast<int>(xw), 0x01010101, static_cast<int>(t_sum), false));
                    t_sq = static_cast<uint32_t>(__builtin_amdgcn_sdot4(static_cast<int>(xw), static_cast<int>(xw), static_cast<int>(t_sq), false));
                } else {
                    t_sum = __builtin_amdgcn_udot4(xw, 0x01010101u, t_sum, false);
                    t_sq = __builtin_amdgcn_udot4(xw, xw, t_sq, false);
                }
            }
        } else {
            typename TV::rep xm = x.v;  // kind 0: the cells that count, a hidden cell as 0
            if constexpr (KIND != 0) (void)xm;
            if constexpr (MASKED && KIND == 0) {
                // MinMaxLanes::fold_group's loop with the hidden cell zeroed beside each slot's select, the parent's text: an unsigned
                // cell's zeroed form IS its max-side select, and only written like this (hi0 / lo0 the kernel's, one loop) does the
                // compiler keep them as one — else +5 % (u32) and +11 % (u16) instructions (profiles/r09/reduce_launch.md §0)
#pragma unroll
                for (int k = 0; k < CPL; ++k) {
                    const A key = acc_key<T>(x[k]);
                    const A kmin = m[k] ? key : hi0, kmax = m[k] ? key : lo0;
                    xm[k] = m[k] ? x[k] : T(0);
                    acc.mm.vmin[k] = kmin < acc.mm.vmin[k] ? kmin : acc.mm.vmin[k];
                    acc.mm.vmax[k] = kmax > acc.mm.vmax[k] ? kmax : acc.mm.vmax[k];
                }
            } else {
                acc.mm.fold_group(x, m);
            }
            if constexpr (MASKED) {
                if constexpr (CPL == 2) t_cnt += (m.v & 1u) + ((m.v >> 8) & 1u);
                else if constexpr (CPL == 4) t_cnt = mask_word_count(m.v, t_cnt);
                else { t_cnt = mask_word_count(m.v[0], t_cnt); t_cnt = mask_word_count(m.v[1], t_cnt); }
            }
            if constexpr (KIND == 1) {
#pragma unroll
                for (int k = 0; k < CPL; ++k) {
                    double d = static_cast<double>(x[k]) - pivot;
                    if constexpr (MASKED) d = m[k] ? d : 0.0;
                    s1[k] += d;
                    s2[k] = __builtin_fma(d, d, s2[k]);
                }
            } else if constexpr (sizeof(T) == 2) {
                // the sum two cells per instruction (v_dot2); a square already fills 32 bits, so the squares go to 64 bits at once
                // (each pair picked out of the vector by constant indices: bit_cast-ing the vector to dwords and a dword on to a pair
                // made hipcc of ROCm 7 read dword 0 four times)
                auto dot_ones = [&](auto pair) {
                    using P = decltype(pair);
                    if constexpr (SIGNED) t_sum = static_cast<uint32_t>(__builtin_amdgcn_sdot2(pair, P{1, 1}, static_cast<int>(t_sum), false));
                    else t_sum = __builtin_amdgcn_udot2(pair, P{1, 1}, t_sum, false);
                };
                dot_ones(__builtin_shufflevector(xm, xm, 0, 1));
                dot_ones(__builtin_shufflevector(xm, xm, 2, 3));
                dot_ones(__builtin_shufflevector(xm, xm, 4, 5));
                dot_ones(__builtin_shufflevector(xm, xm, 6, 7));
#pragma unroll
                for (int k = 0; k < CPL; ++k) {
                    const uint32_t v = static_cast<uint32_t>(static_cast<int32_t>(xm[k]));
                    acc.sq_lo += v * v;  // x * x mod 2^32 = x * x: at most 2^32 - 2^17 + 1
                }
            } else {
                // 4-byte cells: the sum in 64 bits, the squares (64 bits each) in 128: v_mad_u64_u32 plus the carry
#pragma unroll
                for (int k = 0; k < CPL; ++k) {
                    const int64_t v = static_cast<int64_t>(xm[k]);
                    const uint64_t q = static_cast<uint64_t>(v) * static_cast<uint64_t>(v);
                    acc.sum += v;
                    acc.sq_lo += q;
                    acc.sq_hi += acc.sq_lo < q ? 1u : 0u;
                }
            }
        }
        if constexpr (!MASKED) t_cnt += CPL;
    };

    for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const size_t base = tile * TILE + threadIdx.x;
        if (tile * TILE + TILE <= ngroups) {
            TV x[U];
            MV m[U] = {};
            policy_arms<(MASKED ? 2 : 1)>(cacheable, [&](auto bits) {  // bit 0: the cells, bit 1: the mask (ec_device.hpp)
                constexpr unsigned B = decltype(bits)::value;
#pragma unroll
                for (int j = 0; j < U; ++j) {
                    x[j] = load_cells<!(B & 1u), T, CPL>(p + (base + size_t(j) * BLOCK) * CPL);
                    if constexpr (MASKED) m[j] = load_cells<!(B & 2u), uint8_t, CPL>(mask + (base + size_t(j) * BLOCK) * CPL);
                }
            });
#pragma unroll
            for (int j = 0; j < U; ++j) fold(x[j], m[j]);
        } else {
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const size_t g = base + size_t(j) * BLOCK;
                if (g < ngroups) {
                    MV m = {};
                    if constexpr (MASKED) m = load_cells<true, uint8_t, CPL>(mask + g * CPL);
                    fold(load_cells<true, T, CPL>(p + g * CPL), m);
                }
            }
        }
        // once per tile: the 32-bit accumulators into the lane's 64-bit ones
        acc.cnt += t_cnt;
        if constexpr (KIND == 0 && sizeof(T) <= 2) {
            acc.sum += SIGNED ? static_cast<int64_t>(static_cast<int32_t>(t_sum)) : static_cast<int64_t>(t_sum);
            if constexpr (BYTES) acc.sq_lo += t_sq;
        }
        t_cnt = t_sum = t_sq = 0;
    }
    // horizontal fold of the lane's accumulators, then the ragged tail and the peeled head
    acc.mm.finish();
    if constexpr (KIND == 1) {
        acc.s1 = s1[0];
        acc.s2 = s2[0];
#pragma unroll
        for (int k = 1; k < CPL; ++k) {  // slot order
            acc.s1 += s1[k];
            acc.s2 += s2[k];
        }
    }
    if (blockIdx.x == 0) {
        auto fold_cell = [&](ptrdiff_t i) {
            if (MASKED && !ld_cell(mask + i)) return;
            acc.add(ld_cell(p + i), pivot);
        };
        for (size_t i = ngroups * CPL + threadIdx.x; i < n; i += BLOCK) fold_cell(static_cast<ptrdiff_t>(i));
        for (unsigned h = threadIdx.x; h < head; h += BLOCK) fold_cell(-static_cast<ptrdiff_t>(h) - 1);  // the peeled cells
    }
    Moments r = acc.partial();
    if (block_fold<BLOCK>(r, FoldMoments<KIND>{})) {
        if (record_if_single) write_record<T>(record_if_single, r, pivot);
        else partials[blockIdx.x] = r;
    }
}

// Same reduction, cell-wise loads: any alignment (the plan's other outcome, "unaligned_vector" off).
template <typename T, bool MASKED>
__global__ __launch_bounds__(kBlock) void k_stats_partials_cellwise(const T* __restrict__ p, const uint8_t* __restrict__ mask,
                                                                    size_t n, Moments* __restrict__ partials) {
    const double pivot = stats_pivot<T>(p);
    CellMoments<T, MASKED> acc;
    acc.init();
    const size_t stride = size_t(gridDim.x) * kBlock;
    for (size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
        if (MASKED && !mask[i]) continue;
        acc.add(p[i], pivot);
    }
    Moments r = acc.partial();
    if (block_fold<kBlock>(r, FoldMoments<StatsKind<T>::value>{})) partials[blockIdx.x] = r;
}

// One workgroup folds the partials in a fixed order and writes the record; nparts == 0 (n == 0) writes the empty record.
// first_cell_or_null: the buffer's first cell, for the pivot the partials were taken against.  The block fold is the frame's,
// but over 256 threads, not finalize_fold's 1024: a Moments is 12 registers, and under the 128 VGPRs of a 1024-thread workgroup
// both finalize_fold's four partials per thread and block_fold's fifteen wave results in thread 0 spilled to scratch for the
// f64 kind.  A thread takes every 256th partial, four loads in flight (a device's four workgroups per CU: four partials each).
constexpr int kStatsFinalizeBlock = 256;
template <typename T>
__global__ __launch_bounds__(kStatsFinalizeBlock) void k_stats_finalize(const Moments* __restrict__ partials, int nparts,
                                                                         const T* __restrict__ first_cell_or_null,
                                                                         ec_moments* __restrict__ record) {
    const FoldMoments<StatsKind<T>::value> op;
    Moments acc = moments_identity<T>();
#pragma unroll 4
    for (int i = threadIdx.x; i < nparts; i += kStatsFinalizeBlock) acc = op(acc, partials[i]);
    if (block_fold<kStatsFinalizeBlock>(acc, op)) write_record<T>(record, acc, first_cell_or_null ? stats_pivot<T>(first_cell_or_null) : 0.0);
}

}  // namespace ecd
