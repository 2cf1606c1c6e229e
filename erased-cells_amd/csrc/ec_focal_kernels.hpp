// ec_focal_kernels.hpp — moving-window operations on a raster resident in HBM (gfx950): k_focal<T, MASKED, KIND> (sum / mean and
// min / max) and k_focal_convolve<T, MASKED>.  The rule is the one stated at ec_focal in include/erased_cells.h: taps in row-major
// order, one partial sum per footprint row, individually rounded f64 steps (the translation unit is built with -ffp-contract=off: no
// FMA), one right answer per cell.  The first kernels of the library with reuse between lanes: every other one reads each byte once.
//
// ONE WORKGROUP PER OUTPUT TILE of TW x TH cells, 256 lanes, two fronts (two_front_tile), tiles numbered row-major.
//   1. STAGE  the tile and its halo of rx columns and ry rows, cut to the raster (ecf::tile_at), go to LDS: cells as they are, and the
//      mask bytes of a MASKED launch.  A staged row is contiguous in the raster, so it moves as under-aligned 16-byte global loads (row
//      starts fall on every alignment; ec_window_kernels.hpp) into 16-byte-aligned LDS stores — every LDS row starts at a multiple of
//      16 (ecf::layout_of) — and its last bytes cell by cell.  Loads run under the launch's cache_plan bits (bit 0 cells, bit 1 mask).
//   2. one barrier.
//   3. SEPARABLE kinds (sum / mean, min / max): a HORIZONTAL pass gives every staged row and output column its row result — racc of
//      the rule, which does not depend on the output row, or the row's least / greatest order key — and, when masked, its tap count, in
//      LDS; a barrier; the VERTICAL pass folds 2 ry + 1 of them per output cell in ascending rows.  For sums that IS the rule's order, at
//      2 (2 r + 1) additions per cell in place of (2 r + 1)^2; order keys fold exactly in any order.
//      CONVOLUTION: the rule's double loop per output cell; the weights are kernel arguments, indexed by the loop counters alone, so
//      they are scalar loads.
//   Then each lane owns 16-byte output slots (16 / 8 f64 results, 16 / W cells for min / max) of one tile row: nt_store for a whole
//   slot with one mask_store of its 16 / W' mask bytes beside it (as k_window_resample), cell-wise stores for the last cells of a
//   raster row and for every slot when `cellwise_stores` is set.
//
// CLIPPING.  Staged cell (ly, lx) is raster cell (ys + ly, xs + lx), and a footprint cell lies inside the raster exactly when its staged
// coordinates lie in [0, sh) x [0, sw): one unsigned compare per axis, no wrap into a neighbouring row.  A cell that is no tap is read
// from staged cell 0 of its row instead and dropped by a select, so what it holds — a NaN included — leaves no trace and no lane
// reads outside the stage.
//
// LDS BANKS (cdna_hip_programming.md §2; DESIGN.md "Moving windows" has the arithmetic).  TW is one wave: in the horizontal pass the
// 64 lanes of a wave read 64 neighbouring cells of ONE staged row, so the row pitch never enters — 4-byte cells are 32 neighbouring
// dwords per 32-lane half, 8-byte cells 64 neighbouring banks of ds_read_b64, and 1- and 2-byte cells are read as the dword that
// holds them (4 or 2 lanes share an address: a broadcast) and unpacked with shifts.  Row results are as wide as the output cell (an f64
// sum, or an order key of the cell's own width), so in the vertical pass a lane's slot of them is ONE aligned 16-byte read and
// neighbouring lanes read neighbouring 16 bytes: conflict-free for ds_read_b128 at every width.
//
// Radii are run-time values: kernels are instantiated by cell type x masked x kind only, and the stage is dynamic LDS sized per launch.
#pragma once

#include "ec_focal_plan.hpp"
#include "ec_tile.hpp"

namespace ecd {

constexpr int TW = 64;  // output cells per tile row: one wave
constexpr int TH = 16;  // output rows per tile.  At radius 7 with 8-byte cells and a mask the stage is 38400 bytes (ecf::layout_of)

struct FocalArgs {
    const void* src;
    void* dst;
    const uint8_t* src_mask;
    uint8_t* dst_mask;  // may be null for an unmasked launch without EC_FOCAL_WHOLE
    uint64_t cols, rows;
    uint32_t tiles_x;
    uint32_t rx, ry;
    uint32_t op;     // an ec_focal_op (the separable kinds)
    uint32_t flags;  // EC_FOCAL_WHOLE, EC_FOCAL_NORMALIZE
    uint32_t cacheable;
    uint32_t cellwise_stores;  // "unaligned_vector" is off and a slot of the output can start off a 16-byte boundary
    ecf::Layout lds;
    uint32_t first_tile = 0;  // this launch covers the tiles [first_tile, first_tile + gridDim.x) of the raster (split_launch, ec_runtime.hpp)
};
// What every moving-window entry point does between its refusals and its dispatch (ec_focal.hip; ec_focal_rank.hip calls it too): the
// dtype, the empty raster, the device, then *a with its cache plan and store form — or a status that ends the call (*done).
ec_status focal_args(const char* what, ec_dtype t, const void* src, const uint8_t* src_mask, uint64_t cols, uint64_t rows, uint32_t rx, uint32_t ry,
                     uint32_t op, uint32_t flags, void* dst, uint8_t* dst_mask, const ecf::Layout& lds, const ecf::Grid& g, FocalArgs* a, bool* done);
struct FocalWeights {
    double w[(2 * EC_FOCAL_RADIUS_CAP + 1) * (2 * EC_FOCAL_RADIUS_CAP + 1)];
};

extern __shared__ __attribute__((aligned(16))) unsigned char focal_lds[];

// cell lx of a staged row; 1- and 2-byte cells as the dword that holds them
template <typename T>
__device__ __forceinline__ T staged_cell(const unsigned char* row, uint32_t lx) {
    if constexpr (sizeof(T) >= 4) {
        return reinterpret_cast<const T*>(row)[lx];
    } else {
        const uint32_t w = reinterpret_cast<const uint32_t*>(row)[(lx * uint32_t(sizeof(T))) >> 2];
        using C = typename width_cell<sizeof(T)>::type;
        if constexpr (sizeof(T) == 1) return __builtin_bit_cast(T, C((w >> (8 * (lx & 3u))) & 0xffu));
        else return __builtin_bit_cast(T, C((w >> (16 * (lx & 1u))) & 0xffffu));
    }
}

// step 1: rows of `row_bytes` bytes, `pitch` bytes apart in global memory, into LDS rows `lds_pitch` apart; cells of W bytes
template <int W, bool NT>
__device__ __forceinline__ void focal_stage_rows(const unsigned char* __restrict__ g, uint64_t pitch, uint32_t rows, uint32_t row_bytes,
                                                 unsigned char* lds, uint32_t lds_pitch) {
    using C = typename width_cell<W>::type;
    const uint32_t per_row = (row_bytes + 15u) >> 4, n = rows * per_row;
#pragma unroll 1
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
        const uint32_t ly = i / per_row, b = (i - ly * per_row) << 4;
        const unsigned char* from = g + uint64_t(ly) * pitch + b;
        unsigned char* to = lds + ly * lds_pitch + b;
        if (b + 16u <= row_bytes) {
            *reinterpret_cast<u32x4*>(to) = load_vec<NT>(reinterpret_cast<const u32x4*>(from));
        } else {
#pragma unroll 1
            for (uint32_t k = 0; b + k < row_bytes; k += W)
                *reinterpret_cast<C*>(to + k) = ld_cell(reinterpret_cast<const C*>(from + k));
        }
    }
}

template <typename T, bool MASKED>
__device__ __forceinline__ void focal_stage(const FocalArgs& a, const ecf::Tile& t) {
    constexpr int W = sizeof(T);
    const uint64_t first = t.ys * a.cols + t.xs;
    const unsigned char* cells = static_cast<const unsigned char*>(a.src) + first * W;
    policy_arms<MASKED ? 2 : 1>(a.cacheable, [&](auto bits) {
        constexpr unsigned B = decltype(bits)::value;
        focal_stage_rows<W, !(B & 1u)>(cells, a.cols * W, t.sh, t.sw * W, focal_lds, a.lds.cell_pitch);
        if constexpr (MASKED) focal_stage_rows<1, !(B & 2u)>(a.src_mask + first, a.cols, t.sh, t.sw, focal_lds + a.lds.off_mask, a.lds.mask_pitch);
    });
}

__device__ __forceinline__ ecf::Tile focal_this_tile(const FocalArgs& a) {
    const uint32_t tile = uint32_t(two_front_tile(a.first_tile)), ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    return ecf::tile_at(a.cols, a.rows, a.rx, a.ry, tx, ty, TW, TH);
}

// What a lane does with the CPL results of one output slot: `bits[k]` and `valid[k]` of the `cells` cells from column j0 of tile row oy.
// The mask word and the store pair of a whole slot are the ones k_window_resample uses (SlotMask, slot_store_pair: ec_tile.hpp).  The
// two branches stay here, reading `a` where they need it: behind one more call that takes the mask pointer and the cell-wise flag by
// value the 1-byte rank kernels held 42 VGPRs in place of 34 (profiles/window/frame.md).
template <int OW, int CPL>
__device__ __forceinline__ void focal_store_slot(const FocalArgs& a, const ecf::Tile& t, uint32_t oy, uint32_t j0, uint32_t cells,
                                                 const uint64_t (&bits)[CPL], const bool (&valid)[CPL]) {
    using C = typename width_cell<OW>::type;
    const uint64_t at = (t.y0 + oy) * a.cols + t.x0 + j0;
    C* dst = static_cast<C*>(a.dst) + at;
    if (cells == uint32_t(CPL) && !a.cellwise_stores) {
        u32x4 v{0, 0, 0, 0};
        SlotMask m;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            slot_put<OW>(v, k, C(valid[k] ? bits[k] : 0));
            m.put(k, valid[k]);
        }
        slot_store_pair<CPL>(v, m, static_cast<C*>(a.dst), a.dst_mask, at);
    } else {
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            if (uint32_t(k) < cells) {
                st_cell(C(valid[k] ? bits[k] : 0), dst + k);
                if (a.dst_mask) st_cell(uint8_t(valid[k]), a.dst_mask + at + k);
            }
        }
    }
}

// The order key of a cell in as many bits as the cell has, for an UNSIGNED compare: order_key (ec_order_key.hpp) cut to the cell's
// width, its top bit turned where the key is signed.  Row results of min / max are W bytes wide like the output, so a lane's slot
// of them is 16 contiguous bytes of LDS, as a slot of row sums is.
template <typename T>
struct focal_key {
    static constexpr int W = sizeof(T);
    using C = typename width_cell<W>::type;
    static constexpr bool plain = !is_fp<T>::value && T(-1) > T(0) && W < 8;  // u8, u16, u32: the key is the cell
    static constexpr uint64_t top = uint64_t(1) << (8 * W - 1);
    static __device__ __forceinline__ C of(T v) {
        const C k = C(uint64_t(order_key(v)));
        return plain ? k : C(k ^ C(top));
    }
    static __device__ __forceinline__ T cell(C u) {
        if constexpr (plain) {
            return key_value<T>(int64_t(u));
        } else {
            const uint64_t x = uint64_t(C(u ^ C(top)));
            return key_value<T>(int64_t(x << (64 - 8 * W)) >> (64 - 8 * W));  // sign-extended
        }
    }
};

// ---- sum / mean (KIND = ecf::kSeparableSum, f64 results) and min / max (ecf::kSeparableMinMax, results of type T)
template <typename T, bool MASKED, int KIND>
__global__ __launch_bounds__(kBlock) void k_focal(FocalArgs a) {
    constexpr bool SUM = KIND == ecf::kSeparableSum;
    constexpr int OW = SUM ? 8 : int(sizeof(T)), CPL = 16 / OW, SPR = TW / CPL;  // cells per slot, slots per tile row
    using R = typename width_cell<OW>::type;   // a row result: the bits of an f64 sum, or a focal_key
    using M = typename byte_words<CPL>::type;  // the tap counts of one slot's columns
    const ecf::Tile t = focal_this_tile(a);
    focal_stage<T, MASKED>(a, t);
    __syncthreads();

    const R flip = a.op == EC_FOCAL_MIN ? R(~R(0)) : R(0);  // the minimum is the maximum of the complemented key, as in ec_min_max
    R* racc = reinterpret_cast<R*>(focal_lds + a.lds.off_racc);
    uint8_t* rcnt = focal_lds + a.lds.off_rcnt;  // MASKED only: without a mask a row's tap count is the clip's (below)
    const int32_t lx_first = int32_t(t.x0 - t.xs) - int32_t(a.rx), ly_first = int32_t(t.y0 - t.ys) - int32_t(a.ry);
    const uint32_t nx = 2 * a.rx + 1, ny = 2 * a.ry + 1;

    // horizontal: one staged row per wave and step, lane = output column
#pragma unroll 1
    for (uint32_t i = threadIdx.x; i < t.sh * uint32_t(TW); i += kBlock) {
        const uint32_t ly = i / uint32_t(TW), j = i % uint32_t(TW);
        if (j >= t.ow) continue;
        const unsigned char* row = focal_lds + ly * a.lds.cell_pitch;
        const uint8_t* mrow = focal_lds + a.lds.off_mask + ly * a.lds.mask_pitch;
        double sum = 0.0;
        R best = 0;
        uint32_t cnt = 0;
#pragma unroll 1
        for (uint32_t dx = 0; dx < nx; ++dx) {
            const int32_t lx = lx_first + int32_t(j) + int32_t(dx);
            bool tap = uint32_t(lx) < t.sw;
            const uint32_t at = tap ? uint32_t(lx) : 0u;
            if constexpr (MASKED) tap = tap && mrow[at] != 0;
            const T c = staged_cell<T>(row, at);
            if constexpr (SUM) {
                const double next = sum + to_f64(c);
                sum = tap ? next : sum;
            } else {
                const R k = R(focal_key<T>::of(c) ^ flip);
                best = tap && k > best ? k : best;
            }
            if constexpr (MASKED) cnt += tap ? 1u : 0u;
        }
        if constexpr (SUM) racc[i] = f64_bits(sum);
        else racc[i] = best;
        if constexpr (MASKED) rcnt[i] = uint8_t(cnt);
    }
    __syncthreads();

    // vertical: each lane folds the row results of its slots' columns in ascending rows; a slot's CPL row results are 16 contiguous,
    // 16-byte-aligned bytes of LDS (one ds_read_b128, lanes 16 bytes apart), its counts CPL bytes.
    // A tile has TH * SPR slots: 512 for f64 results (two per lane), but 256 for 4-byte, 128 for 2-byte and only 64 for 1-byte min / max —
    // there a quarter of the workgroup works behind this barrier, each lane through its slot's 16 columns one after the other (u8 MIN 3 x 3:
    // 0.094 of 8 TB/s, profiles/focal/focal.md).  Folding narrow cells several columns per lane-step, or handing the vertical pass columns
    // instead of slots and gathering the slots through LDS, is the next thing to try here.
    const uint32_t full = nx * ny;
#pragma unroll 1
    for (uint32_t s = threadIdx.x; s < uint32_t(TH * SPR); s += kBlock) {
        const uint32_t oy = s / uint32_t(SPR), j0 = (s % uint32_t(SPR)) * CPL;
        if (oy >= t.oh || j0 >= t.ow) continue;
        const uint32_t cells = t.ow - j0 < uint32_t(CPL) ? t.ow - j0 : uint32_t(CPL);
        double acc[CPL];
        R best[CPL];
        uint32_t count[CPL], in_row[CPL];
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            acc[k] = 0.0;
            best[k] = 0;
            count[k] = 0;
            // the columns of column j0 + k's footprint that lie inside the raster: staged columns [lo, hi]
            const int32_t lo = lx_first + int32_t(j0) + k, hi = lo + int32_t(nx) - 1;
            in_row[k] = uint32_t((hi < int32_t(t.sw) ? hi : int32_t(t.sw) - 1) - (lo > 0 ? lo : 0) + 1);
        }
#pragma unroll 1
        for (uint32_t dy = 0; dy < ny; ++dy) {
            const int32_t ly = ly_first + int32_t(oy) + int32_t(dy);
            const bool in = uint32_t(ly) < t.sh;
            const uint32_t at = (in ? uint32_t(ly) : 0u) * uint32_t(TW) + j0;
            const u32x4 r = *reinterpret_cast<const u32x4*>(racc + at);
            M cm{};
            if constexpr (MASKED) cm = *reinterpret_cast<const M*>(rcnt + at);
#pragma unroll
            for (int k = 0; k < CPL; ++k) {  // columns past t.ow hold nothing written; their results are never stored
                const uint32_t c = MASKED ? mask_word_byte<CPL>(cm, k) : in_row[k];
                if constexpr (SUM) {
                    const double next = acc[k] + bits_f64(slot_get<8>(r, k));
                    acc[k] = in ? next : acc[k];
                } else {
                    const R v = slot_get<OW>(r, k);
                    best[k] = in && c != 0 && v > best[k] ? v : best[k];
                }
                count[k] += in ? c : 0u;
            }
        }
        uint64_t bits[CPL];
        bool valid[CPL];
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            valid[k] = (a.flags & EC_FOCAL_WHOLE) ? count[k] == full : count[k] != 0;
            if constexpr (SUM) bits[k] = f64_bits(acc[k]);
            else bits[k] = uint64_t(__builtin_bit_cast(R, focal_key<T>::cell(R(best[k] ^ flip))));
        }
        if constexpr (SUM) {
            if (a.op == EC_FOCAL_MEAN) {  // launch-uniform: a sum pays for no division
#pragma unroll
                for (int k = 0; k < CPL; ++k) bits[k] = f64_bits(acc[k] / static_cast<double>(count[k]));
            }
        }
        focal_store_slot<OW, CPL>(a, t, oy, j0, cells, bits, valid);
    }
}

// ---- convolution (correlation: weight [dy][dx] meets cell (i - ry + dy, j - rx + dx)), f64 results
template <typename T, bool MASKED>
__global__ __launch_bounds__(kBlock) void k_focal_convolve(FocalArgs a, FocalWeights w) {
    constexpr int CPL = 2, SPR = TW / CPL;
    const ecf::Tile t = focal_this_tile(a);
    focal_stage<T, MASKED>(a, t);
    __syncthreads();
    const int32_t lx_first = int32_t(t.x0 - t.xs) - int32_t(a.rx), ly_first = int32_t(t.y0 - t.ys) - int32_t(a.ry);
    const uint32_t nx = 2 * a.rx + 1, ny = 2 * a.ry + 1, full = nx * ny;
#pragma unroll 1
    for (uint32_t s = threadIdx.x; s < uint32_t(TH * SPR); s += kBlock) {
        const uint32_t oy = s / uint32_t(SPR), j0 = (s % uint32_t(SPR)) * CPL;
        if (oy >= t.oh || j0 >= t.ow) continue;
        const uint32_t cells = t.ow - j0 < uint32_t(CPL) ? t.ow - j0 : uint32_t(CPL);
        double acc[CPL] = {0.0, 0.0}, wsum[CPL] = {0.0, 0.0};
        uint32_t count[CPL] = {0, 0};
#pragma unroll 1
        for (uint32_t dy = 0; dy < ny; ++dy) {
            const int32_t ly = ly_first + int32_t(oy) + int32_t(dy);
            const bool in = uint32_t(ly) < t.sh;
            const uint32_t sy = in ? uint32_t(ly) : 0u;
            const unsigned char* row = focal_lds + sy * a.lds.cell_pitch;
            const uint8_t* mrow = focal_lds + a.lds.off_mask + sy * a.lds.mask_pitch;
            double racc[CPL] = {0.0, 0.0}, rw[CPL] = {0.0, 0.0};
#pragma unroll 1
            for (uint32_t dx = 0; dx < nx; ++dx) {
                const double weight = w.w[dy * nx + dx];  // the same for every lane: a scalar load
#pragma unroll
                for (int k = 0; k < CPL; ++k) {
                    const int32_t lx = lx_first + int32_t(j0) + k + int32_t(dx);
                    bool tap = in && uint32_t(lx) < t.sw;
                    const uint32_t at = tap ? uint32_t(lx) : 0u;
                    if constexpr (MASKED) tap = tap && mrow[at] != 0;
                    const double term = weight * to_f64(staged_cell<T>(row, at));
                    const double next = racc[k] + term, wnext = rw[k] + weight;
                    racc[k] = tap ? next : racc[k];
                    rw[k] = tap ? wnext : rw[k];
                    count[k] += tap ? 1u : 0u;
                }
            }
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                acc[k] = acc[k] + racc[k];
                wsum[k] = wsum[k] + rw[k];
            }
        }
        uint64_t bits[CPL];
        bool valid[CPL];
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            valid[k] = (a.flags & EC_FOCAL_WHOLE) ? count[k] == full : count[k] != 0;
            double r = acc[k];
            if (a.flags & EC_FOCAL_NORMALIZE) {
                valid[k] = valid[k] && !(wsum[k] == 0.0);
                r = acc[k] / wsum[k];
            }
            bits[k] = f64_bits(r);
        }
        focal_store_slot<8, CPL>(a, t, oy, j0, cells, bits, valid);
    }
}

}  // namespace ecd
