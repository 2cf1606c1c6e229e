// ec_focal_rank_kernels.hpp — ec_focal_rank and ec_focal_majority (include/erased_cells.h) on gfx950: the order statistics of a
// moving window.  k_focal_rank<T, KB> joins the two halves the library had: the tile-and-halo stage of k_focal (ec_focal_kernels.hpp)
// and the register-resident sorting network of k_composite_rank (ec_composite_rank_cell.hpp), through ec_focal_rank_cell.hpp.
//
// ONE WORKGROUP PER OUTPUT TILE of TW x TH cells, the frame of k_focal:
//   1. STAGE  focal_stage: the tile and its halo, cut to the raster, and the mask bytes of a masked launch go to LDS under the launch's
//      cache_plan bits.  The layout is ecf::rank_layout_of: cells and mask bytes, no row results.
//   2. a barrier.
//   3. SORT   lane = output column, wave = output row (TW is one wave; a wave takes rows w, w + 4, ..): the lane GATHERS the taps of its
//      cell from LDS into KB words, KB the footprint's size rounded up to a power of two (1, 4, 8, 16, 32, 64), sorts them with
//      rank_sort and keeps rank_pick(r(count)) or majority_pick — a launch-uniform branch behind the one sort.  A lane has one cell in
//      flight: its KB words are all the registers the largest network leaves (DESIGN.md "Order statistics of a moving window").
//   4. The cell's bits and its validity byte go to LDS, and behind a second barrier each lane owns 16-byte output slots as in
//      k_focal's vertical pass: one aligned 16-byte read of LDS, then focal_store_slot — nt_store and one mask_store, or cell-wise
//      under `cellwise_stores`.
//   Steps 3 and 4 are columns-then-slots, not "a lane sorts the cells of its own slot": a slot is 16 / W cells, so with slots only
//   a quarter of the lanes would sort 1-byte cells (the gap k_focal's vertical pass names), and neighbouring lanes would read LDS 16
//   bytes apart.  This way every lane sorts, whatever the cell width.
//
// THE GATHER.  Radii are run-time values, yet every index into the words is a constant: an unrolled loop over b = 0 .. KB - 1 in
// which (dy, dx) advance as wave-uniform counters (dx++, wrap at 2 rx + 1), so b is the tap's row-major position in the footprint,
// the k of its word.  b >= taps is a wave-uniform branch that makes a sentinel, never an LDS read.  A footprint cell outside the
// stage is k_focal's clip — staged cell 0 of the row is read instead and the cell dropped by a select, as is a masked-out one —
// so no lane reads outside the stage and what a dropped cell holds leaves no trace.
//
// LDS BANKS (cdna_hip_programming.md §2).  At each step of the gather the 64 lanes of a wave read 64 neighbouring cells of ONE staged
// row (column j + dx), as in k_focal's horizontal pass: 4-byte cells are neighbouring dwords, 8-byte cells neighbouring
// ds_read_b64, 1- and 2-byte cells the dword that holds them (a broadcast within 4 or 2 lanes).  Results are written one row per
// wave, W bytes a lane, and read back as aligned 16-byte slots, lanes 16 bytes apart.
//
// `masked` (a.src_mask) and the operation (a.op) are launch-uniform branches: kernels are instantiated by cell type x KB only.
#pragma once

#include "ec_focal_kernels.hpp"
#include "ec_focal_rank_cell.hpp"

namespace ecd {

enum : uint32_t { kFocalRankPick = 0, kFocalRankMajority = 1 };  // FocalArgs::op of these kernels

template <typename T, int KB>
__global__ __launch_bounds__(kBlock) void k_focal_rank(FocalArgs a, RankTable rank) {
    constexpr int W = sizeof(T), CPL = 16 / W, SPR = TW / CPL;
    using C = typename width_cell<W>::type;
    using M = typename byte_words<CPL>::type;
    using Word = typename rank_word<T>::type;
    const ecf::Tile t = focal_this_tile(a);
    const bool masked = a.src_mask != nullptr;
    if (masked) focal_stage<T, true>(a, t);
    else focal_stage<T, false>(a, t);
    __syncthreads();

    const int32_t lx_first = int32_t(t.x0 - t.xs) - int32_t(a.rx), ly_first = int32_t(t.y0 - t.ys) - int32_t(a.ry);
    const uint32_t nx = 2 * a.rx + 1, taps = nx * (2 * a.ry + 1);
    const uint32_t need = (a.flags & EC_FOCAL_WHOLE) ? taps : 1u;
    C* res = reinterpret_cast<C*>(focal_lds + a.lds.off_racc);
    uint8_t* res_valid = focal_lds + a.lds.off_rcnt;

#pragma unroll 1
    for (uint32_t i = threadIdx.x; i < uint32_t(TH * TW); i += kBlock) {
        // TW is one wave, so a wave's lanes share oy: pinned to a scalar register, the row addresses and (dy, dx) are scalar too
        const uint32_t oy = uint32_t(__builtin_amdgcn_readfirstlane(int(i / uint32_t(TW)))), j = i % uint32_t(TW);
        if (oy >= t.oh || j >= t.ow) continue;
        Word w[KB];
        uint32_t count = 0, dx = 0;
        int32_t ly = ly_first + int32_t(oy);
#pragma unroll
        for (int b = 0; b < KB; ++b) {
            if (uint32_t(b) < taps) {
                const bool in = uint32_t(ly) < t.sh;
                const uint32_t sy = in ? uint32_t(ly) : 0u;
                const int32_t lx = lx_first + int32_t(j) + int32_t(dx);
                bool tap = in && uint32_t(lx) < t.sw;
                const uint32_t at = tap ? uint32_t(lx) : 0u;
                if (masked) tap = tap && focal_lds[a.lds.off_mask + sy * a.lds.mask_pitch + at] != 0;
                const T c = staged_cell<T>(focal_lds + sy * a.lds.cell_pitch, at);
                w[b] = rank_word<T>::make(c, tap, uint32_t(b));
                count += tap ? 1u : 0u;
                if (++dx == nx) {
                    dx = 0;
                    ++ly;
                }
            } else {
                w[b] = rank_word<T>::make(T(0), false, uint32_t(b));
            }
        }
        rank_sort<T, KB>(w);
        Word picked;
        if (a.op == kFocalRankPick) picked = rank_pick<T, KB>(w, rank_of_count<KB>(rank.r, count));
        else picked = majority_pick<T, KB>(w, count);
        bool valid;
        const T r = focal_rank_finish<T>(picked, count, need, &valid);
        res[i] = __builtin_bit_cast(C, r);
        res_valid[i] = valid ? 1 : 0;
    }
    __syncthreads();

#pragma unroll 1
    for (uint32_t s = threadIdx.x; s < uint32_t(TH * SPR); s += kBlock) {
        const uint32_t oy = s / uint32_t(SPR), j0 = (s % uint32_t(SPR)) * CPL;
        if (oy >= t.oh || j0 >= t.ow) continue;
        const uint32_t cells = t.ow - j0 < uint32_t(CPL) ? t.ow - j0 : uint32_t(CPL);
        const uint32_t at = oy * uint32_t(TW) + j0;
        const u32x4 r = *reinterpret_cast<const u32x4*>(res + at);
        const M vm = *reinterpret_cast<const M*>(res_valid + at);
        uint64_t bits[CPL];
        bool valid[CPL];
#pragma unroll
        for (int k = 0; k < CPL; ++k) {  // columns past t.ow hold nothing written; their results are never stored
            bits[k] = uint64_t(slot_get<W>(r, k));
            valid[k] = mask_word_byte<CPL>(vm, k) != 0;
        }
        focal_store_slot<W, CPL>(a, t, oy, j0, cells, bits, valid);
    }
}

}  // namespace ecd
