// ec_focal_rank_cell.hpp — one cell of ec_focal_rank / ec_focal_majority (include/erased_cells.h): the taps of a cell's footprint as
// the words of ec_composite_rank_cell.hpp — rank_word<T>::make(cell, is-a-tap, k), k the tap's row-major position in the footprint
// (k <= 63) — sorted by rank_sort, and one of them kept:
//
//   rank_pick(w, rank_of_count(r, count))   the tap at position r(count): ec_focal_rank.  Taps of equal key have equal bits, so the
//                                           k that breaks ties in the sort cannot reach the result
//   majority_pick<T, N>(w, count)           the key that occurs most often, the least of those that tie: ec_focal_majority
//
// rank_word, rank_sort, rank_pick, rank_of_count and RankTable are used as they are.  The sentinel of a cell that is no tap sorts
// above every valid word (k = 255 > 63), also above a u64 maximum and an all-ones NaN, so the `count` taps stand first.
//
// Self-contained like its siblings: no HIP runtime include, host/test_focal_rank_cell.cpp runs it under a plain C++ compiler.
#pragma once

#include <stdint.h>

#include "ec_composite_rank_cell.hpp"

namespace ecd {

constexpr int kFocalRankMaxTaps = 64;  // EC_FOCAL_RANK_MAX_TAPS: what one sorting network holds
static_assert(kFocalRankMaxTaps == kCompositeMaxLayers, "the networks and the table r(c) are ec_composite_rank's");

// the network a footprint of `taps` cells is sorted by: 1, 4, 8, 16, 32 or 64 (a footprint has an odd number of cells, so never 2)
constexpr int focal_rank_bucket(uint32_t taps) { return rank_bucket(int(taps)); }

// do two words hold the same key?  (k aside: equal keys are equal bits of the cell.)  The sentinel of an 8-byte cell has the key of a
// u64 maximum or an all-ones NaN: majority_pick never asks about a position that is no tap.
template <typename T>
EC_HD bool rank_same_key(typename rank_word<T>::type a, typename rank_word<T>::type b) {
    if constexpr (sizeof(T) == 8) return a.key == b.key;
    else return (a >> 8) == (b >> 8);
}

// The word of the most frequent key among the first `count` of N sorted words; among keys of equal greatest frequency the least.
// One pass, every index a constant: the run length restarts where the key changes, and the running best is replaced only by a
// STRICTLY longer run, so the first — the least — of several longest runs stays.  Only positions j < count are looked at: the
// sentinels behind them never extend or form a run.  count == 0 returns w[0], a sentinel: the cell is invalid and stores nothing of it.
template <typename T, int N>
EC_HD typename rank_word<T>::type majority_pick(const typename rank_word<T>::type (&w)[N], uint32_t count) {
    typename rank_word<T>::type best = w[0];
    uint32_t best_len = 1, run = 1;
    EC_UNROLL
    for (int j = 1; j < N; ++j) {
        run = rank_same_key<T>(w[j], w[j - 1]) ? run + 1 : 1;
        const bool take = uint32_t(j) < count && run > best_len;
        best = rank_select<T>(take, w[j], best);
        best_len = take ? run : best_len;
    }
    return best;
}

// the cell's bits from the word picked: valid iff count > 0, or count == full under EC_FOCAL_WHOLE (`need` is 1 or full)
template <typename T>
EC_HD T focal_rank_finish(typename rank_word<T>::type picked, uint32_t count, uint32_t need, bool* valid) {
    const bool ok = count >= need;  // need >= 1: a cell without a tap, whose pick is a sentinel, is never ok
    *valid = ok;
    return ok ? rank_word<T>::value(picked) : T(0);
}

}  // namespace ecd
