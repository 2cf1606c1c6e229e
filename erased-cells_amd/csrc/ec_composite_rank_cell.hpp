// ec_composite_rank_cell.hpp — one cell of ec_composite_rank (include/erased_cells.h): the valid layers of a cell's stack in ascending
// order of the pair (order_key(cell), k), and the one at position r(count) kept.  The rule is the header's; this is its only
// statement in code:
//
//   rank_position / rank_table   r(c) for c = 1 .. 64 from (num, den, method): integer arithmetic, on the host, once per call
//   rank_word<T>                 a layer's cell as one unsigned word that sorts as the pair does: (biased key << 8 | k) in 32 bits
//                                for 1- and 2-byte cells, in 64 bits for 4-byte cells, a (key, k) pair compared lexicographically
//                                for 8-byte cells.  A layer that is not valid is the sentinel (all ones, k = 255): above every valid
//                                word, since k <= 63 — also above a u64 maximum and an all-ones positive NaN
//   rank_sort<T, N>              a bitonic network of N = 2^m words, every comparator ascending, every index a constant
//   rank_pick<T, N>              the word at position r by a select chain (a dynamic index would put the words in memory)
//   rank_finish<T>               valid iff count >= min_count; the value (key_value of the word's key: the transform is a bijection on
//                                bits, NaN payloads come through), the mask byte and the aux byte of the cell
//
// Self-contained like ec_composite_cell.hpp: no HIP runtime include, host/test_composite_rank_cell.cpp runs it under a plain C++ compiler.
#pragma once

#include <stdint.h>

#include "ec_composite_cell.hpp"

#if defined(__clang__)
#define EC_UNROLL _Pragma("unroll")
#else
#define EC_UNROLL
#endif

namespace ecd {

// ec_rank_method (erased_cells.h)
constexpr int kRankLower = 0, kRankUpper = 1;
constexpr uint32_t kRankMaxDen = 65535;

constexpr bool valid_rank_method(int m) { return m == kRankLower || m == kRankUpper; }
constexpr bool valid_rank_fraction(uint32_t num, uint32_t den) { return den >= 1 && den <= kRankMaxDen && num <= den; }

// the position kept among c valid layers (1 <= c <= 64): num * (c - 1) <= 65535 * 63, so 32 bits hold everything
constexpr uint32_t rank_position(uint32_t num, uint32_t den, int method, uint32_t c) {
    return method == kRankUpper ? (num * (c - 1) + den - 1) / den : (num * (c - 1)) / den;
}

// r(c) for every count; entry 0 is never read (a cell without a valid layer stores nothing of the stack)
struct RankTable {  // a word per entry: in the kernel's argument block every entry is then one aligned scalar load
    uint32_t r[kCompositeMaxLayers + 1];
};
inline RankTable rank_table(uint32_t num, uint32_t den, int method) {
    RankTable t;
    t.r[0] = 0;
    for (uint32_t c = 1; c <= uint32_t(kCompositeMaxLayers); ++c) t.r[c] = rank_position(num, den, method, c);
    return t;
}

// the least power of two that holds k layers: the network a stack of k layers is sorted by
constexpr int rank_bucket(int k) { return k <= 1 ? 1 : 2 * rank_bucket((k + 1) / 2); }

struct RankPair {  // 8-byte cells
    uint64_t key;
    uint32_t k;
};

template <typename T, int BYTES = sizeof(T)>
struct rank_word {  // 1- and 2-byte cells: key + 2^15 is 0 .. 98303, 17 bits
    using type = uint32_t;
    static EC_HD type make(T v, bool valid, uint32_t k) {
        const uint32_t w = static_cast<uint32_t>(static_cast<int32_t>(order_key<T>(v)) + 32768) << 8 | k;
        return valid ? w : ~uint32_t(0);
    }
    static EC_HD bool less(type a, type b) { return a < b; }
    static EC_HD uint32_t layer(type w) { return w & 0xffu; }
    static EC_HD T value(type w) { return key_value<T>(static_cast<int64_t>(static_cast<int32_t>(w >> 8) - 32768)); }
};
template <typename T>
struct rank_word<T, 4> {  // key + 2^31 is 0 .. 2^32 + 2^31 - 1, 33 bits
    using type = uint64_t;
    static EC_HD type make(T v, bool valid, uint32_t k) {
        const uint64_t w = static_cast<uint64_t>(order_key<T>(v) + (int64_t(1) << 31)) << 8 | k;
        return valid ? w : ~uint64_t(0);
    }
    static EC_HD bool less(type a, type b) { return a < b; }
    static EC_HD uint32_t layer(type w) { return static_cast<uint32_t>(w) & 0xffu; }
    static EC_HD T value(type w) { return key_value<T>(static_cast<int64_t>(w >> 8) - (int64_t(1) << 31)); }
};
template <typename T>
struct rank_word<T, 8> {  // the key with its sign bit flipped orders as unsigned
    using type = RankPair;
    static EC_HD type make(T v, bool valid, uint32_t k) {
        const uint64_t key = static_cast<uint64_t>(order_key<T>(v)) ^ 0x8000000000000000ull;
        return type{valid ? key : ~uint64_t(0), valid ? k : 255u};
    }
    static EC_HD bool less(type a, type b) { return a.key < b.key || (a.key == b.key && a.k < b.k); }
    static EC_HD uint32_t layer(type w) { return w.k; }
    static EC_HD T value(type w) { return key_value<T>(static_cast<int64_t>(w.key ^ 0x8000000000000000ull)); }
};

template <typename T>
EC_HD typename rank_word<T>::type rank_select(bool c, typename rank_word<T>::type a, typename rank_word<T>::type b) {
    if constexpr (sizeof(T) == 8) return RankPair{c ? a.key : b.key, c ? a.k : b.k};
    else return c ? a : b;
}

// lo <- the lesser, hi <- the greater.  The words of a cell are distinct (k is), sentinels aside, and two sentinels are the same
// bits: which of them goes where is no question.
template <typename T>
EC_HD void rank_exchange(typename rank_word<T>::type& lo, typename rank_word<T>::type& hi) {
    const bool swap = rank_word<T>::less(hi, lo);
    const typename rank_word<T>::type a = rank_select<T>(swap, hi, lo), b = rank_select<T>(swap, lo, hi);
    lo = a;
    hi = b;
}

// Bitonic sort with every comparator ascending: the merge of size s first compares i with its mirror image in the block
// (i ^ (s - 1)), then halves.  N (N / 2) log2 N (log2 N + 1) / 4 exchanges: 1, 3, 24, 80, 240, 672 for N = 2 .. 64.
// The stages are template recursion and every loop has the constant trip count N, so that the unroller leaves no loop behind
// and every index into w is a constant (nested loops with shifted bounds were left rolled, and w went to memory).
template <typename T, int N, int J>
EC_HD void rank_halves(typename rank_word<T>::type (&w)[N]) {  // i against i ^ J, then J / 2 .. 1
    if constexpr (J > 0) {
        EC_UNROLL
        for (int i = 0; i < N; ++i)
            if ((i & J) == 0) rank_exchange<T>(w[i], w[i | J]);
        rank_halves<T, N, J / 2>(w);
    }
}
template <typename T, int N, int S>
EC_HD void rank_merges(typename rank_word<T>::type (&w)[N]) {  // the merges of size S, 2 S .. N
    if constexpr (S <= N) {
        EC_UNROLL
        for (int i = 0; i < N; ++i)
            if ((i ^ (S - 1)) > i) rank_exchange<T>(w[i], w[i ^ (S - 1)]);
        rank_halves<T, N, S / 4>(w);
        rank_merges<T, N, 2 * S>(w);
    }
}
template <typename T, int N>
EC_HD void rank_sort(typename rank_word<T>::type (&w)[N]) {
    static_assert(N >= 1 && (N & (N - 1)) == 0 && N <= kCompositeMaxLayers, "a power of two up to 64");
    rank_merges<T, N, 2>(w);
}

template <typename T, int N>
EC_HD typename rank_word<T>::type rank_pick(const typename rank_word<T>::type (&w)[N], uint32_t r) {
    typename rank_word<T>::type x = w[0];
    EC_UNROLL
    for (int j = 1; j < N; ++j) x = rank_select<T>(r == uint32_t(j), w[j], x);
    return x;
}

// r(count) for count <= N without a lane-indexed table: a select chain over the entries, which are launch-uniform.  On the device
// every entry is pinned to a scalar register first, and the table holds words: byte entries came in from the kernel's argument
// block by unaligned vector loads with the default cache policy (tools/isa_audit.py found them) and lived in vector registers.
#if defined(__HIP_DEVICE_COMPILE__)
#define EC_RANK_UNIFORM(x) static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(x)))
#else
#define EC_RANK_UNIFORM(x) static_cast<uint32_t>(x)
#endif
template <int N>
EC_HD uint32_t rank_of_count(const uint32_t (&r)[kCompositeMaxLayers + 1], uint32_t count) {
    uint32_t x = 0;
    EC_UNROLL
    for (int c = 1; c <= N; ++c) x = count == uint32_t(c) ? EC_RANK_UNIFORM(r[c]) : x;
    return x;
}

// the cell's value from the word picked; *mask its mask byte, *aux the layer or EC_COMPOSITE_NONE
template <typename T>
EC_HD T rank_finish(typename rank_word<T>::type picked, uint32_t count, uint32_t min_count, uint8_t* mask, uint8_t* aux) {
    const bool ok = count >= min_count;  // min_count >= 1: a cell without a valid layer, whose pick is a sentinel, is never ok
    *mask = ok ? 1 : 0;
    *aux = ok ? static_cast<uint8_t>(rank_word<T>::layer(picked)) : kCompositeNone;
    return ok ? rank_word<T>::value(picked) : T(0);
}

// one cell whose N words are made (layers past the stack's height as sentinels) and counted
template <typename T, int N>
EC_HD T rank_cell(typename rank_word<T>::type (&w)[N], uint32_t count, const uint32_t (&r)[kCompositeMaxLayers + 1], uint32_t min_count,
                  uint8_t* mask, uint8_t* aux) {
    rank_sort<T, N>(w);
    return rank_finish<T>(rank_pick<T, N>(w, rank_of_count<N>(r, count)), count, min_count, mask, aux);
}

}  // namespace ecd
