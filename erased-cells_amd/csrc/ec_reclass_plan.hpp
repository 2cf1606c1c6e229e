// ec_reclass_plan.hpp — the host side of the reclassification (include/erased_cells.h: ec_reclass_table_build, ec_reclass) in
// plain C++: the thresholds and the record's layout, and what the launch and the kernels share.  The refusals and the builder:
// ec_reclass_checks.hpp.
//
// The thresholds.  For every pair of the lattice the cast t -> UT = union(t, bt) is monotone non-decreasing in t's own order,
// and a break is never a NaN, so NaN payloads decide nothing: "UT(x) >= b" (right: "UT(x) > b") over the cells of type t is
// "order_key<T>(x) >= thr" for the smallest key whose cell satisfies the predicate.  It is found by bisection over T's key
// range — at most 64 steps, the midpoint taken in unsigned arithmetic — with the predicate decided by cell_order
// (ec_compare_cell.hpp), the very function ec_compare_scalar's kernels run.  A break whose predicate fails at T's greatest key
// is reached by no cell and has no threshold; breaks ascend, so such breaks are a suffix and n_reached counts the others.
//
// Self-contained: no HIP include and nothing from this library but ec_lattice.hpp, ec_order_key.hpp and ec_compare_cell.hpp,
// so that host/test_reclass_plan.cpp runs these very functions under the address and undefined-behaviour sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "ec_compare_cell.hpp"
#include "ec_lattice.hpp"
#include "ec_order_key.hpp"

namespace ecr {

constexpr int32_t kMaxBreaks = 255;    // EC_RECLASS_MAX_BREAKS
constexpr int32_t kSlots = 256;        // class values and validity bytes of a record
constexpr int kBlock = 256;            // threads of a workgroup of the reclass kernels: one per slot of the record
constexpr int kU = 2;                  // groups per lane of a tile: the default "map_u"
constexpr uint64_t kMaxTiles = 0x7fffffffull;

static_assert(sizeof(ec_reclass_table) == EC_RECLASS_TABLE_BYTES && EC_RECLASS_TABLE_BYTES % 16 == 0, "the record's size is part of the ABI");
static_assert(offsetof(ec_reclass_table, thr) == 40 && offsetof(ec_reclass_table, value_bits) == 2080 && offsetof(ec_reclass_table, valid) == 4128,
              "the record has no padding the builder does not write");

// the least and greatest order key of a cell of type T (every key between them is a cell's: order_key is a bijection)
template <typename T>
constexpr int64_t key_min() {
    if constexpr (sizeof(T) == 8) return INT64_MIN;                       // u64 (biased), i64, f64
    else if constexpr (ecd::is_fp<T>::value) return INT32_MIN;            // f32: every bit pattern
    else if constexpr (T(-1) > T(0)) return 0;                            // u8, u16, u32
    else return -(int64_t(1) << (8 * sizeof(T) - 1));                     // i8, i16, i32
}
template <typename T>
constexpr int64_t key_max() {
    if constexpr (sizeof(T) == 8) return INT64_MAX;
    else if constexpr (ecd::is_fp<T>::value) return INT32_MAX;
    else if constexpr (T(-1) > T(0)) return (int64_t(1) << (8 * sizeof(T))) - 1;
    else return (int64_t(1) << (8 * sizeof(T) - 1)) - 1;
}

// CellValue(x) >= CellValue(b) (right: >) in the union type
template <typename T, typename BT>
inline bool at_or_past(int64_t key, BT b, bool right) {
    return ecd::cell_order<T, BT>(ecd::key_value<T>(key), b) >= (right ? 1 : 0);
}

// The smallest key of T whose cell is at or past the break; false when no cell of type T is.
template <typename T, typename BT>
inline bool threshold(BT b, bool right, int64_t* thr) {
    int64_t lo = key_min<T>(), hi = key_max<T>();
    if (!at_or_past<T, BT>(hi, b, right)) return false;
    while (lo < hi) {  // at_or_past(hi) holds, at_or_past(lo - 1) does not
        const int64_t mid = static_cast<int64_t>(static_cast<uint64_t>(lo) + (static_cast<uint64_t>(hi) - static_cast<uint64_t>(lo)) / 2);
        if (at_or_past<T, BT>(mid, b, right)) hi = mid;
        else lo = mid + 1;
    }
    *thr = lo;
    return true;
}

// Why breaks of type BT are refused for a raster of type T, or null: a NaN, or not strictly ascending in the union type.
template <typename T, typename BT>
inline const char* breaks_refusal(const BT* b, int32_t n_breaks) {
    using U = typename ecd::union_cell<T, BT>::type;
    if constexpr (ecd::is_fp<BT>::value)
        for (int32_t j = 0; j < n_breaks; ++j)
            if (b[j] != b[j]) return "a break is NaN";
    for (int32_t j = 1; j < n_breaks; ++j)
        if (ecd::cell_order<U, U>(static_cast<U>(b[j - 1]), static_cast<U>(b[j])) >= 0)
            return "the breaks are not strictly ascending in the union of the raster's and the breaks' types";
    return nullptr;
}

template <typename T, typename BT>
inline int32_t thresholds(const BT* b, int32_t n_breaks, bool right, int64_t* thr) {
    int32_t n_reached = 0;
    while (n_reached < n_breaks && threshold<T, BT>(b[n_reached], right, thr + n_reached)) ++n_reached;
    return n_reached;
}

// f(T{}, BT{}) for the pair of codes (both valid)
template <typename T, typename F>
inline auto with_break_type(int bt, F&& f) -> decltype(f(uint8_t{}, uint8_t{})) {
    switch (bt) {
#define EC_RECLASS_ROW(ID, BT) case ID: return f(T{}, BT{});
        EC_WITH_CT(EC_RECLASS_ROW)
#undef EC_RECLASS_ROW
    }
    return decltype(f(uint8_t{}, uint8_t{})){};
}
template <typename F>
inline auto with_pair(int t, int bt, F&& f) -> decltype(f(uint8_t{}, uint8_t{})) {
    switch (t) {
#define EC_RECLASS_ROW(ID, T) case ID: return with_break_type<T>(bt, f);
        EC_WITH_CT(EC_RECLASS_ROW)
#undef EC_RECLASS_ROW
    }
    return decltype(f(uint8_t{}, uint8_t{})){};
}

// a cell's bytes from the start of an ec_value's payload, in the low bytes of a word
inline uint64_t low_bytes(const ec_value& v, size_t size) {
    uint64_t bits = 0;
    memcpy(&bits, &v.v, size);  // little-endian host, as everywhere in this library
    return bits;
}

// c = #{ j < n_reached : thr[j] <= key }: the class through the record, as the kernels compute it (a plain loop here)
inline int32_t class_of(const ec_reclass_table& tab, int64_t key) {
    int32_t c = 0;
    for (int32_t j = 0; j < tab.n_reached; ++j) c += tab.thr[j] <= key;
    return c;
}

// The steps of the kernels' branch-free upper bound over n_reached thresholds: ceil(log2(n_reached + 1)), 0 .. 8.
constexpr int search_steps(int32_t n_reached) {
    int steps = 0;
    while ((int32_t(1) << steps) < n_reached + 1) ++steps;
    return steps;
}

// The tiles of a launch: groups of cpl cells, kBlock * kU groups per workgroup, one workgroup per tile.
constexpr size_t cpl(size_t cell_size, size_t out_size) { return 16 / (cell_size > out_size ? cell_size : out_size); }
constexpr uint64_t tiles(uint64_t n, size_t cpl_) { return (n / cpl_ + uint64_t(kBlock) * kU - 1) / (uint64_t(kBlock) * kU); }

}  // namespace ecr
