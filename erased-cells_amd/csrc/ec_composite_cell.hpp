// ec_composite_cell.hpp — one cell of ec_composite (include/erased_cells.h): the fold of a stack of layers, one layer at a
// time, and what the cell stores at the end.  The rule is the header's; this is its only statement in code:
//
//   composite_step    FIRST / LAST the pick, MIN / MAX the strict-improvement compare under the reference's total order
//                     (src/value.rs:248-265 through order_key, ec_order_key.hpp), SUM / MEAN `acc = acc + double(cell)`
//   composite_finish  valid iff count >= min_count (the validity rule of src/masked/masked_buffer.rs:143-148, 208-217 over K layers);
//                     the value, the mask byte and the aux byte of the cell
//
// Every step is a select, not a branch: a layer that is not valid changes nothing, whatever its cell holds.  MEAN is SUM with a
// launch-uniform flag at the finish.
//
// Self-contained like ec_compare_cell.hpp: no HIP runtime include, host/test_composite_cell.cpp runs it under a plain C++ compiler.
#pragma once

#include <stdint.h>

#include "ec_order_key.hpp"

namespace ecd {

// ec_composite_op (erased_cells.h) as the kernels' template argument; MEAN runs the SUM kernels
constexpr int kCompositeFirst = 0, kCompositeLast = 1, kCompositeMin = 2, kCompositeMax = 3, kCompositeSum = 4, kCompositeMean = 5;
constexpr int kCompositeMaxLayers = 64;
constexpr uint8_t kCompositeNone = 255;

constexpr bool valid_composite_op(int op) { return op >= kCompositeFirst && op <= kCompositeMean; }
constexpr bool composite_sums(int op) { return op == kCompositeSum || op == kCompositeMean; }

// what a cell carries through the layers
template <typename T, bool SUMS>
struct CompositeState {  // FIRST, LAST, MIN, MAX: the cell picked so far; the layer it came from and the count share a word (both are
    T val;               // at most 255), which is a register per cell less in the kernels
    uint32_t idx_count;  // idx << 8 | count
    EC_HD uint32_t count() const { return idx_count & 0xffu; }
    EC_HD uint32_t idx() const { return idx_count >> 8; }
};
template <typename T>
struct CompositeState<T, true> {  // SUM, MEAN
    double acc;
    uint32_t n;
    EC_HD uint32_t count() const { return n; }
};
template <typename T, int OP>
using composite_state = CompositeState<T, composite_sums(OP)>;
template <typename T, int OP>
struct composite_result { using type = T; };
template <typename T> struct composite_result<T, kCompositeSum> { using type = double; };
template <typename T> struct composite_result<T, kCompositeMean> { using type = double; };

template <typename T, int OP>
EC_HD composite_state<T, OP> composite_init() {
    if constexpr (composite_sums(OP)) return composite_state<T, OP>{0.0, 0u};
    else return composite_state<T, OP>{T(0), uint32_t(kCompositeNone) << 8};
}

// `v` is strictly better than the running extreme `cur`: only then does a layer replace it, so equal keys keep the least k
template <typename T, bool MAX>
EC_HD bool composite_better(T v, T cur) {
    if constexpr (is_fp<T>::value) {
        const int64_t a = order_key<T>(v), b = order_key<T>(cur);
        return MAX ? a > b : a < b;
    } else {
        return MAX ? v > cur : v < cur;
    }
}

// layer k, whose cell is `v`, VALID or not
template <typename T, int OP>
EC_HD void composite_step(composite_state<T, OP>& s, T v, bool valid, uint32_t k) {
    if constexpr (composite_sums(OP)) {
        const double a = s.acc + static_cast<double>(v);  // one rounded f64 addition; a 64-bit integer converts by rounding
        s.acc = valid ? a : s.acc;
        s.n += valid ? 1u : 0u;
    } else {
        bool take;
        if constexpr (OP == kCompositeFirst) take = valid && s.count() == 0;
        else if constexpr (OP == kCompositeLast) take = valid;
        else take = valid && (s.count() == 0 || composite_better<T, OP == kCompositeMax>(v, s.val));
        s.val = take ? v : s.val;
        s.idx_count = (take ? k << 8 | s.count() : s.idx_count) + (valid ? 1u : 0u);
    }
}

// the cell's value; *mask its mask byte, *aux its aux byte (the layer picked or EC_COMPOSITE_NONE; for SUM / MEAN the count)
template <typename T, int OP>
EC_HD typename composite_result<T, OP>::type composite_finish(const composite_state<T, OP>& s, uint32_t min_count, bool mean, uint8_t* mask,
                                                              uint8_t* aux) {
    const bool ok = s.count() >= min_count;
    *mask = ok ? 1 : 0;
    if constexpr (composite_sums(OP)) {
        *aux = static_cast<uint8_t>(s.count());
        return ok ? (mean ? s.acc / static_cast<double>(s.count()) : s.acc) : 0.0;
    } else {
        (void)mean;
        *aux = ok ? static_cast<uint8_t>(s.idx()) : kCompositeNone;
        return ok ? s.val : T(0);
    }
}

}  // namespace ecd
