// ec_compare_cell.hpp — one cell of ec_compare / ec_compare_scalar: impl Ord for CellValue (src/value.rs:248-265,
// PartialEq :267-271) as a predicate.
//
// Both cells are converted to CellType::union of their types (`unify`, src/value.rs:103-107; the lattice is constexpr,
// ec_lattice.hpp) with static_cast — Rust `as` for every widening pair, as ConvertFn relies on — and compared there:
// an integer union natively, f32 / f64 through order_key (total_cmp).  The relation is the 3-bit truth table over
// Ordering (bit 0 Less, bit 1 Equal, bit 2 Greater: ec_cmp, erased_cells.h) and a launch-uniform VALUE, so there is one
// kernel per type pair, not one per relation.
//
// Self-contained like ec_order_key.hpp: no HIP runtime include, host/test_compare_cell.cpp runs it under a plain C++ compiler.
#pragma once

#include <stdint.h>

#include "ec_lattice.hpp"
#include "ec_order_key.hpp"

namespace ecd {

template <typename L, typename R>
struct union_cell {
    using type = typename ecl::cell_of<ecl::union_of(ecl::dtype_of<L>::value, ecl::dtype_of<R>::value)>::type;
};

constexpr bool valid_relation(int rel) { return rel >= 1 && rel <= 6; }

// Ordering of CellValue(l) against CellValue(r): -1 Less, 0 Equal, +1 Greater
template <typename L, typename R>
EC_HD int cell_order(L l, R r) {
    using U = typename union_cell<L, R>::type;
    const U a = static_cast<U>(l), b = static_cast<U>(r);
    if constexpr (is_fp<U>::value) {
        const int64_t ka = order_key<U>(a), kb = order_key<U>(b);
        return int(ka > kb) - int(ka < kb);
    } else {
        return int(a > b) - int(a < b);
    }
}

// (rel >> (1 + CellValue(l).cmp(CellValue(r)))) & 1
template <typename L, typename R>
EC_HD uint8_t cell_cmp(L l, R r, uint32_t rel) {
    return static_cast<uint8_t>((rel >> (1 + cell_order<L, R>(l, r))) & 1u);
}

}  // namespace ecd
