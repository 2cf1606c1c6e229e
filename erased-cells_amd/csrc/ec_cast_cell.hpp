// ec_cast_cell.hpp — one cell of ec_cast / ec_cast_scaled (include/erased_cells.h): a cell of type S as a cell of type D, for
// all 100 ordered pairs, where CellValue::convert (src/value.rs:74-98) refuses 59 of them.
//
//   cast_as<S, D>     Rust's `as`: integers keep their low bits, a float becomes an integer by truncation toward zero,
//                     saturated, NaN -> 0; into f32 by round to nearest even, overflow to +-inf, a NaN stays a NaN of its sign.
//   cast_round<S, D>  the storing rule (GDALAdjustValueToDataType's shape, the TODO of src/value.rs:75): integers are clamped
//                     to D's range in exact integer arithmetic, a float is rounded half away from zero by ONE f64 add and a
//                     truncation (round_cell), then saturated; the 64-bit limits are compared in f64; NaN -> 0.  Into f32 as `as`.
//   scaled<S, D>      the storing direction of a scale and offset: cast_round of to_f64(x) * scale + offset, the product and
//                     the sum rounded individually — never an fma: every includer is built with
//                     -ffp-contract=off (csrc/Makefile, host/Makefile), see `scaled`.
// For the 41 pairs with can_fit_into(S, D) all three are the value-preserving conversion ConvertFn makes.
//
// No float-to-integer static_cast is reached with a value outside the destination's range (undefined behaviour in C++): every
// such cast is behind a clamp.  Self-contained like ec_compare_cell.hpp: no HIP runtime include, host/test_cast_cell.cpp runs
// it under a plain C++ compiler, plain and under the address and undefined-behaviour sanitizers.
#pragma once

#include <stdint.h>

#include "ec_order_key.hpp"

namespace ecd {

template <typename T>
struct cell_limits {  // the range of an integer cell type
    static constexpr bool is_signed = T(-1) < T(0);
    static constexpr T hi = is_signed ? T((uint64_t(1) << (8 * sizeof(T) - 1)) - 1) : T(~uint64_t(0));
    static constexpr T lo = is_signed ? T(-hi - 1) : T(0);
};

// v, already integral or about to be truncated toward zero, as a cell of the integer type T, saturated; NaN -> 0.  The 64-bit
// limits are compared in f64 (2^63 and 2^64 are f64 values, the largest i64 / u64 are not); the narrower ranges are exact in
// f64 and clamped there, so that the cast that follows is always in range.
template <typename T>
EC_HD T saturate_cell(double v) {
    static_assert(!is_fp<T>::value, "an integer destination");
    constexpr bool SIGNED = cell_limits<T>::is_signed;
    if constexpr (sizeof(T) == 8 && !SIGNED) {
        return v >= 18446744073709551616.0 ? ~uint64_t(0) : !(v > 0.0) ? uint64_t(0) : static_cast<uint64_t>(v);
    } else if constexpr (sizeof(T) == 8) {
        return v >= 9223372036854775808.0 ? INT64_MAX : v <= -9223372036854775808.0 ? INT64_MIN : v != v ? int64_t(0) : static_cast<int64_t>(v);
    } else {
        constexpr double lo = static_cast<double>(cell_limits<T>::lo), hi = static_cast<double>(cell_limits<T>::hi);
        return v != v ? T(0) : static_cast<T>(static_cast<int64_t>(v < lo ? lo : v > hi ? hi : v));
    }
}

// r as a cell of type T: f64 as it is, f32 rounded to nearest even, integers rounded half away from zero by ONE f64 add and a
// truncation, then saturated as Rust's `as` saturates.  (The one add rounds 0.49999999999999994 + 0.5 up to 1.0: that cell is 1.)
template <typename T>
EC_HD T round_cell(double r) {
    if constexpr (sizeof(T) == 8 && is_fp<T>::value) return r;
    else if constexpr (is_fp<T>::value) return static_cast<float>(r);
    else return saturate_cell<T>(__builtin_trunc(r + __builtin_copysign(0.5, r)));
}

template <typename S, typename D>
EC_HD D cast_as(S v) {
    if constexpr (is_fp<S>::value && !is_fp<D>::value) return saturate_cell<D>(static_cast<double>(v));  // clamped, then truncated by the cast
    else return static_cast<D>(v);  // integers: the low bits / sign extension; into a float: round to nearest even
}

template <typename S, typename D>
EC_HD D cast_round(S v) {
    if constexpr (is_fp<D>::value) {
        return static_cast<D>(v);
    } else if constexpr (is_fp<S>::value) {
        return round_cell<D>(static_cast<double>(v));
    } else {  // integer to integer: clamped, exact in integers (no detour through f64)
        using LS = cell_limits<S>;
        using LD = cell_limits<D>;
        if constexpr (LS::is_signed) {
            if (v < S(0)) {
                if constexpr (!LD::is_signed) return D(0);
                else if constexpr (sizeof(D) < sizeof(S)) return v < static_cast<S>(LD::lo) ? LD::lo : static_cast<D>(v);
                else return static_cast<D>(v);
            }
        }
        const uint64_t u = static_cast<uint64_t>(v);  // v >= 0
        return u > static_cast<uint64_t>(LD::hi) ? LD::hi : static_cast<D>(u);
    }
}

template <typename S, typename D>
EC_HD D scaled(S v, double scale, double offset) {
    // Compile with -ffp-contract=off, as the library and host/Makefile do (the device the resampling kernels rely on).  No pragma
    // here: under -ffp-contract=fast — hipcc's default — this compiler fuses the two statements whatever FP_CONTRACT pragma stands
    // in the block, so a pragma would promise what it does not keep; tests hold 0.1 * 10.0 + -1.0 to 0.0 on the host and the GPU.
    const double p = static_cast<double>(v) * scale;  // rounded
    const double y = p + offset;                      // rounded again: two operations, never an fma
    if constexpr (sizeof(D) == 8 && is_fp<D>::value) return y;
    else return cast_round<double, D>(y);
}

}  // namespace ecd
