// ec_order_key.hpp — the reference's per-cell order as integer keys (src/value.rs:248-265): ints natural, floats
// f32/f64::total_cmp (value.rs:260-261).  Every cell type maps to an int64 whose natural order is the reference order.
//
// Self-contained: no HIP runtime include; under a plain C++ compiler the two function attributes are defined away, so a
// stand-alone host program runs the very functions the kernels run (host/test_compare_cell.cpp).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define EC_HD inline
#endif

namespace ecd {

template <typename T> struct is_fp { static constexpr bool value = false; };
template <> struct is_fp<float> { static constexpr bool value = true; };
template <> struct is_fp<double> { static constexpr bool value = true; };

template <typename T>
EC_HD int64_t order_key(T v) {
    if constexpr (sizeof(T) == 8 && !is_fp<T>::value && T(-1) > T(0)) {
        return static_cast<int64_t>(static_cast<uint64_t>(v) ^ 0x8000000000000000ull);  // u64
    } else if constexpr (!is_fp<T>::value) {
        return static_cast<int64_t>(v);
    } else if constexpr (sizeof(T) == 4) {
        int32_t b = __builtin_bit_cast(int32_t, v);
        b ^= static_cast<int32_t>(static_cast<uint32_t>(b >> 31) >> 1);
        return b;
    } else {
        int64_t b = __builtin_bit_cast(int64_t, v);
        b ^= static_cast<int64_t>(static_cast<uint64_t>(b >> 63) >> 1);
        return b;
    }
}

template <typename T>
EC_HD T key_value(int64_t k) {
    if constexpr (sizeof(T) == 8 && !is_fp<T>::value && T(-1) > T(0)) {
        return static_cast<T>(static_cast<uint64_t>(k) ^ 0x8000000000000000ull);
    } else if constexpr (!is_fp<T>::value) {
        return static_cast<T>(k);
    } else if constexpr (sizeof(T) == 4) {
        int32_t b = static_cast<int32_t>(k);
        b ^= static_cast<int32_t>(static_cast<uint32_t>(b >> 31) >> 1);
        return __builtin_bit_cast(float, b);
    } else {
        int64_t b = k;
        b ^= static_cast<int64_t>(static_cast<uint64_t>(b >> 63) >> 1);
        return __builtin_bit_cast(double, b);
    }
}

}  // namespace ecd
