// ec_zonal_table_cell.hpp — the arithmetic of one cell and of one zone of ec_zonal_table_* (include/erased_cells.h, "Zonal
// statistics over a table in global memory"): the unit a zone's kind-1 sums are truncated to, the truncation of one deviation,
// the carry-free limbs the truncated values are added in, the flags of a zone's infinities, and the one rounding at finalize.
//
//   d = m * 2^-1074 with an integer m, exactly, for every finite f64.  L = bit length of the zone's largest |m|, k = max(L - 63, 0),
//   t = sign(m) * (|m| >> k): |t| < 2^63.  T = sum of t over at most 2^32 cells: |T| < 2^95.  s = T * 2^(k - 1074), rounded once.
//
//   limbs     t = lo + hi * 2^32 with lo = t mod 2^32 (0 .. 2^32 - 1) and hi = floor(t / 2^32) (-2^31 .. 2^31 - 1).  Over 2^32 cells the
//             lo's sum stays below 2^64 and the hi's within int64, so two 64-bit words under plain integer adds hold T: no carry
//             ever crosses a word, and an add needs nothing returned.  The kind-0 squares (q < 2^64, q = lo + hi * 2^32, both
//             halves unsigned) go the same way.
//   maximum   non-negative doubles order as their bits do, and NaN > inf > finite: ONE unsigned max of |d|'s bits carries both the
//             zone's largest magnitude and its class.  The largest w = fl(d * d) is fl(dmax * dmax) (rounding is monotonic).
//
// Self-contained like ec_regions_cell.hpp: no HIP runtime include; host/test_zonal_table_cell.cpp runs these very functions.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "ec_order_key.hpp"  // EC_HD

#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif

namespace ezt {

constexpr uint64_t kSignBit = 0x8000000000000000ull;
constexpr uint64_t kInfBits = 0x7FF0000000000000ull;
constexpr uint64_t kQuietNan = 0x7FF8000000000000ull;  // the NaN every record with a NaN deviation, or with both infinities, holds
constexpr uint64_t kFracMask = 0x000FFFFFFFFFFFFFull;
constexpr uint64_t kFlagPosInf = 1, kFlagNegInf = 2;

EC_HD uint64_t f64_bits(double v) { return __builtin_bit_cast(uint64_t, v); }
EC_HD double bits_f64(uint64_t b) { return __builtin_bit_cast(double, b); }
EC_HD int bit_length(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

// |d|'s bits: what the zone's maximum is taken of
EC_HD uint64_t abs_bits(double d) { return f64_bits(d) & ~kSignBit; }
// the flag of an infinite deviation, 0 for any other
EC_HD uint64_t inf_flag(double d) {
    const uint64_t b = f64_bits(d);
    return (b & ~kSignBit) != kInfBits ? 0 : (b & kSignBit) ? kFlagNegInf : kFlagPosInf;
}

// k of a zone whose largest |d| (finite) has the bits `max_bits`: |m| = frac (subnormal) or (2^52 + frac) << (exp - 1).
EC_HD int unit_shift(uint64_t max_bits) {
    const int exp = static_cast<int>(max_bits >> 52);
    const int len = exp == 0 ? bit_length(max_bits & kFracMask) : exp + 52;
    return len > 63 ? len - 63 : 0;
}

// t of one finite deviation d in a zone of unit 2^(k - 1074); |d| is at most the zone's maximum, so |t| < 2^63.
EC_HD int64_t trunc_units(double d, int k) {
    const uint64_t b = f64_bits(d);
    const int exp = static_cast<int>((b >> 52) & 0x7FF);
    const uint64_t mant = exp ? (b & kFracMask) | (uint64_t(1) << 52) : (b & kFracMask);
    const int up = (exp ? exp - 1 : 0) - k;  // |m| >> k = mant << up
    const uint64_t mag = up >= 0 ? mant << up : (up > -64 ? mant >> -up : 0);
    return (b & kSignBit) ? -static_cast<int64_t>(mag) : static_cast<int64_t>(mag);
}

// the bits of the zone's largest w = fl(dmax * dmax); kInfBits when it overflows
EC_HD uint64_t square_bits(uint64_t max_bits) {
    const double m = bits_f64(max_bits);
    return f64_bits(m * m);
}

// A signed sum in two carry-free words.
struct Limbs {
    uint64_t lo;  // sum of t mod 2^32
    int64_t hi;   // sum of floor(t / 2^32)
};
EC_HD void limbs_add(Limbs& a, int64_t t) {
    a.lo += static_cast<uint64_t>(t) & 0xFFFFFFFFull;
    a.hi += t >> 32;
}

// M * 2^e, M = mag_hi * 2^64 + mag_lo < 2^96, rounded to nearest even once; `e` >= -1074, so the product is a multiple of 2^-1074 and
// the only rounding is the cut to 53 bits.  +0.0 for M == 0; +-infinity on overflow, as IEEE rounds.
EC_HD double pow2(int x) { return bits_f64(static_cast<uint64_t>(x + 1023) << 52); }  // -1022 <= x <= 1023
EC_HD double fixed_to_f64(bool negative, uint64_t mag_hi, uint64_t mag_lo, int e) {
    if ((mag_hi | mag_lo) == 0) return 0.0;
    const int len = mag_hi ? 64 + bit_length(mag_hi) : bit_length(mag_lo);
    const int drop = len > 53 ? len - 53 : 0;  // 0 .. 43
    uint64_t q = mag_lo;
    if (drop > 0) {
        q = (mag_lo >> drop) | (mag_hi << (64 - drop));
        const uint64_t rest = mag_lo & ((uint64_t(1) << drop) - 1), half = uint64_t(1) << (drop - 1);
        if (rest > half || (rest == half && (q & 1))) ++q;  // q may become 2^53: still exact as a double
    }
    double r = static_cast<double>(q);  // exact
    const int x = e + drop;             // -1074 .. 1004
    if (x >= -1022) {
        r = r * pow2(x);  // exact, or overflows to infinity
    } else {
        r = r * pow2(-537);  // exact: q >= 1
        r = r * pow2(x + 537);  // exact: a multiple of 2^-1074 of fewer than 54 bits
    }
    return negative ? -r : r;
}

// T of two limbs as sign and magnitude, then fixed_to_f64.
EC_HD double limbs_to_f64(uint64_t lo, int64_t hi, int e) {
    // T = hi * 2^32 + lo in 128-bit two's complement
    uint64_t w0 = lo + (static_cast<uint64_t>(hi) << 32);
    uint64_t w1 = static_cast<uint64_t>(hi >> 32) + (w0 < lo ? 1u : 0u);
    const bool negative = (w1 & kSignBit) != 0;
    if (negative) {
        w0 = ~w0 + 1;
        w1 = ~w1 + (w0 == 0 ? 1u : 0u);
    }
    return fixed_to_f64(negative, w1, w0, e);
}

// What pass B needs of a zone: whether s1 / s2 are sums at all, and their units.
struct ZoneUnits {
    bool sum1, sum2;  // false: the record's value follows from the class and the flags alone, nothing is added
    int k1, k2;
};
EC_HD ZoneUnits zone_units(uint64_t max_bits) {
    ZoneUnits u{false, false, 0, 0};
    if (max_bits >= kInfBits) return u;
    u.sum1 = true;
    u.k1 = unit_shift(max_bits);
    const uint64_t w = square_bits(max_bits);
    if (w >= kInfBits) return u;
    u.sum2 = true;
    u.k2 = unit_shift(w);
    return u;
}

// s1 and s2 of a record from the zone's words.
EC_HD void zone_sums(uint64_t max_bits, uint64_t flags, uint64_t t1_lo, int64_t t1_hi, uint64_t t2_lo, int64_t t2_hi, double* s1, double* s2) {
    if (max_bits > kInfBits) {  // a NaN deviation
        *s1 = *s2 = bits_f64(kQuietNan);
        return;
    }
    if (max_bits == kInfBits) {
        const bool pos = (flags & kFlagPosInf) != 0, neg = (flags & kFlagNegInf) != 0;
        *s1 = bits_f64(pos && neg ? kQuietNan : pos ? kInfBits : (kInfBits | kSignBit));
        *s2 = bits_f64(kInfBits);
        return;
    }
    const ZoneUnits u = zone_units(max_bits);
    *s1 = limbs_to_f64(t1_lo, t1_hi, u.k1 - 1074);
    *s2 = u.sum2 ? limbs_to_f64(t2_lo, t2_hi, u.k2 - 1074) : bits_f64(kInfBits);
}

}  // namespace ezt
