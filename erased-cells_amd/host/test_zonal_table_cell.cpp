// test_zonal_table_cell.cpp — csrc/ec_zonal_table_cell.hpp alone, on the host: the functions the kernels of ec_zonal_table_* run for one
// cell and one zone (include/erased_cells.h states the rule), against 128-bit integer arithmetic.
//   1. unit_shift / trunc_units against __int128 over every exponent gap 0 .. 70 between a zone's largest deviation and the cell,
//      subnormals included; the same values scaled by powers of two (where m no longer fits 128 bits) give the same t.
//   2. fixed_to_f64 / limbs_to_f64 against exact rounding (the compiler's own 128-bit conversion, then an exact scaling) at every
//      bit length 1 .. 96, with ties to even and to odd, one below and one above the tie, both signs, units from 2^-1074 to overflow.
//   3. zone_sums' classes: NaN, the infinities of one sign and of both, an overflowing square, the empty zone.
//   4. 16 threads adding one zone's cells into std::atomic words in shuffled orders and cuts: identical words every time, equal to
//      the serial 128-bit sums (build with -fsanitize=thread for the _tsan form).
// Stand-alone: its own main, links nothing from the library.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "ec_zonal_table_cell.hpp"

using namespace ezt;
typedef unsigned __int128 u128;
typedef __int128 i128;

static long checks = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        ++checks;                                               \
        if (!(cond)) {                                          \
            std::fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);                  \
            std::fprintf(stderr, "\n");                         \
            std::exit(1);                                       \
        }                                                       \
    } while (0)

static double make(int biased_exp, uint64_t frac, bool neg) {
    return bits_f64((neg ? kSignBit : 0) | (uint64_t(biased_exp) << 52) | (frac & kFracMask));
}
// m of a double whose biased exponent is at most 75: it fits 128 bits
static u128 units_of(double d) {
    const uint64_t b = f64_bits(d);
    const int exp = int((b >> 52) & 0x7FF);
    const uint64_t mant = exp ? (b & kFracMask) | (uint64_t(1) << 52) : (b & kFracMask);
    return u128(mant) << (exp ? exp - 1 : 0);
}
static int length_of(u128 v) {
    int n = 0;
    while (v) { ++n; v >>= 1; }
    return n;
}

static void test_truncation() {
    std::mt19937_64 rng(0x7AB1E);
    const uint64_t fracs[] = {0, 1, kFracMask, 0x8000000000000ull, 0x5555555555555ull};
    for (int top = 1; top <= 75; ++top) {
        for (int gap = 0; gap <= 70 && gap <= top; ++gap) {
            for (int rep = 0; rep < 8; ++rep) {
                const uint64_t fmax = rep < 5 ? fracs[rep] : rng(), fd = rep < 5 ? fracs[4 - rep] : rng();
                const double dmax = make(top, fmax, false);
                double d = make(top - gap, fd, (rep & 1) != 0);  // top - gap == 0: a subnormal
                if (abs_bits(d) > abs_bits(dmax)) d = (rep & 1) ? -dmax : dmax;
                const int len = length_of(units_of(dmax));
                const int k = len > 63 ? len - 63 : 0;
                CHECK(unit_shift(abs_bits(dmax)) == k, "unit_shift top %d", top);
                const u128 mag = units_of(std::fabs(d)) >> k;
                CHECK(mag < (u128(1) << 63), "the reference's own bound");
                const int64_t want = (f64_bits(d) & kSignBit) ? -int64_t(uint64_t(mag)) : int64_t(uint64_t(mag));
                CHECK(trunc_units(d, k) == want, "trunc_units top %d gap %d rep %d", top, gap, rep);
                // the same pair 2^s times larger: k grows by s (once it is positive), t stays
                for (int s : {1, 52, 500, 1900}) {
                    if (top + s > 2046 || top - gap == 0) continue;
                    const double dmax_s = make(top + s, fmax, false), d_s = bits_f64(f64_bits(d) + (uint64_t(s) << 52));
                    const int ks = unit_shift(abs_bits(dmax_s));
                    if (k > 0) {
                        CHECK(ks == k + s, "scaled unit_shift");
                        CHECK(trunc_units(d_s, ks) == want, "scaled trunc_units top %d gap %d s %d", top, gap, s);
                    }
                }
            }
        }
    }
    // subnormal-only zones: k = 0, t = m
    for (uint64_t f : {uint64_t(1), uint64_t(2), kFracMask, uint64_t(0x123456789ABCD)}) {
        CHECK(unit_shift(f) == 0, "subnormal unit");
        CHECK(trunc_units(bits_f64(f), 0) == int64_t(f) && trunc_units(bits_f64(f | kSignBit), 0) == -int64_t(f), "subnormal t");
    }
    CHECK(unit_shift(0) == 0 && trunc_units(0.0, 0) == 0 && trunc_units(-0.0, 0) == 0, "zeros");
    // the largest finite double: L = 2046 + 52, and its own t has 63 bits
    const uint64_t big = kInfBits - 1;
    CHECK(unit_shift(big) == 2098 - 63, "largest k");
    CHECK(trunc_units(bits_f64(big), unit_shift(big)) == int64_t((uint64_t(1) << 63) - (uint64_t(1) << 10)), "largest t");
}

static double exact(bool neg, u128 mag, int e) {
    const double r = std::ldexp(static_cast<double>(mag), e);  // the conversion rounds to nearest even; the scaling is exact or overflows
    return neg ? -r : r;
}

static void check_conversion(u128 mag, int e, int len) {
    for (int neg = 0; neg < 2; ++neg) {
        const double want = exact(neg != 0, mag, e), got = fixed_to_f64(neg != 0, uint64_t(mag >> 64), uint64_t(mag), e);
        CHECK(f64_bits(want) == f64_bits(got), "fixed_to_f64 length %d e %d: %a, not %a", len, e, got, want);
        // through the limbs: T = +-mag as lo + hi * 2^32
        const i128 T = neg ? -i128(mag) : i128(mag);
        const uint64_t lo = uint64_t(T) & 0xFFFFFFFFull;
        const int64_t hi = int64_t((T - i128(lo)) >> 32);
        const double via = limbs_to_f64(lo, hi, e);
        CHECK(f64_bits(via) == f64_bits(want), "limbs_to_f64 length %d e %d", len, e);
    }
}

static void test_conversion() {
    std::mt19937_64 rng(0xF1A7);
    const int units[] = {-1074, -1073, -1060, -1022, -1000, -537, -1, 0, 1, 500, 900, 928, 950, 961};
    for (int len = 1; len <= 95; ++len) {  // |T| < 2^95; 96 below through fixed_to_f64's own bound
        const u128 top = u128(1) << (len - 1);
        std::vector<u128> mags = {top, top | (top - 1)};
        if (len > 53) {
            const int drop = len - 53;
            const u128 half = u128(1) << (drop - 1), keep_even = top, keep_odd = top | (u128(1) << drop);
            for (u128 kept : {keep_even, keep_odd, top | (top - 1)})
                for (u128 low : {half, half - 1, half + 1, u128(0), (u128(1) << drop) - 1}) mags.push_back(((kept >> drop) << drop) | low);
        }
        for (int r = 0; r < 16; ++r) mags.push_back(top | ((u128(rng()) << 64 | rng()) & (top - 1)));
        for (u128 mag : mags)
            for (int e : units) check_conversion(mag, e, len);
    }
    for (u128 mag : {u128(1) << 95, (u128(1) << 96) - 1, (u128(1) << 95) | (u128(1) << 42), (u128(1) << 95) | (u128(1) << 42) | 1})
        for (int e : units)
            for (int neg = 0; neg < 2; ++neg)
                CHECK(f64_bits(exact(neg != 0, mag, e)) == f64_bits(fixed_to_f64(neg != 0, uint64_t(mag >> 64), uint64_t(mag), e)), "length 96");
    CHECK(f64_bits(fixed_to_f64(false, 0, 0, 0)) == 0 && f64_bits(fixed_to_f64(true, 0, 0, -1074)) == 0, "T == 0 gives +0.0");
    CHECK(std::isinf(fixed_to_f64(false, 0, uint64_t(1) << 62, 962)) && fixed_to_f64(true, 0, uint64_t(1) << 62, 962) < 0, "overflow");
}

static void test_classes() {
    double s1, s2;
    zone_sums(0, 0, 0, 0, 0, 0, &s1, &s2);
    CHECK(f64_bits(s1) == 0 && f64_bits(s2) == 0, "empty zone");
    zone_sums(kInfBits + 1, kFlagPosInf, 5, 0, 5, 0, &s1, &s2);
    CHECK(f64_bits(s1) == kQuietNan && f64_bits(s2) == kQuietNan, "NaN");
    zone_sums(kInfBits, kFlagPosInf, 5, 0, 5, 0, &s1, &s2);
    CHECK(f64_bits(s1) == kInfBits && f64_bits(s2) == kInfBits, "+inf");
    zone_sums(kInfBits, kFlagNegInf, 5, 0, 5, 0, &s1, &s2);
    CHECK(f64_bits(s1) == (kInfBits | kSignBit) && f64_bits(s2) == kInfBits, "-inf");
    zone_sums(kInfBits, kFlagPosInf | kFlagNegInf, 5, 0, 5, 0, &s1, &s2);
    CHECK(f64_bits(s1) == kQuietNan && f64_bits(s2) == kInfBits, "both infinities");
    // an overflowing square: d = 2^600, one cell
    const double d = std::ldexp(1.0, 600);
    const ZoneUnits u = zone_units(abs_bits(d));
    CHECK(u.sum1 && !u.sum2, "2^600 squared overflows");
    Limbs t{0, 0};
    limbs_add(t, trunc_units(d, u.k1));
    zone_sums(abs_bits(d), 0, t.lo, t.hi, 0, 0, &s1, &s2);
    CHECK(s1 == d && f64_bits(s2) == kInfBits, "s1 stays a sum, s2 = +inf");
    CHECK(inf_flag(INFINITY) == kFlagPosInf && inf_flag(-INFINITY) == kFlagNegInf && inf_flag(1.0) == 0 && inf_flag(NAN) == 0, "flags");
    CHECK(abs_bits(NAN) > kInfBits && abs_bits(-INFINITY) == kInfBits && abs_bits(-1.0) < kInfBits, "NaN > inf > finite as integers");
}

// One zone's cells under 16 threads: every thread folds runs of its share into a local entry and adds it to the shared words.
struct Words {
    std::atomic<uint64_t> count{0}, t1_lo{0}, t1_hi{0}, t2_lo{0}, t2_hi{0}, flags{0};
};

static void test_threads() {
    std::mt19937_64 rng(0x7EA45);
    const int n = 1 << 14, threads = 16;
    std::vector<double> d(n);
    for (int i = 0; i < n; ++i) {
        const int e = int(rng() % 90) - 30;  // deviations that span more than 63 bits
        d[i] = std::ldexp(double(int64_t(rng() >> 11)) / 9007199254740992.0 - 0.5, e);
    }
    d[7] = std::ldexp(1.0, 70);
    uint64_t maxb = 0;
    for (double x : d) maxb = abs_bits(x) > maxb ? abs_bits(x) : maxb;
    const ZoneUnits u = zone_units(maxb);
    CHECK(u.sum1 && u.sum2 && u.k1 > 0, "the zone truncates");
    i128 T1 = 0, T2 = 0;
    for (double x : d) {
        T1 += trunc_units(x, u.k1);
        T2 += trunc_units(x * x, u.k2);
    }
    uint64_t first[5] = {0, 0, 0, 0, 0};
    for (int round = 0; round < 6; ++round) {
        std::vector<int> order(n);
        for (int i = 0; i < n; ++i) order[i] = i;
        std::shuffle(order.begin(), order.end(), rng);
        Words w;
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t)
            pool.emplace_back([&, t] {
                std::mt19937 cut(unsigned(round * 97 + t));
                Limbs a{0, 0}, b{0, 0};
                uint64_t cnt = 0;
                auto flush = [&] {
                    w.count.fetch_add(cnt, std::memory_order_relaxed);
                    w.t1_lo.fetch_add(a.lo, std::memory_order_relaxed);
                    w.t1_hi.fetch_add(uint64_t(a.hi), std::memory_order_relaxed);
                    w.t2_lo.fetch_add(b.lo, std::memory_order_relaxed);
                    w.t2_hi.fetch_add(uint64_t(b.hi), std::memory_order_relaxed);
                    a = b = Limbs{0, 0};
                    cnt = 0;
                };
                for (int i = t; i < n; i += threads) {
                    const double x = d[size_t(order[size_t(i)])];
                    limbs_add(a, trunc_units(x, u.k1));
                    limbs_add(b, trunc_units(x * x, u.k2));
                    ++cnt;
                    if (cut() % 5 == 0) flush();  // a run ends
                }
                flush();
            });
        for (auto& th : pool) th.join();
        const uint64_t got[5] = {w.count.load(), w.t1_lo.load(), w.t1_hi.load(), w.t2_lo.load(), w.t2_hi.load()};
        if (round == 0)
            for (int k = 0; k < 5; ++k) first[k] = got[k];
        for (int k = 0; k < 5; ++k) CHECK(got[k] == first[k], "round %d word %d differs", round, k);
        CHECK(got[0] == uint64_t(n), "count");
        CHECK(i128(int64_t(got[2])) * (i128(1) << 32) + i128(got[1]) == T1, "T1 is the serial sum");
        CHECK(i128(int64_t(got[4])) * (i128(1) << 32) + i128(got[3]) == T2, "T2 is the serial sum");
    }
    double s1, s2;
    zone_sums(maxb, 0, first[1], int64_t(first[2]), first[3], int64_t(first[4]), &s1, &s2);
    CHECK(f64_bits(s1) == f64_bits(exact(T1 < 0, u128(T1 < 0 ? -T1 : T1), u.k1 - 1074)), "s1 of the threads' words");
    CHECK(f64_bits(s2) == f64_bits(exact(false, u128(T2), u.k2 - 1074)), "s2 of the threads' words");
}

int main() {
    test_truncation();
    test_conversion();
    test_classes();
    test_threads();
    std::printf("test_zonal_table_cell: %ld checks passed\n", checks);
    return 0;
}
