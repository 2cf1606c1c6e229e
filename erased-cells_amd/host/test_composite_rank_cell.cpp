// test_composite_rank_cell.cpp — one cell of ec_composite_rank (csrc/ec_composite_rank_cell.hpp: rank_word / rank_sort / rank_pick /
// rank_finish and the table r(c)), run from the header alone under a plain C++ compiler: the very functions the kernels run.  Links
// nothing from the library.
//
// For every cell type and every stack height K = 1 .. 64, stacks drawn from the type's special values (extremes, signed zeros, NaNs
// of both signs, the u64 maximum) under random validity, through the network of K's bucket: the cell must be what std::sort of the
// valid (key, k) pairs gives at position r(count) — the order written here as a three-way total order without order_key — for
// several (num, den, method) and every min_count that changes the answer.  K up to 5 is covered exhaustively over the validity
// patterns and over a palette of three.  Also: the table against the formula, the network on every 0/1 input (the zero-one principle)
// up to 16 wires, and the sentinel above every valid word.
// Built plain and, as test_composite_rank_cell_san, under the address and undefined-behaviour sanitizers.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>

#include "ec_composite_rank_cell.hpp"

using namespace ecd;

static unsigned long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        ++g_checks;                                       \
        if (!(cond)) {                                    \
            if (++g_failed <= 20) {                       \
                std::fprintf(stderr, "FAILED %s: ", #cond); \
                std::fprintf(stderr, __VA_ARGS__);        \
                std::fprintf(stderr, "\n");               \
            }                                             \
        }                                                 \
    } while (0)

template <typename T>
static uint64_t bits_of(T v) {
    uint64_t b = 0;
    std::memcpy(&b, &v, sizeof v);
    return b;
}

// Ordering of the reference (src/value.rs:248-265) written out: ints natural; floats total_cmp as sign, then magnitude bits
template <typename T>
static int total_order(T a, T b) {
    if constexpr (std::is_floating_point<T>::value) {
        const uint64_t sign = uint64_t(1) << (8 * sizeof(T) - 1);
        const uint64_t ba = bits_of(a), bb = bits_of(b);
        const bool na = ba & sign, nb = bb & sign;
        if (na != nb) return na ? -1 : 1;
        const uint64_t ma = ba & (sign - 1), mb = bb & (sign - 1);
        if (ma == mb) return 0;
        return ((ma < mb) != na) ? -1 : 1;  // among negatives the larger magnitude is the lesser
    } else {
        return a < b ? -1 : a > b ? 1 : 0;
    }
}

template <typename T>
static T from_bits(uint64_t b) {
    T v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}

template <typename T>
static std::vector<T> specials() {
    std::vector<T> s;
    using lim = std::numeric_limits<T>;
    if constexpr (std::is_floating_point<T>::value) {
        const uint64_t ones = sizeof(T) == 4 ? 0x7fffffffull : 0x7fffffffffffffffull;  // the all-ones positive NaN: the greatest key
        for (T v : {T(0), T(-0.0), T(1), T(-1), T(3), T(0.1), lim::max(), lim::lowest(), lim::min(), lim::denorm_min(), lim::infinity(),
                    T(-lim::infinity()), lim::quiet_NaN(), T(-lim::quiet_NaN()), from_bits<T>(ones), from_bits<T>(~uint64_t(0))})
            s.push_back(v);
    } else {
        for (T v : {T(0), T(1), T(2), T(7), lim::max(), T(lim::max() - 1), T(lim::max() / 2), T(lim::max() / 2 + 1), lim::min(), T(lim::min() + 1)}) s.push_back(v);
        if constexpr (std::is_signed<T>::value) s.push_back(T(-1));
    }
    return s;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

struct Fraction {
    uint32_t num, den;
    int method;
};
static const Fraction kFractions[] = {{0, 1, kRankLower}, {1, 1, kRankUpper}, {1, 2, kRankLower}, {1, 2, kRankUpper}, {1, 3, kRankLower},
                                      {1, 3, kRankUpper}, {9, 10, kRankLower}, {9, 10, kRankUpper}, {65535, 65535, kRankLower}, {1, 65535, kRankUpper}};

// the header's rule, independently: the valid (cell, k) pairs sorted, position r, or nothing
template <typename T>
static void expect(const T* v, const bool* valid, int k_layers, const Fraction& f, uint32_t min_count, uint64_t* bits, uint8_t* mask, uint8_t* aux) {
    std::vector<std::pair<T, int>> s;
    for (int k = 0; k < k_layers; ++k)
        if (valid[k]) s.push_back({v[k], k});
    std::sort(s.begin(), s.end(), [](const std::pair<T, int>& a, const std::pair<T, int>& b) {
        const int o = total_order(a.first, b.first);
        return o < 0 || (o == 0 && a.second < b.second);
    });
    const uint64_t c = s.size();
    if (c < min_count || c == 0) {
        *bits = 0, *mask = 0, *aux = 255;
        return;
    }
    const uint64_t r = f.method == kRankUpper ? (uint64_t(f.num) * (c - 1) + f.den - 1) / f.den : (uint64_t(f.num) * (c - 1)) / f.den;
    *bits = bits_of(s[r].first), *mask = 1, *aux = uint8_t(s[r].second);
}

template <typename T, int N>
static void run_cell(const T* v, const bool* valid, int k_layers, const char* name) {
    using W = typename rank_word<T>::type;
    for (const Fraction& f : kFractions) {
        const RankTable tab = rank_table(f.num, f.den, f.method);
        for (uint32_t mc = 1; mc <= uint32_t(k_layers); mc += (k_layers > 6 ? uint32_t(k_layers) / 3 + 1 : 1)) {
            W w[N];
            uint32_t count = 0;
            for (int b = 0; b < N; ++b) {
                const bool ok = b < k_layers && valid[b];
                w[b] = rank_word<T>::make(b < k_layers ? v[b] : T(0), ok, uint32_t(b));
                count += ok;
            }
            uint8_t mask = 7, aux = 7, wm, wa;
            const T got = rank_cell<T, N>(w, count, tab.r, mc, &mask, &aux);
            uint64_t want;
            expect<T>(v, valid, k_layers, f, mc, &want, &wm, &wa);
            CHECK(bits_of(got) == want && mask == wm && aux == wa,
                  "%s K=%d q=%u/%u method=%d min_count=%u: got %016" PRIx64 " mask %d aux %d, want %016" PRIx64 " mask %d aux %d", name, k_layers,
                  f.num, f.den, f.method, mc, bits_of(got), mask, aux, want, wm, wa);
        }
    }
}

template <typename T>
static void run_bucket(const T* v, const bool* valid, int k, const char* name) {
    switch (rank_bucket(k)) {
        case 1: return run_cell<T, 1>(v, valid, k, name);
        case 2: return run_cell<T, 2>(v, valid, k, name);
        case 4: return run_cell<T, 4>(v, valid, k, name);
        case 8: return run_cell<T, 8>(v, valid, k, name);
        case 16: return run_cell<T, 16>(v, valid, k, name);
        case 32: return run_cell<T, 32>(v, valid, k, name);
        default: return run_cell<T, 64>(v, valid, k, name);
    }
}

template <typename T>
static void test_type(const char* name) {
    const std::vector<T> sp = specials<T>();
    T v[64];
    bool valid[64];
    // every K, stacks from the palette under random validity: all valid, mostly valid, sparse
    for (int k = 1; k <= 64; ++k)
        for (int round = 0; round < 8; ++round) {
            for (int j = 0; j < k; ++j) {
                v[j] = sp[rnd() % (round % 2 ? 3 : sp.size())];  // odd rounds: three values, ties everywhere
                valid[j] = round < 2 || (rnd() % 100) < (round < 6 ? 70u : 15u);
            }
            run_bucket<T>(v, valid, k, name);
        }
    // K <= 5 exhaustively: every validity pattern over every stack of a palette of three (floats: +0.0, -0.0 and the all-ones NaN)
    const T pal[3] = {sp[0], sp[1], sp[sp.size() - 2]};
    for (int k = 1; k <= 5; ++k) {
        int total = 1;
        for (int j = 0; j < k; ++j) total *= 3;
        for (int code = 0; code < total; ++code)
            for (int pat = 0; pat < (1 << k); ++pat) {
                int c = code;
                for (int j = 0; j < k; ++j, c /= 3) v[j] = pal[c % 3], valid[j] = (pat >> j) & 1;
                run_bucket<T>(v, valid, k, name);
            }
    }
    // the sentinel lies above every valid word, whatever the cell and the layer
    for (T x : sp)
        for (uint32_t k : {0u, 63u}) {
            const auto s = rank_word<T>::make(x, false, k), w = rank_word<T>::make(x, true, k);
            CHECK(rank_word<T>::less(w, s) && !rank_word<T>::less(s, w), "%s sentinel", name);
            CHECK(bits_of(rank_word<T>::value(w)) == bits_of(x) && rank_word<T>::layer(w) == k, "%s round trip", name);
        }
}

// the zero-one principle: a comparator network that sorts every 0/1 input sorts every input
template <int N>
static void test_network() {
    for (uint32_t pat = 0; pat < (1u << N); ++pat) {
        uint32_t w[N];
        for (int i = 0; i < N; ++i) w[i] = rank_word<uint8_t>::make(uint8_t((pat >> i) & 1), true, 0);
        rank_sort<uint8_t, N>(w);
        bool sorted = true;
        for (int i = 0; i + 1 < N; ++i) sorted = sorted && w[i] <= w[i + 1];
        CHECK(sorted, "network of %d wires, input %x", N, pat);
    }
}

static void test_table() {
    for (const Fraction& f : kFractions) {
        const RankTable t = rank_table(f.num, f.den, f.method);
        for (uint64_t c = 1; c <= 64; ++c) {
            const uint64_t r = f.method == kRankUpper ? (uint64_t(f.num) * (c - 1) + f.den - 1) / f.den : (uint64_t(f.num) * (c - 1)) / f.den;
            CHECK(t.r[c] == r && r < c, "r(%d) of %u/%u method %d", int(c), f.num, f.den, f.method);
        }
    }
    CHECK(rank_bucket(1) == 1 && rank_bucket(2) == 2 && rank_bucket(3) == 4 && rank_bucket(5) == 8 && rank_bucket(9) == 16 && rank_bucket(17) == 32 &&
              rank_bucket(33) == 64 && rank_bucket(64) == 64 && rank_bucket(32) == 32,
          "buckets");
    CHECK(valid_rank_fraction(0, 1) && valid_rank_fraction(65535, 65535) && !valid_rank_fraction(1, 0) && !valid_rank_fraction(2, 1) &&
              !valid_rank_fraction(1, 65536) && valid_rank_method(0) && valid_rank_method(1) && !valid_rank_method(2) && !valid_rank_method(-1),
          "refusal predicates");
}

int main() {
    test_table();
    test_network<2>();
    test_network<4>();
    test_network<8>();
    test_network<16>();
    test_type<uint8_t>("u8");
    test_type<uint16_t>("u16");
    test_type<uint32_t>("u32");
    test_type<uint64_t>("u64");
    test_type<int8_t>("i8");
    test_type<int16_t>("i16");
    test_type<int32_t>("i32");
    test_type<int64_t>("i64");
    test_type<float>("f32");
    test_type<double>("f64");
    if (g_failed) {
        std::fprintf(stderr, "%lu of %lu checks FAILED\n", g_failed, g_checks);
        return 1;
    }
    std::printf("%lu checks passed\n", g_checks);
    return 0;
}
