// test_focal_rank_cell.cpp — one cell of ec_focal_rank / ec_focal_majority (csrc/ec_focal_rank_cell.hpp: majority_pick, and rank_pick
// over words whose k is the tap's position in the footprint), run from the header alone under a plain C++ compiler: the very functions
// the kernel runs.  Links nothing from the library.
//
// For every cell type — every word form: 1-, 2-, 4- and 8-byte cells, signed, unsigned and float — every bucket N = 1, 4, 8, 16, 32,
// 64 and every count in 0 .. N, footprints of N positions drawn from the type's special values (extremes, signed zeros, NaNs of both
// signs and several payloads, the u64 maximum and the all-ones NaN, whose keys are the sentinel's) with exactly `count` of them taps,
// at random positions: the majority must be what counting in a std::map ordered by the total order gives — the most frequent key,
// the least among equals, "equal" being equal bits — and the rank pick what std::sort gives at position r(count).  The order is
// written here as a three-way total order without order_key.  Palettes of two and three values make ties for the greatest frequency
// the rule, not the exception; with every tap the u64 maximum (or the all-ones NaN) the sentinels behind them hold the same key,
// and must not lengthen the run.  Footprints of up to 5 positions are covered exhaustively over a palette of three and every tap pattern.
// Built plain and, as test_focal_rank_cell_san, under the address and undefined-behaviour sanitizers.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <type_traits>
#include <vector>

#include "ec_focal_rank_cell.hpp"

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

template <typename T>
static T from_bits(uint64_t b) {
    T v;
    std::memcpy(&v, &b, sizeof v);
    return v;
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
struct TotalLess {
    bool operator()(T a, T b) const { return total_order(a, b) < 0; }
};

// the greatest cell of the total order first: its key is the sentinel's for 8-byte cells
template <typename T>
static std::vector<T> specials() {
    std::vector<T> s;
    using lim = std::numeric_limits<T>;
    if constexpr (std::is_floating_point<T>::value) {
        const uint64_t ones = sizeof(T) == 4 ? 0x7fffffffull : 0x7fffffffffffffffull;  // the all-ones positive NaN: the greatest key
        for (T v : {from_bits<T>(ones), T(0), T(-0.0), T(1), T(-1), T(0.1), lim::max(), lim::lowest(), lim::denorm_min(), lim::infinity(),
                    T(-lim::infinity()), lim::quiet_NaN(), T(-lim::quiet_NaN()), from_bits<T>(bits_of(lim::quiet_NaN()) | 1), from_bits<T>(~uint64_t(0))})
            s.push_back(v);
    } else {
        for (T v : {lim::max(), T(0), T(1), T(2), T(7), T(lim::max() - 1), T(lim::max() / 2), T(lim::max() / 2 + 1), lim::min(), T(lim::min() + 1)}) s.push_back(v);
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
static const Fraction kFractions[] = {{0, 1, kRankLower}, {1, 1, kRankUpper}, {1, 2, kRankLower}, {1, 2, kRankUpper},
                                      {1, 3, kRankUpper}, {9, 10, kRankLower}, {9, 10, kRankUpper}, {65534, 65535, kRankLower}};

// one footprint of N positions, tap[b] says which are taps; `full`: the tap count EC_FOCAL_WHOLE asks for
template <typename T, int N>
static void run_cell(const T* v, const bool* tap, const char* name) {
    using W = typename rank_word<T>::type;
    W w[N];
    uint32_t count = 0;
    std::vector<T> taps;
    for (int b = 0; b < N; ++b) {
        w[b] = rank_word<T>::make(v[b], tap[b], uint32_t(b));  // a cell that is no tap: whatever it holds leaves no trace
        count += tap[b];
        if (tap[b]) taps.push_back(v[b]);
    }
    rank_sort<T, N>(w);
    for (uint32_t j = 0; j < uint32_t(N); ++j)  // the taps stand first, the sentinels behind them
        CHECK((rank_word<T>::layer(w[j]) != 255u) == (j < count), "%s N=%d count=%u: position %u", name, N, count, j);

    // the majority by counting
    std::map<T, uint32_t, TotalLess<T>> freq;
    for (T x : taps) ++freq[x];
    uint32_t most = 0;
    T want = T(0);
    for (const auto& kv : freq)
        if (kv.second > most) most = kv.second, want = kv.first;  // ascending keys, strictly more: the least of the most frequent
    for (uint32_t need : {1u, uint32_t(N)}) {
        bool valid = !count;
        const T got = focal_rank_finish<T>(majority_pick<T, N>(w, count), count, need, &valid);
        const bool ok = count >= need;
        CHECK(valid == ok && bits_of(got) == (ok ? bits_of(want) : 0), "%s majority N=%d count=%u need=%u: got %016" PRIx64 " valid %d, want %016" PRIx64,
              name, N, count, need, bits_of(got), int(valid), bits_of(want));
    }

    // position r(count) of the sorted taps
    std::sort(taps.begin(), taps.end(), TotalLess<T>());
    for (const Fraction& f : kFractions) {
        const RankTable tab = rank_table(f.num, f.den, f.method);
        bool valid = !count;
        const T got = focal_rank_finish<T>(rank_pick<T, N>(w, rank_of_count<N>(tab.r, count)), count, 1, &valid);
        uint64_t expect = 0;
        if (count) {
            const uint64_t c = count, r = f.method == kRankUpper ? (uint64_t(f.num) * (c - 1) + f.den - 1) / f.den : (uint64_t(f.num) * (c - 1)) / f.den;
            expect = bits_of(taps[r]);
        }
        CHECK(valid == (count != 0) && bits_of(got) == expect, "%s rank N=%d count=%u q=%u/%u method=%d: got %016" PRIx64 ", want %016" PRIx64, name, N,
              count, f.num, f.den, f.method, bits_of(got), expect);
    }
}

template <typename T, int N>
static void test_bucket(const char* name) {
    const std::vector<T> sp = specials<T>();
    T v[N];
    bool tap[N];
    for (uint32_t count = 0; count <= uint32_t(N); ++count)
        for (int round = 0; round < 12; ++round) {
            // palettes: everything; three values; two values; the greatest cell only (rounds 3, 7, 11): every tap holds the sentinel's key
            const size_t pal = round % 4 == 0 ? sp.size() : round % 4 == 1 ? 3 : round % 4 == 2 ? 2 : 1;
            for (int b = 0; b < N; ++b) v[b] = sp[rnd() % pal], tap[b] = false;
            for (uint32_t placed = 0; placed < count;) {  // exactly `count` taps at random positions
                const int b = int(rnd() % N);
                if (!tap[b]) tap[b] = true, ++placed;
            }
            run_cell<T, N>(v, tap, name);
        }
}

// footprints of up to 5 positions (the 8-word network) exhaustively: a palette of three — the greatest cell among them — at every
// position and every tap pattern
template <typename T>
static void test_exhaustive(const char* name) {
    const std::vector<T> sp = specials<T>();
    const T pal[3] = {sp[0], sp[1], sp[2]};
    T v[8];
    bool tap[8];
    for (int k = 1; k <= 5; ++k) {
        int total = 1;
        for (int j = 0; j < k; ++j) total *= 3;
        for (int code = 0; code < total; ++code)
            for (int pat = 0; pat < (1 << k); ++pat) {
                int c = code;
                for (int j = 0; j < 8; ++j) v[j] = pal[0], tap[j] = false;  // positions past the footprint: never taps
                for (int j = 0; j < k; ++j, c /= 3) v[j] = pal[c % 3], tap[j] = (pat >> j) & 1;
                run_cell<T, 8>(v, tap, name);
            }
    }
}

template <typename T>
static void test_type(const char* name) {
    test_bucket<T, 1>(name);
    test_bucket<T, 4>(name);
    test_bucket<T, 8>(name);
    test_bucket<T, 16>(name);
    test_bucket<T, 32>(name);
    test_bucket<T, 64>(name);
    test_exhaustive<T>(name);
    // the sentinel lies above every valid word at every tap position, and a word gives its cell back
    for (T x : specials<T>())
        for (uint32_t k : {0u, 8u, 63u}) {
            const auto s = rank_word<T>::make(x, false, k), w = rank_word<T>::make(x, true, k);
            CHECK(rank_word<T>::less(w, s) && !rank_word<T>::less(s, w), "%s sentinel", name);
            CHECK(bits_of(rank_word<T>::value(w)) == bits_of(x) && rank_word<T>::layer(w) == k, "%s round trip", name);
            CHECK(rank_same_key<T>(w, rank_word<T>::make(x, true, 63u - k)), "%s same key, another position", name);
        }
}

int main() {
    CHECK(focal_rank_bucket(1) == 1 && focal_rank_bucket(3) == 4 && focal_rank_bucket(5) == 8 && focal_rank_bucket(7) == 8 && focal_rank_bucket(9) == 16 &&
              focal_rank_bucket(15) == 16 && focal_rank_bucket(21) == 32 && focal_rank_bucket(25) == 32 && focal_rank_bucket(35) == 64 &&
              focal_rank_bucket(49) == 64 && focal_rank_bucket(63) == 64,
          "buckets");
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
