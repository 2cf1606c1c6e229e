// test_reclass_plan.cpp — csrc/ec_reclass_plan.hpp and csrc/ec_reclass_checks.hpp alone, under a plain C++17 compiler (and, as test_reclass_plan_san, under the
// address and undefined-behaviour sanitizers): the thresholds against the union-order predicate itself for EVERY cell of the 1-
// and 2-byte types and for planted cells of the wider ones, the key ranges, unreachable suffixes, the refusals in the order
// include/erased_cells.h states, that a refused build writes nothing and a build defines every byte, and the kernels'
// branch-free search (restated here in plain C++) against the plain count.  Needs no GPU and nothing from the library.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "ec_reclass_checks.hpp"

static int g_checks = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) {                                                                 \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

using namespace ecr;

// a refusal as these checks read it: its text (null: none), the type flag left in *bad
static const char* told(const ecv::Refusal& r, bool* bad) {
    *bad = r.bad_type;
    return r.why;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

// the kernels' search (ec_reclass_kernels.hpp reclass_search), one cell
static int32_t search(const int64_t* thr, int32_t nr, int64_t key) {
    int32_t c = 0;
    for (int step = (1 << search_steps(nr)) >> 1; step != 0; step >>= 1) {
        const int idx = c + step - 1;
        CHECK(idx >= 0 && idx < kMaxBreaks);
        c += (idx < nr && thr[idx] <= key) ? step : 0;
    }
    return c;
}

template <typename T>
static ec_value value_of(int dt, T x) {
    ec_value v;
    std::memset(&v, 0, sizeof v);
    v.dtype = static_cast<uint8_t>(dt);
    std::memcpy(&v.v, &x, sizeof x);
    return v;
}

// class of the cell with key `key` by the rule itself: the count of breaks at or below it in the union order
template <typename T, typename BT>
static int32_t rule(int64_t key, const std::vector<BT>& b, bool right) {
    int32_t c = 0;
    for (BT x : b) c += ecd::cell_order<T, BT>(ecd::key_value<T>(key), x) >= (right ? 1 : 0);
    return c;
}

template <typename BT>
static std::vector<BT> some_breaks(int n, int round) {
    std::vector<BT> b;
    if constexpr (ecd::is_fp<BT>::value) {
        // around the narrow types' ranges, fractions included; the last rounds reach past every 16-bit cell
        const double lo = round == 0 ? -1.5 : -70000.0, hi = round == 0 ? 300.0 : 70000.0;
        for (int j = 0; j < n; ++j) b.push_back(static_cast<BT>(lo + (hi - lo) * (j + 0.37) / n));
        if (round == 2) { b.front() = -std::numeric_limits<BT>::infinity(); b.back() = std::numeric_limits<BT>::infinity(); }
    } else {
        const double lo = double(std::numeric_limits<BT>::lowest()), hi = double(std::numeric_limits<BT>::max());
        const double span = round == 0 ? (hi - lo) : 600.0, base = round == 0 ? lo : (lo < 0 ? -300.0 : 0.0);
        for (int j = 0; j < n; ++j) {
            double x = base + span * (j + 0.5) / n;
            if (x < lo) x = lo;
            const BT v = x >= hi ? std::numeric_limits<BT>::max() : static_cast<BT>(x);  // double(max) is past the range of a 64-bit type
            if (b.empty() || v > b.back()) b.push_back(v);
        }
    }
    return b;
}

template <typename T, typename BT>
static void exhaustive() {
    constexpr int t = ecl::dtype_of<T>::value, bt = ecl::dtype_of<BT>::value;
    for (int round = 0; round < 3; ++round)
        for (int n : {1, 3, 8, sizeof(T) == 1 ? 255 : 40})
            for (int right = 0; right < 2; ++right) {
                const std::vector<BT> b = some_breaks<BT>(n, round);
                std::vector<ec_value> vals;
                for (size_t c = 0; c <= b.size(); ++c) vals.push_back(value_of<uint8_t>(EC_U8, uint8_t(c)));
                ec_reclass_table tab;
                bool bad = false;
                const char* why = told(build(t, bt, b.data(), int32_t(b.size()), right, EC_U8, vals.data(), nullptr, nullptr, &tab), &bad);
                CHECK(why == nullptr && !bad);
                CHECK(tab.n_reached >= 0 && tab.n_reached <= tab.n_breaks && tab.n_breaks == int32_t(b.size()));
                for (int32_t j = 1; j < tab.n_reached; ++j) CHECK(tab.thr[j - 1] <= tab.thr[j]);
                for (int32_t j = tab.n_reached; j < kMaxBreaks; ++j) CHECK(tab.thr[j] == 0);
                for (int64_t key = key_min<T>(); key <= key_max<T>(); ++key) {
                    const int32_t want = rule<T, BT>(key, b, right != 0);
                    CHECK(class_of(tab, key) == want);
                    CHECK(search(tab.thr, tab.n_reached, key) == want);
                }
            }
}

template <typename T>
static void exhaustive_all_breaks() {
    exhaustive<T, uint8_t>(); exhaustive<T, uint16_t>(); exhaustive<T, uint32_t>(); exhaustive<T, uint64_t>();
    exhaustive<T, int8_t>(); exhaustive<T, int16_t>(); exhaustive<T, int32_t>(); exhaustive<T, int64_t>();
    exhaustive<T, float>(); exhaustive<T, double>();
}

// wide types: cells planted at the breaks and beside them, at the ends of the key range, and random keys
template <typename T, typename BT>
static void planted(const std::vector<BT>& b) {
    constexpr int t = ecl::dtype_of<T>::value, bt = ecl::dtype_of<BT>::value;
    std::vector<ec_value> vals;
    for (size_t c = 0; c <= b.size(); ++c) vals.push_back(value_of<uint8_t>(EC_U8, uint8_t(c)));
    for (int right = 0; right < 2; ++right) {
        ec_reclass_table tab;
        bool bad = false;
        CHECK(told(build(t, bt, b.data(), int32_t(b.size()), right, EC_U8, vals.data(), nullptr, nullptr, &tab), &bad) == nullptr);
        std::vector<int64_t> keys = {key_min<T>(), key_min<T>() + 1, key_max<T>() - 1, key_max<T>(), 0, -1, 1};
        for (int32_t j = 0; j < tab.n_reached; ++j)
            for (int64_t d = -2; d <= 2; ++d) {
                const int64_t k = tab.thr[j];
                if ((d < 0 && k < key_min<T>() - d) || (d > 0 && k > key_max<T>() - d)) continue;
                keys.push_back(k + d);
            }
        for (int i = 0; i < 2000; ++i) {
            const uint64_t r = rnd();
            keys.push_back(sizeof(T) == 8 ? int64_t(r) : int64_t(int32_t(uint32_t(r))));
        }
        for (int64_t key : keys) {
            if (key < key_min<T>() || key > key_max<T>()) continue;
            const int32_t want = rule<T, BT>(key, b, right != 0);
            CHECK(class_of(tab, key) == want);
            CHECK(search(tab.thr, tab.n_reached, key) == want);
        }
    }
}

int main() {
    static_assert(key_min<uint8_t>() == 0 && key_max<uint8_t>() == 255 && key_min<int8_t>() == -128 && key_max<int16_t>() == 32767, "key ranges");
    static_assert(key_max<uint32_t>() == 4294967295ll && key_min<float>() == INT32_MIN && key_min<uint64_t>() == INT64_MIN, "key ranges");
    static_assert(search_steps(0) == 0 && search_steps(1) == 1 && search_steps(2) == 2 && search_steps(3) == 2 && search_steps(4) == 3 &&
                  search_steps(7) == 3 && search_steps(8) == 4 && search_steps(127) == 7 && search_steps(128) == 8 && search_steps(255) == 8, "steps");
    static_assert(cpl(1, 1) == 16 && cpl(2, 1) == 8 && cpl(4, 8) == 2 && tiles(0, 16) == 0 && tiles(16 * 512, 16) == 1 && tiles(16 * 512 + 16, 16) == 2, "tiles");

    exhaustive_all_breaks<uint8_t>();
    exhaustive_all_breaks<int8_t>();
    exhaustive_all_breaks<uint16_t>();
    exhaustive_all_breaks<int16_t>();

    const double inf = std::numeric_limits<double>::infinity();
    const float finf = std::numeric_limits<float>::infinity();
    planted<float, double>({-inf, -1e30, -0.0, 0.0, 0.3, 16777216.0, 16777217.0, 1e30, inf});
    planted<float, float>({-finf, -0.0f, 0.0f, 0.3f, 16777216.0f, finf});
    planted<float, int32_t>({INT32_MIN, -16777217, -1, 0, 1, 16777216, 16777217, INT32_MAX});
    planted<double, double>({-inf, -0.0, 0.0, 0.3, 9007199254740992.0, inf});
    planted<double, uint64_t>({0, 1, 9007199254740992ull, 9007199254740994ull, UINT64_MAX - 4096});  // distinct in Float64
    planted<double, float>({-finf, -0.0f, 0.0f, 0.3f, finf});
    planted<uint64_t, uint64_t>({0, 1, 9007199254740992ull, 9007199254740993ull, 9007199254740994ull, UINT64_MAX});
    planted<uint64_t, double>({-1.0, 0.0, 0.5, 9007199254740992.0, 9007199254740994.0, 18446744073709551616.0});
    planted<uint64_t, int64_t>({INT64_MIN, -1, 0, 9007199254740992ll, INT64_MAX});
    planted<int64_t, uint64_t>({0, 1, 9007199254740993ull, 9223372036854775808ull, UINT64_MAX});
    planted<int64_t, int64_t>({INT64_MIN, -9007199254740993ll, 0, 9007199254740993ll, INT64_MAX});
    planted<int64_t, double>({-inf, -9223372036854775808.0, -0.5, 0.5, 9223372036854775808.0, inf});
    planted<uint32_t, uint32_t>({0, 1, 16777217u, 2147483647u, 2147483648u, UINT32_MAX});
    planted<uint32_t, float>({-1.0f, 0.5f, 16777216.0f, 4294967296.0f});
    planted<uint32_t, int8_t>({-128, -1, 0, 1, 127});
    planted<int32_t, uint32_t>({0, 1, 2147483647u, 2147483648u, UINT32_MAX});
    planted<int32_t, double>({-2147483648.5, -0.5, 0.5, 2147483646.5, 2147483647.0, 2147483647.5});
    planted<int32_t, int32_t>({INT32_MIN, -1, 0, 1, INT32_MAX});

    // u64 2^53 + 1 compares exactly against u64 breaks and in Float64 against f64 or i64 ones
    {
        const uint64_t x = 9007199254740993ull;
        const int64_t key = ecd::order_key<uint64_t>(x);
        CHECK((rule<uint64_t, uint64_t>(key, {9007199254740992ull, 9007199254740993ull, 9007199254740994ull}, false) == 2));
        CHECK((rule<uint64_t, double>(key, {9007199254740992.0, 9007199254740994.0}, false) == 1));
        CHECK((rule<uint64_t, double>(key, {9007199254740992.0, 9007199254740994.0}, true) == 0));  // it IS 2^53 there
        CHECK((rule<uint64_t, int64_t>(key, {9007199254740992ll, 9007199254740993ll}, true) == 0));  // both breaks are 2^53 in f64: refused as breaks, but the predicate holds
    }
    // a u8 raster with breaks -1.5, 0.2, 0.7, 255.0, 300.0: repeated thresholds and an unreachable suffix
    {
        const double b[5] = {-1.5, 0.2, 0.7, 255.0, 300.0};
        ec_value vals[6];
        for (int c = 0; c < 6; ++c) vals[c] = value_of<uint8_t>(EC_U8, uint8_t(10 + c));
        ec_reclass_table tab;
        bool bad = false;
        CHECK(told(build(EC_U8, EC_F64, b, 5, 0, EC_U8, vals, nullptr, nullptr, &tab), &bad) == nullptr);
        CHECK(tab.n_reached == 4 && tab.thr[0] == 0 && tab.thr[1] == 1 && tab.thr[2] == 1 && tab.thr[3] == 255);
        CHECK(class_of(tab, 0) == 1 && class_of(tab, 1) == 3 && class_of(tab, 254) == 3 && class_of(tab, 255) == 4);
        CHECK(told(build(EC_U8, EC_F64, b, 5, 1, EC_U8, vals, nullptr, nullptr, &tab), &bad) == nullptr);
        CHECK(tab.n_reached == 3 && tab.thr[0] == 0 && tab.thr[1] == 1 && tab.thr[2] == 1);  // no u8 cell is > 255.0
        const double far[2] = {1e9, 2e9};
        CHECK(told(build(EC_U8, EC_F64, far, 2, 0, EC_U8, vals, nullptr, nullptr, &tab), &bad) == nullptr);
        CHECK(tab.n_reached == 0 && tab.n_breaks == 2);
    }
    // the refusals, in order; a refused build writes nothing
    {
        const double b[3] = {0.0, 1.0, 2.0};
        const double nan_b[3] = {0.0, std::nan(""), 2.0};
        const double flat[3] = {0.0, 1.0, 1.0};
        const int64_t same_in_f64[2] = {9007199254740992ll, 9007199254740993ll};
        ec_value vals[4], bad_vals[4];
        for (int c = 0; c < 4; ++c) bad_vals[c] = vals[c] = value_of<uint16_t>(EC_U16, uint16_t(c));
        bad_vals[3].dtype = EC_U8;
        const ec_value nd = value_of<uint16_t>(EC_U16, 65535), bad_nd = value_of<uint8_t>(EC_U8, 255);
        unsigned char canary[sizeof(ec_reclass_table)], before[sizeof(ec_reclass_table)];
        std::memset(canary, 0xA5, sizeof canary);
        std::memcpy(before, canary, sizeof before);
        ec_reclass_table* out = reinterpret_cast<ec_reclass_table*>(canary);
        bool bad = false;
        auto refused = [&](const char* why, bool type) {
            CHECK(why != nullptr && bad == type);
            CHECK(std::memcmp(canary, before, sizeof before) == 0);
            return why;
        };
        // everything wrong at once: n_breaks speaks first
        CHECK(std::strstr(refused(told(build(99, 99, nullptr, 0, 7, 99, nullptr, nullptr, nullptr, out), &bad), false), "n_breaks"));
        CHECK(std::strstr(refused(told(build(99, 99, nullptr, 256, 7, 99, nullptr, nullptr, nullptr, out), &bad), false), "n_breaks"));
        CHECK(std::strstr(refused(told(build(99, 99, nullptr, 3, 7, 99, nullptr, nullptr, nullptr, out), &bad), false), "right"));
        CHECK(std::strstr(refused(told(build(99, EC_F64, nullptr, 3, 0, EC_U16, nullptr, nullptr, nullptr, out), &bad), true), "dtype"));
        CHECK(std::strstr(refused(told(build(EC_F32, 10, nullptr, 3, 0, EC_U16, nullptr, nullptr, nullptr, out), &bad), true), "dtype"));
        CHECK(std::strstr(refused(told(build(EC_F32, EC_F64, nullptr, 3, 0, 200, nullptr, nullptr, nullptr, out), &bad), true), "dtype"));
        CHECK(std::strstr(refused(told(build(EC_F32, EC_F64, nullptr, 3, 0, EC_U16, bad_vals, nullptr, &bad_nd, out), &bad), false), "null"));
        CHECK(std::strstr(refused(told(build(EC_F32, EC_F64, nan_b, 3, 0, EC_U16, nullptr, nullptr, &bad_nd, out), &bad), false), "null"));
        CHECK(std::strstr(told(build(EC_F32, EC_F64, nan_b, 3, 0, EC_U16, bad_vals, nullptr, &bad_nd, nullptr), &bad), "null"));
        CHECK(std::strstr(refused(told(build(EC_F32, EC_F64, nan_b, 3, 0, EC_U16, bad_vals, nullptr, &bad_nd, out), &bad), false), "class value"));
        CHECK(std::strstr(refused(told(build(EC_F32, EC_F64, nan_b, 3, 0, EC_U16, vals, nullptr, &bad_nd, out), &bad), false), "nodata"));
        CHECK(std::strstr(refused(told(build(EC_F32, EC_F64, nan_b, 3, 0, EC_U16, vals, nullptr, &nd, out), &bad), false), "NaN"));
        CHECK(std::strstr(refused(told(build(EC_F32, EC_F64, flat, 3, 0, EC_U16, vals, nullptr, &nd, out), &bad), false), "ascending"));
        CHECK(std::strstr(refused(told(build(EC_F32, EC_I64, same_in_f64, 2, 0, EC_U16, vals, nullptr, &nd, out), &bad), false), "ascending"));
        CHECK(told(build(EC_I64, EC_I64, same_in_f64, 2, 0, EC_U16, vals, nullptr, &nd, out), &bad) == nullptr);  // exact in Int64
        // every byte defined: two builds into differently poisoned memory agree
        unsigned char a[sizeof(ec_reclass_table)], c[sizeof(ec_reclass_table)];
        std::memset(a, 0x00, sizeof a);
        std::memset(c, 0xFF, sizeof c);
        const uint8_t valid[4] = {1, 0, 7, 1};
        CHECK(told(build(EC_F32, EC_F64, b, 3, 1, EC_U16, vals, valid, &nd, reinterpret_cast<ec_reclass_table*>(a)), &bad) == nullptr);
        CHECK(told(build(EC_F32, EC_F64, b, 3, 1, EC_U16, vals, valid, &nd, reinterpret_cast<ec_reclass_table*>(c)), &bad) == nullptr);
        CHECK(std::memcmp(a, c, sizeof a) == 0);
        ec_reclass_table tab;
        std::memcpy(&tab, a, sizeof tab);
        CHECK(tab.t == EC_F32 && tab.dt == EC_U16 && tab.n_breaks == 3 && tab.n_reached == 3 && tab.flags == (EC_RECLASS_HAS_NODATA | EC_RECLASS_DROPS));
        CHECK(tab.nodata_bits == 65535 && tab.reserved0 == 0 && tab.reserved1 == 0);
        CHECK(tab.valid[0] == 1 && tab.valid[1] == 0 && tab.valid[2] == 1 && tab.valid[3] == 1 && tab.valid[4] == 0 && tab.valid[255] == 0);
        CHECK(tab.value_bits[3] == 3 && tab.value_bits[4] == 0);
        CHECK(told(build(EC_F32, EC_F64, b, 3, 1, EC_U16, vals, nullptr, nullptr, &tab), &bad) == nullptr && tab.flags == 0 && tab.valid[3] == 1 && tab.valid[4] == 0);
    }
    // ec_reclass's refusals, in order
    {
        alignas(16) static unsigned char mem[8192 + EC_RECLASS_TABLE_BYTES];
        unsigned char* src = mem; unsigned char* dst = mem + 1024; unsigned char* dm = mem + 3072; unsigned char* tab = mem + 8192;
        bool bad = false;
        CHECK(std::strstr(told(reclass_refusal(0, 1, nullptr, nullptr, 5, nullptr, nullptr, nullptr), &bad), "dtype") && bad);
        CHECK(std::strstr(told(reclass_refusal(1, 0, nullptr, nullptr, 5, nullptr, nullptr, nullptr), &bad), "dtype") && bad);
        CHECK(told(reclass_refusal(1, 2, nullptr, nullptr, 0, nullptr, nullptr, nullptr), &bad) == nullptr && !bad);
        CHECK(std::strstr(told(reclass_refusal(1, 2, nullptr, nullptr, 5, tab + 1, dst, nullptr), &bad), "null") && !bad);
        CHECK(std::strstr(told(reclass_refusal(1, 2, src, nullptr, 5, nullptr, dst, nullptr), &bad), "null"));
        CHECK(std::strstr(told(reclass_refusal(1, 2, src, nullptr, 5, tab + 1, nullptr, nullptr), &bad), "null"));
        CHECK(std::strstr(told(reclass_refusal(1, 2, src, nullptr, 5, tab + 8, src, nullptr), &bad), "16-byte"));
        CHECK(std::strstr(told(reclass_refusal(8, 8, src, nullptr, size_t(1) << 42, tab, src, nullptr), &bad), "tiles"));
        CHECK(std::strstr(told(reclass_refusal(1, 2, src, nullptr, 100, tab, src + 99, nullptr), &bad), "dst overlaps"));
        CHECK(std::strstr(told(reclass_refusal(1, 2, src, dst + 199, 100, tab, dst, nullptr), &bad), "dst overlaps"));
        CHECK(std::strstr(told(reclass_refusal(1, 2, src, nullptr, 100, dst + 16, dst, nullptr), &bad), "dst overlaps"));
        CHECK(std::strstr(told(reclass_refusal(1, 2, src, nullptr, 100, tab, dst, src + 50), &bad), "dst_mask overlaps an input"));
        CHECK(std::strstr(told(reclass_refusal(1, 2, src, nullptr, 100, tab, dst, tab + 4000), &bad), "dst_mask overlaps an input"));
        CHECK(std::strstr(told(reclass_refusal(1, 2, src, nullptr, 100, tab, dst, dst + 199), &bad), "dst_mask overlaps dst"));
        CHECK(told(reclass_refusal(1, 2, src, src + 100, 100, tab, dst, dm), &bad) == nullptr);
    }
    std::printf("test_reclass_plan: %d checks passed\n", g_checks);
    return 0;
}
