// test_composite_cell.cpp — the fold steps of ec_composite (csrc/ec_composite_cell.hpp: composite_init / composite_step /
// composite_finish), run from the header alone under a plain C++ compiler: the very functions the kernels run.  Links nothing
// from the library.
//
// For every cell type and op, stacks of 1 .. 64 cells drawn from the type's special values (extremes, signed zeros, NaNs of both
// signs, integers beyond 2^53) under random validity, every min_count: the fold must give what an independent statement of the
// header's rule gives — the valid cells listed first, then picked by position or by a three-way total order written here without
// order_key, or summed in a plain loop.  Also the stated cells: the sum of a single -0.0, a tie, count < min_count.
// Built plain and, as test_composite_cell_san, under the address and undefined-behaviour sanitizers.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>

#include "ec_composite_cell.hpp"

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
static std::vector<T> specials() {
    std::vector<T> s;
    using lim = std::numeric_limits<T>;
    if constexpr (std::is_floating_point<T>::value) {
        const T big = sizeof(T) == 4 ? T(0x1p60) : T(1e16);
        for (T v : {T(0), T(-0.0), T(1), T(-1), T(3), T(0.1), T(128), big, T(-big), lim::max(), lim::lowest(), lim::min(), lim::denorm_min(),
                    lim::infinity(), T(-lim::infinity()), lim::quiet_NaN(), T(-lim::quiet_NaN())})
            s.push_back(v);
    } else {
        for (T v : {T(0), T(1), T(2), T(7), lim::max(), T(lim::max() - 1), T(lim::max() / 2), T(lim::max() / 2 + 1), lim::min(), T(lim::min() + 1)}) s.push_back(v);
        if constexpr (sizeof(T) == 8) {
            s.push_back(T((uint64_t(1) << 53) + 1));
            s.push_back(T((uint64_t(1) << 53) + 3));
            s.push_back(T((uint64_t(1) << 62) + 1025));
        }
        if constexpr (std::is_signed<T>::value) {
            s.push_back(T(-1));
            s.push_back(T(-2));
        }
    }
    return s;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return uint32_t(g_rng >> 32);
}

static bool same_f64(double a, double b) { return bits_of(a) == bits_of(b) || (std::isnan(a) && std::isnan(b)); }

template <typename T, int OP>
static void run_stack(const std::vector<T>& cells, const std::vector<bool>& valid, uint32_t min_count, const char* type) {
    const int k_layers = int(cells.size());
    auto s = composite_init<T, OP>();
    for (int k = 0; k < k_layers; ++k) composite_step<T, OP>(s, cells[k], valid[k], uint32_t(k));
    uint8_t mask = 7, aux = 7;
    const auto got = composite_finish<T, OP>(s, min_count, false, &mask, &aux);
    // the rule, stated independently
    std::vector<int> at;
    for (int k = 0; k < k_layers; ++k)
        if (valid[k]) at.push_back(k);
    const bool ok = at.size() >= min_count;
    CHECK(mask == (ok ? 1 : 0), "%s op %d: mask %d", type, OP, int(mask));
    if constexpr (OP == kCompositeSum) {
        double acc = 0.0;
        for (int k : at) acc = acc + static_cast<double>(cells[k]);
        CHECK(aux == at.size(), "%s sum: aux %d, count %zu", type, int(aux), at.size());
        CHECK(same_f64(got, ok ? acc : 0.0), "%s sum of %d layers", type, k_layers);
        uint8_t m2, a2;
        const double mean = composite_finish<T, OP>(s, min_count, true, &m2, &a2);
        CHECK(same_f64(mean, ok ? acc / double(at.size()) : 0.0) && m2 == mask && a2 == aux, "%s mean of %d layers", type, k_layers);
        if (!ok) CHECK(bits_of(got) == 0 && bits_of(mean) == 0, "%s: an invalid cell is all-zero bits", type);
    } else {
        int pick = -1;
        for (int k : at) {
            if (pick < 0) pick = k;
            else if (OP == kCompositeLast) pick = k;
            else if (OP == kCompositeMin && total_order<T>(cells[k], cells[pick]) < 0) pick = k;
            else if (OP == kCompositeMax && total_order<T>(cells[k], cells[pick]) > 0) pick = k;
        }
        if (ok) {
            CHECK(aux == pick, "%s op %d: aux %d, picked %d of %d", type, OP, int(aux), pick, k_layers);
            CHECK(bits_of(got) == bits_of(cells[pick]), "%s op %d: bits", type, OP);
        } else {
            CHECK(aux == kCompositeNone && bits_of(got) == 0, "%s op %d: an invalid cell is zero bits and aux 255", type, OP);
        }
    }
}

template <typename T>
static void run_type(const char* type) {
    const std::vector<T> sp = specials<T>();
    for (int k_layers : {1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 63, 64}) {
        for (int rep = 0; rep < 40; ++rep) {
            std::vector<T> cells(k_layers);
            std::vector<bool> valid(k_layers);
            const uint32_t density = rep % 4;  // 0: none masked out .. 3: most
            for (int k = 0; k < k_layers; ++k) {
                cells[k] = sp[rnd() % sp.size()];
                valid[k] = density == 0 || rnd() % 4 >= density;
            }
            if (rep == 1) std::fill(valid.begin(), valid.end(), false);
            for (uint32_t mc : {1u, 2u, uint32_t(k_layers)}) {
                if (mc > uint32_t(k_layers)) continue;
                run_stack<T, kCompositeFirst>(cells, valid, mc, type);
                run_stack<T, kCompositeLast>(cells, valid, mc, type);
                run_stack<T, kCompositeMin>(cells, valid, mc, type);
                run_stack<T, kCompositeMax>(cells, valid, mc, type);
                run_stack<T, kCompositeSum>(cells, valid, mc, type);
            }
        }
    }
}

static void stated_cells() {
    uint8_t m, a;
    {  // the sum of a single -0.0 is +0.0; MIN copies the bits
        auto s = composite_init<double, kCompositeSum>();
        composite_step<double, kCompositeSum>(s, -0.0, true, 0);
        CHECK((bits_of(composite_finish<double, kCompositeSum>(s, 1, false, &m, &a)) == 0 && m == 1 && a == 1), "sum of -0.0");
        auto p = composite_init<double, kCompositeMin>();
        composite_step<double, kCompositeMin>(p, -0.0, true, 0);
        CHECK((bits_of(composite_finish<double, kCompositeMin>(p, 1, false, &m, &a)) == uint64_t(1) << 63 && a == 0), "min of -0.0");
    }
    {  // a tie keeps the least k; -0.0 is less than +0.0
        auto s = composite_init<uint16_t, kCompositeMax>();
        const uint16_t col[5] = {7, 9, 9, 7, 8};
        for (uint32_t k = 0; k < 5; ++k) composite_step<uint16_t, kCompositeMax>(s, col[k], true, k);
        CHECK((composite_finish<uint16_t, kCompositeMax>(s, 1, false, &m, &a) == 9 && a == 1), "tie of the maximum");
        auto z = composite_init<float, kCompositeMin>();
        composite_step<float, kCompositeMin>(z, 0.0f, true, 0);
        composite_step<float, kCompositeMin>(z, -0.0f, true, 1);
        CHECK((bits_of(composite_finish<float, kCompositeMin>(z, 1, false, &m, &a)) == 0x80000000u && a == 1), "-0.0 < +0.0");
    }
    {  // an invalid layer contributes nothing, not even a NaN; count < min_count stores zero bits
        auto s = composite_init<float, kCompositeSum>();
        composite_step<float, kCompositeSum>(s, std::numeric_limits<float>::quiet_NaN(), false, 0);
        composite_step<float, kCompositeSum>(s, 2.5f, true, 1);
        CHECK((composite_finish<float, kCompositeSum>(s, 1, true, &m, &a) == 2.5 && m == 1 && a == 1), "NaN under a cleared mask byte");
        CHECK((bits_of(composite_finish<float, kCompositeSum>(s, 2, true, &m, &a)) == 0 && m == 0 && a == 1), "count < min_count");
    }
    {  // u64 above 2^53: double() rounds, then every addition rounds
        auto s = composite_init<uint64_t, kCompositeSum>();
        const uint64_t col[3] = {(uint64_t(1) << 53) + 1, 1, 3};
        for (uint32_t k = 0; k < 3; ++k) composite_step<uint64_t, kCompositeSum>(s, col[k], true, k);
        CHECK((composite_finish<uint64_t, kCompositeSum>(s, 1, false, &m, &a) == 0x1p53 + 4.0), "u64 above 2^53");
    }
    static_assert(valid_composite_op(0) && valid_composite_op(5) && !valid_composite_op(-1) && !valid_composite_op(6), "ec_composite_op is 0..5");
    static_assert(composite_sums(4) && composite_sums(5) && !composite_sums(3), "SUM and MEAN");
    static_assert((std::is_same<composite_result<uint8_t, kCompositeMean>::type, double>::value) && (std::is_same<composite_result<int8_t, kCompositeMax>::type, int8_t>::value), "result types");
}

int main() {
    stated_cells();
    run_type<uint8_t>("u8");
    run_type<uint16_t>("u16");
    run_type<uint32_t>("u32");
    run_type<uint64_t>("u64");
    run_type<int8_t>("i8");
    run_type<int16_t>("i16");
    run_type<int32_t>("i32");
    run_type<int64_t>("i64");
    run_type<float>("f32");
    run_type<double>("f64");
    if (g_failed) {
        std::fprintf(stderr, "%lu of %lu checks FAILED\n", g_failed, g_checks);
        return 1;
    }
    std::printf("%lu checks passed\n", g_checks);
    return 0;
}
