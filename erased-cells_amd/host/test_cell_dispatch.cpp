// test_cell_dispatch.cpp — the cell-type dispatcher (csrc/ec_dispatch.hpp) and the type list it switches over
// (csrc/ec_lattice.hpp) alone, under a plain C++17 compiler: every code reaches its type exactly once, a pair in argument
// order, and any other code reaches nothing and gives the fallback back.  Prints "cell dispatch ok" and exits 0, or says
// what failed and exits 1.
#include <climits>
#include <cstdio>
#include <type_traits>

#include "ec_dispatch.hpp"
#include "ec_lattice.hpp"

using ecl::cell_t;

#define EC_CHECK_ROUND_TRIP(ID, T)                                                                   \
    static_assert(std::is_same<ecl::cell_of<ecl::dtype_of<T>::value>::type, T>::value, "cell_of<dtype_of<T>> is T"); \
    static_assert(ecl::dtype_of<ecl::cell_of<ID>::type>::value == ID, "dtype_of<cell_of<ID>> is ID");
EC_WITH_CT(EC_CHECK_ROUND_TRIP)
#undef EC_CHECK_ROUND_TRIP
static_assert(std::is_same<ecl::cell_of<EC_U8>::type, uint8_t>::value && std::is_same<ecl::cell_of<EC_U16>::type, uint16_t>::value &&
                  std::is_same<ecl::cell_of<EC_U32>::type, uint32_t>::value && std::is_same<ecl::cell_of<EC_U64>::type, uint64_t>::value &&
                  std::is_same<ecl::cell_of<EC_I8>::type, int8_t>::value && std::is_same<ecl::cell_of<EC_I16>::type, int16_t>::value &&
                  std::is_same<ecl::cell_of<EC_I32>::type, int32_t>::value && std::is_same<ecl::cell_of<EC_I64>::type, int64_t>::value &&
                  std::is_same<ecl::cell_of<EC_F32>::type, float>::value && std::is_same<ecl::cell_of<EC_F64>::type, double>::value,
              "the ten cell types, written out once more");

static int failures = 0;
#define EXPECT(cond, ...)                    \
    do {                                     \
        if (!(cond)) {                       \
            ++failures;                      \
            std::printf("FAILED %s: ", #cond); \
            std::printf(__VA_ARGS__);        \
            std::printf("\n");               \
        }                                    \
    } while (0)

static const int kBad[] = {-1, 10, 255, INT_MAX};
constexpr int kFallback = -77;

static void single_codes() {
    for (int t = 0; t < EC_NTYPES; ++t) {
        int calls = 0, code = -1;
        size_t size = 0;
        const int got = ecl::with_cell_type(t, [&](auto c) {
            using T = cell_t<decltype(c)>;
            ++calls;
            code = ecl::dtype_of<T>::value;
            size = sizeof(T);
            return 1000 + ecl::dtype_of<T>::value;
        }, kFallback);
        EXPECT(calls == 1 && code == t && size == ecl::size_of(t) && got == 1000 + t, "code %d: %d calls, tag %d of %zu bytes, result %d", t, calls, code, size, got);
    }
    for (int t : kBad) {
        int calls = 0, lazy = 0;
        const int got = ecl::with_cell_type(t, [&](auto) { ++calls; return 0; }, kFallback);
        EXPECT(calls == 0 && got == kFallback, "code %d: %d calls, result %d", t, calls, got);
        const int got2 = ecl::with_cell_type(t, [&](auto) { ++calls; return 0; }, [&] { ++lazy; return kFallback; });
        EXPECT(calls == 0 && lazy == 1 && got2 == kFallback, "code %d, callable fallback: %d calls, run %d times, result %d", t, calls, lazy, got2);
    }
    // a callable fallback is not run for a code that has a type
    int lazy = 0;
    const int got = ecl::with_cell_type(EC_F32, [&](auto c) { return int(sizeof(cell_t<decltype(c)>)); }, [&] { ++lazy; return kFallback; });
    EXPECT(lazy == 0 && got == 4, "callable fallback run %d times for EC_F32, result %d", lazy, got);
}

static void pairs() {
    for (int a = 0; a < EC_NTYPES; ++a)
        for (int b = 0; b < EC_NTYPES; ++b) {
            int calls = 0, first = -1, second = -1, lazy = 0;
            const int got = ecl::with_cell_types(a, b, [&](auto ca, auto cb) {
                ++calls;
                first = ecl::dtype_of<cell_t<decltype(ca)>>::value;
                second = ecl::dtype_of<cell_t<decltype(cb)>>::value;
                return 100 * first + second;
            }, [&] { ++lazy; return kFallback; });
            EXPECT(calls == 1 && lazy == 0 && first == a && second == b && got == 100 * a + b, "pair (%d, %d): %d calls with (%d, %d), result %d", a, b, calls, first, second, got);
        }
    for (int bad : kBad)
        for (int good = 0; good <= EC_NTYPES; ++good) {  // good == EC_NTYPES: both positions bad
            const int other = good < EC_NTYPES ? good : bad;
            const int pair[2][2] = {{bad, other}, {other, bad}};
            for (const auto& p : pair) {
                int calls = 0;
                const int got = ecl::with_cell_types(p[0], p[1], [&](auto, auto) { ++calls; return 0; }, kFallback);
                EXPECT(calls == 0 && got == kFallback, "pair (%d, %d): %d calls, result %d", p[0], p[1], calls, got);
            }
        }
}

static void widths() {
    for (size_t bytes = 0; bytes <= 17; ++bytes) {
        int calls = 0;
        bool is_unsigned_word = false;
        const int got = ecl::with_cell_width(bytes, [&](auto w) {
            using W = cell_t<decltype(w)>;
            ++calls;
            is_unsigned_word = std::is_same<W, uint8_t>::value || std::is_same<W, uint16_t>::value || std::is_same<W, uint32_t>::value || std::is_same<W, uint64_t>::value;
            return int(sizeof(W));
        }, kFallback);
        if (bytes == 1 || bytes == 2 || bytes == 4 || bytes == 8)
            EXPECT(calls == 1 && is_unsigned_word && got == int(bytes), "width %zu: %d calls, result %d", bytes, calls, got);
        else
            EXPECT(calls == 0 && got == kFallback, "width %zu: %d calls, result %d", bytes, calls, got);
    }
    const int got = ecl::with_cell_width(ecl::size_of(EC_NTYPES), [](auto) { return 0; }, kFallback);  // size_of a bad code is 0
    EXPECT(got == kFallback, "the width of a bad code: result %d", got);
}

static void values() {
    ec_value v;
    ecl::put_value<float>(&v, EC_F32, -2.5f);
    EXPECT(v.dtype == EC_F32 && ecl::value_as<float>(v) == -2.5f && (v.v.bits >> 32) == 0, "put_value / value_as of an f32: %g, bits %llx", double(ecl::value_as<float>(v)), (unsigned long long)v.v.bits);
    ecl::put_value<int64_t>(&v, EC_I64, INT64_MIN);
    EXPECT(v.dtype == EC_I64 && ecl::value_as<int64_t>(v) == INT64_MIN && ecl::value_as<uint8_t>(v) == 0, "put_value / value_as of an i64");
}

int main() {
    single_codes();
    pairs();
    widths();
    values();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("cell dispatch ok\n");
    return 0;
}
