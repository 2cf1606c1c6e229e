// test_cast_cell.cpp — cast_as, cast_round and scaled (csrc/ec_cast_cell.hpp), the per-cell functions of ec_cast / ec_cast_scaled,
// run from the header alone under a plain C++ compiler: the very functions the kernels run.  Links nothing from the library.
//
// stdin: lines `st dt bits` — two dtype codes (decimal) and the source cell's bits (hex, zero-extended to 64) — or
// `st dt bits scale_bits offset_bits` with the two f64 parameters of `scaled` as hex bits.
// stdout: per 3-field line `as round` — the destination cell's bits (hex) under EC_CAST_AS and EC_CAST_ROUND; per 5-field line
// the bits of scaled's cell; `all lines answered: N` at the end.  tests/test_cast_ref.py feeds every pair over the special-values
// table and compares with tests/cast_ref.py.  Built plain and, as test_cast_cell_san, under the address and
// undefined-behaviour sanitizers (float-cast-overflow among them: no out-of-range float-to-integer cast may be reached).
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "ec_cast_cell.hpp"

enum { U8, U16, U32, U64, I8, I16, I32, I64, F32, F64 };  // ec_dtype, with_ct! order

#define WITH_CT(X) \
    X(U8, uint8_t) X(U16, uint16_t) X(U32, uint32_t) X(U64, uint64_t) X(I8, int8_t) X(I16, int16_t) X(I32, int32_t) X(I64, int64_t) \
    X(F32, float) X(F64, double)

template <typename T>
static T cell_of_bits(uint64_t bits) {
    T v;
    std::memcpy(&v, &bits, sizeof v);  // little-endian: the low bytes
    return v;
}
template <typename T>
static uint64_t bits_of_cell(T v) {
    uint64_t bits = 0;
    std::memcpy(&bits, &v, sizeof v);
    return bits;
}

struct Query {
    uint64_t bits;
    bool scaled;
    double scale, offset;
};

template <typename S, typename D>
static void answer(const Query& q) {
    const S v = cell_of_bits<S>(q.bits);
    if (q.scaled) std::printf("%" PRIx64 "\n", bits_of_cell<D>(ecd::scaled<S, D>(v, q.scale, q.offset)));
    else std::printf("%" PRIx64 " %" PRIx64 "\n", bits_of_cell<D>(ecd::cast_as<S, D>(v)), bits_of_cell<D>(ecd::cast_round<S, D>(v)));
}

template <typename S>
static bool answer_s(int dt, const Query& q) {
#define ROW(ID, T) case ID: answer<S, T>(q); return true;
    switch (dt) { WITH_CT(ROW) }
#undef ROW
    return false;
}

int main() {
    static_assert(ecd::cell_limits<int8_t>::lo == -128 && ecd::cell_limits<int8_t>::hi == 127 && ecd::cell_limits<uint16_t>::hi == 65535, "limits");
    static_assert(ecd::cell_limits<int64_t>::lo == INT64_MIN && ecd::cell_limits<uint64_t>::hi == UINT64_MAX, "limits");
    char line[256];
    unsigned long lines = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        int st, dt;
        uint64_t sb = 0, ob = 0;
        Query q{};
        const int got = std::sscanf(line, "%d %d %" SCNx64 " %" SCNx64 " %" SCNx64, &st, &dt, &q.bits, &sb, &ob);
        if (got != 3 && got != 5) {
            std::fprintf(stderr, "line %lu: %d fields\n", lines + 1, got);
            return 1;
        }
        q.scaled = got == 5;
        q.scale = cell_of_bits<double>(sb);
        q.offset = cell_of_bits<double>(ob);
        bool ok = false;
#define ROW(ID, T) case ID: ok = answer_s<T>(dt, q); break;
        switch (st) { WITH_CT(ROW) }
#undef ROW
        if (!ok) {
            std::fprintf(stderr, "line %lu: bad dtype %d / %d\n", lines + 1, st, dt);
            return 1;
        }
        ++lines;
    }
    std::printf("all lines answered: %lu\n", lines);
    return 0;
}
