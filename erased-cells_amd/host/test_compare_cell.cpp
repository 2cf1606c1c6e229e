// test_compare_cell.cpp — cell_cmp (csrc/ec_compare_cell.hpp), the one per-cell function of ec_compare / ec_compare_scalar, run
// from the header alone under a plain C++ compiler: the very function the kernels run.  Links nothing from the library.
//
// stdin: lines `lt rt lbits rbits` — two dtype codes (decimal) and the two cells' bits (hex, zero-extended to 64).
// stdout: per line the six results for rel = 1..6 (EC_CMP_LT, EQ, LE, GT, NE, GE) as six characters 0 / 1, and
// `all lines answered` at the end.  tests/test_compare_cell.py feeds the special-values cross product of all 100 type pairs
// and compares with tests/compare_ref.py.  Built plain and, as test_compare_cell_san, under the address and
// undefined-behaviour sanitizers.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "ec_compare_cell.hpp"

#define WITH_CT(X) \
    X(EC_U8, uint8_t) X(EC_U16, uint16_t) X(EC_U32, uint32_t) X(EC_U64, uint64_t) X(EC_I8, int8_t) X(EC_I16, int16_t) \
    X(EC_I32, int32_t) X(EC_I64, int64_t) X(EC_F32, float) X(EC_F64, double)

template <typename T>
static T cell_of_bits(uint64_t bits) {
    T v;
    std::memcpy(&v, &bits, sizeof v);  // little-endian: the low bytes
    return v;
}

template <typename L, typename R>
static void answer(uint64_t lb, uint64_t rb, char out[7]) {
    const L l = cell_of_bits<L>(lb);
    const R r = cell_of_bits<R>(rb);
    for (uint32_t rel = 1; rel <= 6; ++rel) out[rel - 1] = ecd::cell_cmp<L, R>(l, r, rel) ? '1' : '0';
    out[6] = 0;
}

template <typename L>
static bool answer_l(int rt, uint64_t lb, uint64_t rb, char out[7]) {
#define ROW(ID, T) case ID: answer<L, T>(lb, rb, out); return true;
    switch (rt) { WITH_CT(ROW) }
#undef ROW
    return false;
}

int main() {
    static_assert(ecd::valid_relation(1) && ecd::valid_relation(6) && !ecd::valid_relation(0) && !ecd::valid_relation(7), "ec_cmp is 1..6");
    int lt, rt;
    uint64_t lb, rb;
    unsigned long lines = 0;
    while (std::scanf("%d %d %" SCNx64 " %" SCNx64, &lt, &rt, &lb, &rb) == 4) {
        char out[7];
        bool ok = false;
#define ROW(ID, T) case ID: ok = answer_l<T>(rt, lb, rb, out); break;
        switch (lt) { WITH_CT(ROW) }
#undef ROW
        if (!ok) {
            std::fprintf(stderr, "line %lu: bad dtype %d / %d\n", lines + 1, lt, rt);
            return 1;
        }
        std::puts(out);
        ++lines;
    }
    std::printf("all lines answered: %lu\n", lines);
    return 0;
}
