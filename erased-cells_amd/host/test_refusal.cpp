// test_refusal.cpp — csrc/ec_refusal.hpp alone, under a plain C++17 compiler (and, as test_refusal_san, under the address and
// undefined-behaviour sanitizers): the interval test on blocks that touch, nest, are equal, are absent or empty, or end at the last
// address; the walk over a table of overlaps; the alignment test; the refusal value.  Addresses are plain integers, never
// dereferenced.  Needs no GPU and nothing from the library.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ec_refusal.hpp"

static int g_checks = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) {                                                                 \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

using namespace ecv;

static const void* at(uintptr_t a) { return reinterpret_cast<const void*>(a); }
// both argument orders and both spellings agree
static bool meet(uintptr_t a, size_t abytes, uintptr_t b, size_t bbytes) {
    const bool one = overlap(at(a), abytes, at(b), bbytes);
    CHECK(one == overlap(at(b), bbytes, at(a), abytes));
    CHECK(one == overlap(Span{at(a), abytes}, Span{at(b), bbytes}));
    return one;
}

int main() {
    // touching, by one byte, nested, equal
    CHECK(!meet(1000, 100, 1100, 50) && meet(1000, 101, 1100, 50) && meet(1000, 100, 1099, 1));
    CHECK(!meet(1000, 100, 900, 100) && meet(1000, 100, 900, 101));
    CHECK(meet(1000, 100, 1010, 10) && meet(1000, 100, 1000, 1) && meet(1000, 100, 1099, 1) && !meet(1000, 100, 999, 1));
    CHECK(meet(1000, 100, 1000, 100) && meet(1000, 1, 1000, 1));
    // every pair of small blocks against the bytes themselves
    for (uintptr_t a = 1; a < 8; ++a)
        for (size_t ab = 0; ab < 5; ++ab)
            for (uintptr_t b = 1; b < 8; ++b)
                for (size_t bb = 0; bb < 5; ++bb) {
                    bool shared = false;
                    for (uintptr_t x = a; x < a + ab; ++x) shared = shared || (x >= b && x < b + bb);
                    CHECK(meet(a, ab, b, bb) == shared);
                }
    // an absent block or an empty one overlaps nothing, itself included
    CHECK(!meet(0, 100, 0, 100) && !meet(0, 100, 50, 100) && !meet(0, SIZE_MAX, 1, SIZE_MAX));
    CHECK(!meet(1000, 0, 1000, 100) && !meet(1050, 0, 1000, 100) && !meet(1000, 0, 1000, 0));
    // blocks that end at the last address: no end is computed, so none wraps
    const uintptr_t top = UINTPTR_MAX;
    CHECK(meet(top - 9, 10, top, 1) && meet(top - 9, 10, top - 9, 10) && meet(top - 99, 100, top - 9, 10) && meet(top, 1, top, 1));
    CHECK(!meet(top - 9, 10, top - 19, 10) && meet(top - 9, 10, top - 19, 11) && !meet(top - 9, 10, 1, 100));
    CHECK(meet(1, SIZE_MAX, top, 1) && meet(1, SIZE_MAX, 1, 1) && !meet(2, SIZE_MAX - 1, 1, 1));

    // the alignment test: never on an absent pointer
    CHECK(!misaligned(nullptr, 1) && !misaligned(nullptr, 2) && !misaligned(nullptr, 8) && !misaligned(nullptr, 16));
    CHECK(!misaligned(at(4096), 16) && misaligned(at(4097), 2) && misaligned(at(4104), 16) && !misaligned(at(4104), 8) && !misaligned(at(4097), 1));
    CHECK(misaligned(at(top), 2) && !misaligned(at(top - 15), 16));

    // the table walk: the first row that overlaps, whatever comes after it; null for none
    const Span a{at(1000), 100}, b{at(1100), 100}, c{at(1150), 100}, none{nullptr, 100}, empty{at(1000), 0};
    {
        const OverlapRow rows[] = {{a, b, "a on b"}, {none, a, "nothing on a"}, {empty, a, "no bytes on a"}, {b, c, "b on c"}, {c, b, "c on b"}, {a, a, "a on a"}};
        CHECK(std::strcmp(first_overlap(rows), "b on c") == 0);
    }
    {
        const OverlapRow rows[] = {{a, a, "a on a"}, {b, c, "b on c"}};
        CHECK(std::strcmp(first_overlap(rows), "a on a") == 0);
    }
    {
        const OverlapRow rows[] = {{a, b, "a on b"}, {a, c, "a on c"}, {none, none, "nothing"}};
        CHECK(first_overlap(rows) == nullptr);
        const OverlapRow last[] = {{a, b, "a on b"}, {a, c, "a on c"}, {c, b, "c on b"}};
        CHECK(std::strcmp(first_overlap(last), "c on b") == 0);
    }

    // the refusal value
    const Refusal pass{}, arg{"why"}, type{"bad", true}, walked{first_overlap({{a, b, "a on b"}})};
    CHECK(!pass && pass.why == nullptr && !pass.bad_type && !walked);
    CHECK(arg && !arg.bad_type && std::strcmp(arg.why, "why") == 0 && type && type.bad_type);

    std::printf("test_refusal: %d checks passed\n", g_checks);
    return 0;
}
