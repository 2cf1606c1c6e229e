// ec_refusal.hpp — what the argument checks of the raster families (ec_distance, ec_regions, ec_zonal*, ec_zonal_table*, ec_reclass)
// share, in plain C++: the verdict of a check, the interval test, the alignment test, and the walk over a family's table of
// overlaps.  A family's refusal function returns a Refusal; its overlap step is one table of OverlapRow in the order
// include/erased_cells.h states, so that order is data a reader sees.  ecd::refused (ec_runtime.hpp) turns a Refusal into the
// call's status and error text.
//
// Self-contained: nothing from this library and no HIP include, so that host/test_refusal.cpp and the families' own host programs
// run these very functions under the address and undefined-behaviour sanitizers.  Pointers are compared as integers and never
// dereferenced.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace ecv {

// Why a call is refused, or nothing (why null).  bad_type: the status is EC_ERR_UNSUPPORTED_TYPE, else EC_ERR_ARG.
struct Refusal {
    const char* why = nullptr;
    bool bad_type = false;
    explicit operator bool() const { return why != nullptr; }
};

// `bytes` bytes from p on.  A null p or no bytes: nothing, which overlaps nothing.
struct Span {
    const void* p;
    size_t bytes;
};

// Do the two intervals share a byte?  Decided from the distance of the two starts, so no end is computed: an interval that ends
// at the last address is like any other.
inline bool overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
    if (!a || !b || abytes == 0 || bbytes == 0) return false;
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y ? y - x < abytes : x - y < bbytes;
}
inline bool overlap(Span a, Span b) { return overlap(a.p, a.bytes, b.p, b.bytes); }

// Is p off a multiple of k bytes (k > 0)?  Never for a null p: an absent optional argument passes every alignment test.
inline bool misaligned(const void* p, size_t k) { return reinterpret_cast<uintptr_t>(p) % k != 0; }

// One overlap a family refuses, and its text.
struct OverlapRow {
    Span a, b;
    const char* text;
};

// The text of the first row whose two spans overlap, or null.
template <size_t N>
inline const char* first_overlap(const OverlapRow (&rows)[N]) {
    for (const OverlapRow& r : rows)
        if (overlap(r.a, r.b)) return r.text;
    return nullptr;
}

}  // namespace ecv
