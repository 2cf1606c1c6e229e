// ec_dispatch.hpp — from an ec_dtype code to code instantiated on the C type: the one `match` that `with_ct!` stamps in the
// reference (src/lib.rs:85-101), for every type-erased entry point of the library.
//
//   with_cell_type(t, f, otherwise)      f(cell_tag<T>{}) for the T whose code is t
//   with_cell_types(a, b, f, otherwise)  f(cell_tag<A>{}, cell_tag<B>{}), a first
//   with_cell_width(bytes, f, otherwise) f(cell_tag<W>{}), W the unsigned word of 1, 2, 4 or 8 bytes (kernels that only move cells)
//
// f is a generic lambda; cell_t<decltype(tag)> is the type.  For any other code or width f is NOT called and `otherwise` comes
// back: a value, or a callable that is run only then (a refusal that records its text: `[] { return set_error(...); }`).  The
// result type is f's.  Plain switches over EC_WITH_CT (ec_lattice.hpp), inlined: nothing is looked up at run time.
//
// Host code with no HIP include: host/test_cell_dispatch.cpp runs it under a plain C++17 compiler.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "ec_lattice.hpp"

namespace ecl {

template <typename T>
struct cell_tag { using type = T; };
template <typename Tag>
using cell_t = typename Tag::type;

template <typename R, typename Otherwise>
inline R no_cell_type(const Otherwise& otherwise) {
    if constexpr (std::is_invocable_v<const Otherwise&>) return otherwise();
    else return otherwise;
}

template <typename F, typename Otherwise>
inline auto with_cell_type(int t, F&& f, const Otherwise& otherwise) -> decltype(f(cell_tag<uint8_t>{})) {
    switch (t) {
#define EC_ROW(ID, T) case ID: return f(cell_tag<T>{});
        EC_WITH_CT(EC_ROW)
#undef EC_ROW
    }
    return no_cell_type<decltype(f(cell_tag<uint8_t>{}))>(otherwise);
}

template <typename F, typename Otherwise>
inline auto with_cell_types(int a, int b, F&& f, const Otherwise& otherwise) -> decltype(f(cell_tag<uint8_t>{}, cell_tag<uint8_t>{})) {
    return with_cell_type(a, [&](auto ta) { return with_cell_type(b, [&](auto tb) { return f(ta, tb); }, otherwise); }, otherwise);
}

template <typename F, typename Otherwise>
inline auto with_cell_width(size_t bytes, F&& f, const Otherwise& otherwise) -> decltype(f(cell_tag<uint8_t>{})) {
    switch (bytes) {
        case 1: return f(cell_tag<uint8_t>{});
        case 2: return f(cell_tag<uint16_t>{});
        case 4: return f(cell_tag<uint32_t>{});
        case 8: return f(cell_tag<uint64_t>{});
    }
    return no_cell_type<decltype(f(cell_tag<uint8_t>{}))>(otherwise);
}

// the scalar of an ec_value: T's bytes at the start of the payload, whatever the tag says
template <typename T>
inline T value_as(const ec_value& v) {
    T x;
    memcpy(&x, &v.v, sizeof x);
    return x;
}
template <typename T>
inline void put_value(ec_value* out, int dtype, T x) {
    memset(out, 0, sizeof *out);
    out->dtype = static_cast<uint8_t>(dtype);
    memcpy(&out->v, &x, sizeof x);
}

}  // namespace ecl
