// ec_compare.hip — ec_compare, ec_compare_scalar, ec_select, ec_masked_select (include/erased_cells.h): per-cell order
// predicates as masks and the pick of cells by a mask, in a translation unit of their own so the build stays parallel.
//
// Every refusal is decided on the host before any device work and before the library asks for a device.  The family
// launches at the default tile shape only (launch_map<kDefaultU>): 100 type pairs x 3 mask counts would otherwise triple
// over the "map_u" knob.
#include <hip/hip_runtime.h>

#include <cstring>

#include "ec_compare_kernels.hpp"
#include "ec_dispatch.hpp"
#include "ec_lattice.hpp"
#include "ec_map_launch.hpp"
#include "ec_runtime.hpp"

namespace ecd {

// the operands of a compare after the checks: up to two masks, in the order given
struct CompareMasks {
    const uint8_t* m[2] = {nullptr, nullptr};
    int n = 0;
    CompareMasks(const uint8_t* a, const uint8_t* b) {
        if (a) m[n++] = a;
        if (b) m[n++] = b;
    }
};

template <typename L, typename R, int NMASK>
static ec_status launch_compare_n(uint32_t rel, const void* l, const void* r, const CompareMasks& ms, size_t n, uint8_t* out, hipStream_t s) {
    CompareFn<L, R, NMASK> fn{static_cast<const L*>(l), static_cast<const R*>(r), ms.m[0], ms.m[1], out, rel};
    constexpr size_t cpl = CompareFn<L, R, NMASK>::CPL;
    const bool al = aligned16(l, r, l) && aligned_to(out, cpl) && (NMASK < 1 || aligned_to(ms.m[0], cpl)) && (NMASK < 2 || aligned_to(ms.m[1], cpl));
    return launch_map<kDefaultU>(fn, n, al, s, "compare");
}

template <typename L, typename R>
static ec_status launch_compare(uint32_t rel, const void* l, const void* r, const CompareMasks& ms, size_t n, uint8_t* out, hipStream_t s) {
    switch (ms.n) {
        case 0: return launch_compare_n<L, R, 0>(rel, l, r, ms, n, out, s);
        case 1: return launch_compare_n<L, R, 1>(rel, l, r, ms, n, out, s);
        default: return launch_compare_n<L, R, 2>(rel, l, r, ms, n, out, s);
    }
}

static ec_status dispatch_compare(uint32_t rel, int lt, const void* l, int rt, const void* r, const CompareMasks& ms, size_t n, uint8_t* out,
                                  hipStream_t s) {
    return ecl::with_cell_types(lt, rt, [&](auto lc, auto rc) { return launch_compare<ecl::cell_t<decltype(lc)>, ecl::cell_t<decltype(rc)>>(rel, l, r, ms, n, out, s); },
                                [] { return set_error(EC_ERR_UNSUPPORTED_TYPE, "compare: bad dtype"); });
}

template <typename L, typename UT>
static ec_status launch_compare_scalar(uint32_t rel, const void* l, const uint8_t* mask, size_t n, const ec_value* rhs_u, uint8_t* out, hipStream_t s) {
    if constexpr (ecl::can_fit_into(ecl::dtype_of<L>::value, ecl::dtype_of<UT>::value)) {
        const UT v = ecl::value_as<UT>(*rhs_u);
        constexpr size_t cpl = 16 / sizeof(L);
        const bool al = aligned16(l, l, l) && aligned_to(out, cpl) && (!mask || aligned_to(mask, cpl));
        if (mask) {
            CompareScalarFn<L, UT, 1> fn{static_cast<const L*>(l), mask, out, v, rel};
            return launch_map<kDefaultU>(fn, n, al, s, "compare_scalar");
        }
        CompareScalarFn<L, UT, 0> fn{static_cast<const L*>(l), nullptr, out, v, rel};
        return launch_map<kDefaultU>(fn, n, al, s, "compare_scalar");
    } else {
        (void)rel; (void)l; (void)mask; (void)n; (void)rhs_u; (void)out; (void)s;
        return set_error(EC_ERR_ARG, "compare_scalar: pair not instantiated");  // unreachable: ut is a union with lt
    }
}

static ec_status dispatch_compare_scalar(uint32_t rel, int lt, const void* l, const uint8_t* mask, size_t n, int ut, const ec_value* rhs_u,
                                         uint8_t* out, hipStream_t s) {
    return ecl::with_cell_types(lt, ut, [&](auto lc, auto uc) { return launch_compare_scalar<ecl::cell_t<decltype(lc)>, ecl::cell_t<decltype(uc)>>(rel, l, mask, n, rhs_u, out, s); },
                                [] { return set_error(EC_ERR_UNSUPPORTED_TYPE, "compare_scalar: bad dtype"); });
}

template <typename W, bool MASKED>
static ec_status launch_select(const void* a, const uint8_t* am, const void* b, const uint8_t* bm, const uint8_t* sel, size_t n, void* out,
                               uint8_t* om, hipStream_t s) {
    SelectFn<W, MASKED> fn{static_cast<const W*>(a), static_cast<const W*>(b), sel, am, bm, static_cast<W*>(out), om};
    constexpr size_t cpl = 16 / sizeof(W);
    const bool al = aligned16(a, b, out) && aligned_to(sel, cpl) &&
                    (!MASKED || (aligned_to(am, cpl) && aligned_to(bm, cpl) && aligned_to(om, cpl)));
    return launch_map<kDefaultU>(fn, n, al, s, MASKED ? "masked_select" : "select");
}

template <bool MASKED>
static ec_status dispatch_select(int t, const void* a, const uint8_t* am, const void* b, const uint8_t* bm, const uint8_t* sel, size_t n, void* out,
                                 uint8_t* om, hipStream_t s) {
    return ecl::with_cell_width(ecl::size_of(t), [&](auto w) { return launch_select<ecl::cell_t<decltype(w)>, MASKED>(a, am, b, bm, sel, n, out, om, s); }, kTypeChecked);
}

}  // namespace ecd

using namespace ecd;

extern "C" ec_status ec_compare(int32_t rel, ec_dtype lt, const void* l, const uint8_t* lmask_or_null, ec_dtype rt, const void* r,
                                const uint8_t* rmask_or_null, size_t n, uint8_t* out_mask, ec_stream stream) {
    if (!valid_relation(rel)) return set_error(EC_ERR_ARG, "ec_compare: relation %d is not an ec_cmp (1..6)", int(rel));
    if (!ecl::valid(lt) || !ecl::valid(rt)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_compare: bad dtype %d / %d", int(lt), int(rt));
    if (n == 0) return EC_OK;
    if (!l || !r || !out_mask) return set_error(EC_ERR_ARG, "ec_compare: null pointer");
    const ec_status st = ensure_ready();
    if (st != EC_OK) return st;
    return dispatch_compare(static_cast<uint32_t>(rel), lt, l, rt, r, CompareMasks(lmask_or_null, rmask_or_null), n, out_mask, S(stream));
}

extern "C" ec_status ec_compare_scalar(int32_t rel, ec_dtype lt, const void* l, const uint8_t* lmask_or_null, size_t n, const ec_value* rhs,
                                       uint8_t* out_mask, ec_stream stream) {
    if (!valid_relation(rel)) return set_error(EC_ERR_ARG, "ec_compare_scalar: relation %d is not an ec_cmp (1..6)", int(rel));
    if (!rhs) return set_error(EC_ERR_ARG, "ec_compare_scalar: null scalar");
    if (!ecl::valid(lt) || !ecl::valid(rhs->dtype))
        return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_compare_scalar: bad dtype %d / %d", int(lt), int(rhs->dtype));
    if (n == 0) return EC_OK;
    if (!l || !out_mask) return set_error(EC_ERR_ARG, "ec_compare_scalar: null pointer");
    const int ut = ecl::union_of(lt, rhs->dtype);
    ec_value rhs_u;
    ec_status st = ec_value_convert(rhs, static_cast<ec_dtype>(ut), &rhs_u);  // a widening: never refused
    if (st != EC_OK) return st;
    st = ensure_ready();
    if (st != EC_OK) return st;
    return dispatch_compare_scalar(static_cast<uint32_t>(rel), lt, l, lmask_or_null, n, ut, &rhs_u, out_mask, S(stream));
}

extern "C" ec_status ec_select(ec_dtype t, const void* a, const void* b, const uint8_t* sel, size_t n, void* out, ec_stream stream) {
    if (!ecl::valid(t)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_select: bad dtype %d", int(t));
    if (n == 0) return EC_OK;
    if (!a || !b || !sel || !out) return set_error(EC_ERR_ARG, "ec_select: null pointer");
    const ec_status st = ensure_ready();
    if (st != EC_OK) return st;
    return dispatch_select<false>(t, a, nullptr, b, nullptr, sel, n, out, nullptr, S(stream));
}

extern "C" ec_status ec_masked_select(ec_dtype t, const void* a, const uint8_t* amask, const void* b, const uint8_t* bmask, const uint8_t* sel,
                                      size_t n, void* out, uint8_t* out_mask, ec_stream stream) {
    if (!ecl::valid(t)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_masked_select: bad dtype %d", int(t));
    if (n == 0) return EC_OK;
    if (!a || !b || !amask || !bmask || !sel || !out || !out_mask) return set_error(EC_ERR_ARG, "ec_masked_select: null pointer");
    const ec_status st = ensure_ready();
    if (st != EC_OK) return st;
    return dispatch_select<true>(t, a, amask, b, bmask, sel, n, out, out_mask, S(stream));
}
