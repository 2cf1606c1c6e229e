// ec_cast.hip — ec_cast and ec_cast_scaled (include/erased_cells.h): a buffer's cells in a storage cell type, for every one of
// the 100 type pairs, in a translation unit of their own so the build stays parallel.
//
// Every refusal is decided on the host before any device work and before the library asks for a device.  The 41 pairs ec_convert
// accepts go to ec_convert (the existing kernels, the existing copy for st == dt); the 59 others are CastFn, in both modes only
// where the modes differ (an integer destination: 54 pairs).  The family launches at the default tile shape only
// (launch_map<kDefaultU>), as ec_compare does.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "ec_cast_kernels.hpp"
#include "ec_dispatch.hpp"
#include "ec_lattice.hpp"
#include "ec_map_launch.hpp"
#include "ec_runtime.hpp"

namespace ecd {

constexpr bool valid_cast_mode(int mode) { return mode == EC_CAST_AS || mode == EC_CAST_ROUND; }

// every stream of a group at the alignment of its own vector access (all of them, when "unaligned_vector" is on)
template <typename Sx, typename Dx, int CPL>
static bool cast_aligned(const void* src, const uint8_t* mask, const void* dst) {
    return aligned_to(src, CPL * sizeof(Sx)) && aligned_to(dst, CPL * sizeof(Dx)) && (!mask || aligned_to(mask, CPL));
}

template <typename Sx, typename Dx>
static ec_status launch_cast(int mode, const void* src, void* dst, size_t n, hipStream_t s) {
    if constexpr (!ecl::can_fit_into(ecl::dtype_of<Sx>::value, ecl::dtype_of<Dx>::value)) {
        constexpr int cpl = CastFn<Sx, Dx, true>::CPL;
        const bool al = cast_aligned<Sx, Dx, cpl>(src, nullptr, dst);
        if constexpr (!is_fp<Dx>::value) {
            if (mode == EC_CAST_AS) {
                CastFn<Sx, Dx, false> fn{static_cast<const Sx*>(src), static_cast<Dx*>(dst)};
                return launch_map<kDefaultU>(fn, n, al, s, "cast(as)");
            }
        }
        CastFn<Sx, Dx, true> fn{static_cast<const Sx*>(src), static_cast<Dx*>(dst)};  // into f32 the two modes are one kernel
        return launch_map<kDefaultU>(fn, n, al, s, "cast(round)");
    } else {
        (void)mode; (void)src; (void)dst; (void)n; (void)s;
        return set_error(EC_ERR_ARG, "cast: pair not instantiated");  // unreachable: the fitting pairs went to ec_convert
    }
}

static ec_status dispatch_cast(int mode, int st, const void* src, int dt, void* dst, size_t n, hipStream_t s) {
    return ecl::with_cell_types(st, dt, [&](auto sc, auto dc) { return launch_cast<ecl::cell_t<decltype(sc)>, ecl::cell_t<decltype(dc)>>(mode, src, dst, n, s); },
                                [] { return set_error(EC_ERR_UNSUPPORTED_TYPE, "cast: bad dtype"); });
}

template <typename Sx, typename Dx>
static ec_status launch_cast_scaled(const void* src, const uint8_t* mask, size_t n, double scale, double offset, const ec_value* nodata, void* dst,
                                    hipStream_t s) {
    constexpr int cpl = CastScaledFn<Sx, Dx, true>::CPL;
    const bool al = cast_aligned<Sx, Dx, cpl>(src, mask, dst);
    if (mask) {
        CastScaledFn<Sx, Dx, true> fn{static_cast<const Sx*>(src), mask, static_cast<Dx*>(dst), scale, offset, ecl::value_as<Dx>(*nodata)};
        return launch_map<kDefaultU>(fn, n, al, s, "cast_scaled(masked)");
    }
    CastScaledFn<Sx, Dx, false> fn{static_cast<const Sx*>(src), nullptr, static_cast<Dx*>(dst), scale, offset, Dx(0)};
    return launch_map<kDefaultU>(fn, n, al, s, "cast_scaled");
}

static ec_status dispatch_cast_scaled(int st, const void* src, const uint8_t* mask, size_t n, double scale, double offset, int dt,
                                      const ec_value* nodata, void* dst, hipStream_t s) {
    return ecl::with_cell_types(st, dt, [&](auto sc, auto dc) { return launch_cast_scaled<ecl::cell_t<decltype(sc)>, ecl::cell_t<decltype(dc)>>(src, mask, n, scale, offset, nodata, dst, s); },
                                [] { return set_error(EC_ERR_UNSUPPORTED_TYPE, "cast_scaled: bad dtype"); });
}

}  // namespace ecd

using namespace ecd;

extern "C" ec_status ec_cast(int32_t mode, ec_dtype st, const void* src, ec_dtype dt, void* dst, size_t n, ec_stream stream) {
    if (!valid_cast_mode(mode)) return set_error(EC_ERR_ARG, "ec_cast: mode %d is not an ec_cast_mode (0, 1)", int(mode));
    if (!ecl::valid(st) || !ecl::valid(dt)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_cast: bad dtype %d / %d", int(st), int(dt));
    if (n == 0) return EC_OK;
    if (!src || !dst) return set_error(EC_ERR_ARG, "ec_cast: null pointer");
    if (ecl::can_fit_into(st, dt)) return ec_convert(st, src, dt, dst, n, stream);  // exactly ec_convert's cells, by its kernels
    const ec_status rc = ensure_ready();
    if (rc != EC_OK) return rc;
    return dispatch_cast(mode, st, src, dt, dst, n, S(stream));
}

extern "C" ec_status ec_cast_scaled(ec_dtype st, const void* src, const uint8_t* mask_or_null, size_t n, double scale, double offset, ec_dtype dt,
                                    const ec_value* nodata_or_null, void* dst, ec_stream stream) {
    if ((mask_or_null != nullptr) != (nodata_or_null != nullptr))
        return set_error(EC_ERR_ARG, "ec_cast_scaled: a mask and a nodata value are given together or not at all");
    if (!ecl::valid(st) || !ecl::valid(dt)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_cast_scaled: bad dtype %d / %d", int(st), int(dt));
    if (nodata_or_null && nodata_or_null->dtype != dt)
        return set_error(EC_ERR_ARG, "ec_cast_scaled: the nodata value has dtype %d, the destination %d", int(nodata_or_null->dtype), int(dt));
    if (!std::isfinite(scale) || !std::isfinite(offset)) return set_error(EC_ERR_ARG, "ec_cast_scaled: scale and offset must be finite");
    if (n == 0) return EC_OK;
    if (!src || !dst) return set_error(EC_ERR_ARG, "ec_cast_scaled: null pointer");
    const ec_status rc = ensure_ready();
    if (rc != EC_OK) return rc;
    return dispatch_cast_scaled(st, src, mask_or_null, n, scale, offset, dt, nodata_or_null, dst, S(stream));
}
