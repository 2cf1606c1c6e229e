// ec_reclass.hip — reclassification (include/erased_cells.h: ec_reclass_table_build, ec_reclass): the refusals and the record
// (ec_reclass_checks.hpp; before any device work and before the library asks for a device) and the launches of the kernels of
// ec_reclass_kernels.hpp, in a translation unit of their own so the build stays parallel.  The sharded form is ec_sharded.hip's.
// The family launches at the default tile shape only (ecr::kU = the default "map_u"), as ec_compare and ec_cast do.
#include <hip/hip_runtime.h>

#include "ec_dispatch.hpp"
#include "ec_lattice.hpp"
#include "ec_reclass_checks.hpp"
#include "ec_reclass_kernels.hpp"
#include "ec_runtime.hpp"

namespace ecd {

static_assert(EC_RECLASS_MAX_BREAKS == ecr::kMaxBreaks, "the plan header restates the C ABI's limit");

template <typename T, typename W>
static ec_status launch_reclass(const void* src, const uint8_t* mask, size_t n, const void* table, void* dst, uint8_t* dst_mask, hipStream_t s) {
    constexpr size_t CPL = ecr::cpl(sizeof(T), sizeof(W));
    const T* sp = static_cast<const T*>(src);
    const ec_reclass_table* tab = static_cast<const ec_reclass_table*>(table);
    W* out = static_cast<W*>(dst);
    const bool aligned = aligned_to(src, CPL * sizeof(T)) && aligned_to(dst, CPL * sizeof(W)) && (!mask || aligned_to(mask, CPL)) &&
                         (!dst_mask || aligned_to(dst_mask, CPL));
    const size_t stream_bytes[1] = {n * sizeof(T)};  // the value operand; mask bytes load nt
    auto launch = [&](auto masked) -> ec_status {
        constexpr bool MASKED = decltype(masked)::value;
        if (aligned) {
            const unsigned policy = cache_plan(stream_bytes, 1);
            return split_launch(ecr::tiles(n, CPL), "reclass", [&](size_t first, unsigned groups) {
                k_reclass<T, W, MASKED, ecr::kU><<<groups, kBlock, 0, s>>>(sp, mask, tab, out, dst_mask, n, policy, first);
            });
        }
        k_reclass_cellwise<T, W, MASKED><<<grid_capped((n + kBlock - 1) / kBlock, 8), kBlock, 0, s>>>(sp, mask, tab, out, dst_mask, n);
        return check_launch("reclass");
    };
    return mask ? launch(std::true_type{}) : launch(std::false_type{});
}

}  // namespace ecd

using namespace ecd;

extern "C" ec_status ec_reclass_table_build(ec_dtype t, ec_dtype bt, const void* breaks_host, int32_t n_breaks, int32_t right, ec_dtype dt,
                                            const ec_value* values, const uint8_t* valid_or_null, const ec_value* nodata_or_null,
                                            void* table_host_out) {
    if (const ecv::Refusal r = ecr::build(t, bt, breaks_host, n_breaks, right, dt, values, valid_or_null, nodata_or_null,
                                          static_cast<ec_reclass_table*>(table_host_out)))
        return refused(r, "ec_reclass_table_build", "(dtype %d, breaks of dtype %d, output dtype %d, %d breaks, right %d)", int(t), int(bt), int(dt),
                       int(n_breaks), int(right));
    return EC_OK;
}

extern "C" ec_status ec_reclass(ec_dtype t, const void* src, const uint8_t* mask_or_null, size_t n, ec_dtype dt, const void* table_dev, void* dst,
                                uint8_t* dst_mask_or_null, ec_stream stream) {
    if (const ecv::Refusal r = ecr::reclass_refusal(ecl::size_of(t), ecl::size_of(dt), src, mask_or_null, n, table_dev, dst, dst_mask_or_null))
        return refused(r, "ec_reclass", "(dtype %d, output dtype %d, %zu cells)", int(t), int(dt), n);
    if (n == 0) return EC_OK;
    const ec_status st = ensure_ready();
    if (st != EC_OK) return st;
    return ecl::with_cell_type(t, [&](auto c) {
        return ecl::with_cell_width(ecl::size_of(dt), [&](auto w) {
            return launch_reclass<ecl::cell_t<decltype(c)>, ecl::cell_t<decltype(w)>>(src, mask_or_null, n, table_dev, dst, dst_mask_or_null, S(stream));
        }, kTypeChecked);
    }, kTypeChecked);
}
