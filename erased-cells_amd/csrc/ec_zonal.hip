// ec_zonal.hip — zonal statistics (include/erased_cells.h: ec_zonal_workspace_bytes, ec_zonal_stats_device,
// ec_zonal_stats_compute, ec_zonal_broadcast): the refusals (ec_zonal_plan.hpp; before any device work and before the library
// asks for a device), the launches of the kernels of ec_zonal_kernels.hpp under the reductions' plan (ec_reduce_plan.hpp), and
// the synchronous form over the library's stream-ordered pool.  The sharded form is ec_sharded.hip's, over zonal_records_host.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "ec_dispatch.hpp"
#include "ec_lattice.hpp"
#include "ec_runtime.hpp"
#include "ec_stats_fold.hpp"
#include "ec_zonal_host.hpp"
#include "ec_zonal_kernels.hpp"

namespace ecd {

static_assert(EC_ZONAL_MAX_ZONES == ecz::kMaxZones, "the plan header restates the C ABI's limit");
// The launch sequence of launch_reduction (ec_reduce_launch.hpp) with what differs here: a second stream that every launch
// has (the zone ids, whose alignment the plan's `residue1` covers beside the mask's), the tables' dynamic LDS, the partials in
// the caller's workspace, one finalize workgroup per zone.  ecz::kPerCu workgroups per CU: not probed — the LDS of four
// workgroups fits a CU at any n_zones and the kernels are bounded at 256 threads.
template <typename T, typename ZT>
static ec_status launch_zonal(const void* p, const uint8_t* mask, const void* zones, size_t n, int32_t n_zones, ec_moments* records,
                              void* workspace, hipStream_t s) {
    const T* tp = static_cast<const T*>(p);
    const ZT* zp = static_cast<const ZT*>(zones);
    Moments* partials = static_cast<Moments*>(workspace);
    unsigned grid = 0;
    if (n > 0) {
        constexpr size_t CPL = 16 / sizeof(T);
        const size_t stream_bytes[3] = {n * sizeof(T), mask ? n : 0, n * sizeof(ZT)};
        const ReduceShape shape = {ecz::kBlock, ecz::kU, ecz::kPerCu, ecz::kBlock, 8};
        const unsigned residue1 = (mask ? residue(mask, CPL) : 0u) | residue(zones, CPL * sizeof(ZT));
        const ReducePlan pl = plan_reduction(p, residue1, sizeof(T), n, shape, stream_bytes, 3);
        grid = pl.grid;
        const unsigned lds = ecz::lds_layout(n_zones, StatsKind<T>::value).bytes;
        ec_moments* direct = pl.single ? records : nullptr;  // one workgroup: it writes the records itself
        auto launch = [&](auto masked) {
            constexpr bool MASKED = decltype(masked)::value;
            if (pl.aligned) k_zonal_partials<T, ZT, MASKED, ecz::kU><<<grid, ecz::kBlock, lds, s>>>(tp, mask, zp, n, n_zones, partials, pl.head_policy, direct);
            else k_zonal_partials_cellwise<T, ZT, MASKED><<<grid, ecz::kBlock, lds, s>>>(tp, mask, zp, n, n_zones, partials, direct);
        };
        if (mask) launch(std::true_type{});
        else launch(std::false_type{});
        if (direct) return check_launch("zonal_stats(single workgroup)");
        const ec_status st = check_launch("zonal_stats(partials)");
        if (st != EC_OK) return st;
    }
    k_zonal_finalize<T><<<static_cast<unsigned>(n_zones), kStatsFinalizeBlock, 0, s>>>(partials, static_cast<int>(grid), n > 0 ? tp : nullptr, records);
    return check_launch("zonal_stats(finalize)");
}

static ec_status dispatch_zonal(int t, const void* p, const uint8_t* mask, int zt, const void* zones, size_t n, int32_t n_zones, ec_moments* records,
                                void* workspace, hipStream_t s) {
    return ecl::with_cell_type(t, [&](auto c) {
        return with_zone_type(zt, [&](auto z) { return launch_zonal<ecl::cell_t<decltype(c)>, ecl::cell_t<decltype(z)>>(p, mask, zones, n, n_zones, records, workspace, s); });
    }, kTypeChecked);
}

// What ec_zonal_stats_device refuses before any device work (the order: ec_zonal_plan.hpp stats_refusal).
static ec_status check_zonal_args(const char* who, ec_dtype t, const void* p, const uint8_t* mask, ec_dtype zt, const void* zones, size_t n,
                                  int32_t n_zones, const void* out, size_t out_bytes, const void* workspace, bool caller_workspace) {
    const ecv::Refusal r = ecz::stats_refusal(n_zones, ecl::size_of(t), zt, p, mask, zones, n, stats_max_cells(t), out, out_bytes, workspace, caller_workspace);
    return zonal_refused(who, r, t, zt, n, n_zones);
}

// The n_zones records of one launch at HOST address recs (records_host).  Arguments checked by the caller (check_zonal_args with
// a workspace of its own making).
ec_status zonal_records_host(ec_dtype t, const void* p, const uint8_t* mask, ec_dtype zt, const void* zones, size_t n, int32_t n_zones,
                             ec_moments* recs, ec_stream stream) {
    auto dispatch = [&](ec_moments* recs_dev, void* workspace, hipStream_t s) {
        return dispatch_zonal(t, p, mask, zt, zones, n, n_zones, recs_dev, workspace, s);
    };
    return records_host(ecz::workspace_bytes(n_zones), "hipMemcpyAsync(zonal records)", n_zones, recs, stream, dispatch);
}

// Arguments of the forms that make their own workspace: the device form's refusals without the workspace's.
ec_status check_zonal_host_args(const char* who, ec_dtype t, const void* p, const uint8_t* mask, ec_dtype zt, const void* zones, size_t n,
                                int32_t n_zones, const void* stats_out) {
    return check_zonal_args(who, t, p, mask, zt, zones, n, n_zones, stats_out, 0, nullptr, false);
}

// launch_gather's kernels: the table staged in LDS
struct BroadcastKernels {
    static constexpr const char* what = "zonal_broadcast";
    template <typename W, typename ZT, bool MASKOUT>
    static constexpr auto vector = k_zonal_broadcast<W, ZT, MASKOUT, ecz::kBroadcastU>;
    template <typename W, typename ZT, bool MASKOUT>
    static constexpr auto cellwise = k_zonal_broadcast_cellwise<W, ZT, MASKOUT>;
};

}  // namespace ecd

using namespace ecd;

extern "C" size_t ec_zonal_workspace_bytes(int32_t n_zones) { return ecz::workspace_bytes(n_zones); }

extern "C" ec_status ec_zonal_stats_device(ec_dtype t, const void* p, const uint8_t* mask_or_null, ec_dtype zt, const void* zones, size_t n,
                                           int32_t n_zones, void* moments_dev, void* workspace_dev, ec_stream stream) {
    ec_status st = check_zonal_args("ec_zonal_stats_device", t, p, mask_or_null, zt, zones, n, n_zones, moments_dev,
                                    size_t(n_zones > 0 ? n_zones : 0) * sizeof(ec_moments), workspace_dev, true);
    if (st != EC_OK) return st;
    if ((st = ensure_ready()) != EC_OK) return st;
    return dispatch_zonal(t, p, mask_or_null, zt, zones, n, n_zones, static_cast<ec_moments*>(moments_dev), workspace_dev, S(stream));
}

extern "C" ec_status ec_zonal_stats_compute(ec_dtype t, const void* p, const uint8_t* mask_or_null, ec_dtype zt, const void* zones, size_t n,
                                            int32_t n_zones, void* stats_out, ec_stream stream) {
    ec_status st = check_zonal_host_args("ec_zonal_stats_compute", t, p, mask_or_null, zt, zones, n, n_zones, stats_out);
    if (st != EC_OK) return st;
    return zonal_compute(n_zones, stats_out,
                         [&](ec_moments* recs) { return zonal_records_host(t, p, mask_or_null, zt, zones, n, n_zones, recs, stream); });
}

extern "C" ec_status ec_zonal_broadcast(ec_dtype zt, const void* zones, size_t n, int32_t n_zones, ec_dtype t, const void* table_dev, void* dst,
                                        uint8_t* dst_mask_or_null, ec_stream stream) {
    const ecv::Refusal r = ecz::broadcast_refusal(n_zones, ecl::size_of(t), zt, zones, table_dev, n, dst, dst_mask_or_null);
    return zonal_gather_call<BroadcastKernels>("ec_zonal_broadcast", r, zt, zones, n, n_zones, t, table_dev, dst, dst_mask_or_null, stream);
}
