// ec_zonal_table.hip — zonal statistics over up to 2^24 zones (include/erased_cells.h: ec_zonal_table_workspace_bytes,
// ec_zonal_table_device, ec_zonal_table_compute, ec_zonal_lookup): the refusals (ec_zonal_table_plan.hpp; before any device work
// and before the library asks for a device), the launches of the kernels of ec_zonal_table_kernels.hpp under the reductions' plan
// (ec_reduce_plan.hpp), and the synchronous form over the library's stream-ordered pool.  The sharded form is ec_sharded.hip's,
// over zonal_table_records_host.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "ec_dispatch.hpp"
#include "ec_lattice.hpp"
#include "ec_runtime.hpp"
#include "ec_stats_fold.hpp"
#include "ec_zonal_host.hpp"
#include "ec_zonal_table_kernels.hpp"

namespace ecd {

static_assert(EC_ZONAL_TABLE_MAX_ZONES == ezt::kMaxZones, "the plan header restates the C ABI's cap");
static_assert(size_t(ezt::kMaxZones) * ezt::words(1) * 8 < (uint64_t(1) << 32) && size_t(ezt::kMaxZones) * sizeof(ec_moments) < (uint64_t(1) << 32),
              "every byte offset into the workspace and the records stays below 2^32");

// init, pass A, pass B for kind 1, finalize: four launches at the most, each the next one's input by stream order alone.
template <typename T, typename ZT>
static ec_status launch_table(const void* p, const uint8_t* mask, const void* zones, size_t n, int32_t n_zones, ec_moments* records, void* workspace,
                              hipStream_t s) {
    constexpr int KIND = StatsKind<T>::value;
    const T* tp = static_cast<const T*>(p);
    const ZT* zp = static_cast<const ZT*>(zones);
    ztword* table = static_cast<ztword*>(workspace);
    const uint32_t total_words = static_cast<uint32_t>(n_zones) * static_cast<uint32_t>(ezt::words(KIND));
    k_ztable_init<T><<<grid_capped((size_t(total_words) + ezt::kBlock - 1) / ezt::kBlock, 8), ezt::kBlock, 0, s>>>(table, total_words);
    ec_status st = check_launch("zonal_table(init)");
    if (st != EC_OK) return st;
    if (n > 0) {
        constexpr size_t CPL = 16 / sizeof(T);
        const size_t stream_bytes[3] = {n * sizeof(T), mask ? n : 0, n * sizeof(ZT)};
        const ReduceShape shape = {ezt::kBlock, ezt::kU, ezt::kPerCu, ezt::kBlock, 8};
        const unsigned residue1 = (mask ? residue(mask, CPL) : 0u) | residue(zones, CPL * sizeof(ZT));
        const ReducePlan pl = plan_reduction(p, residue1, sizeof(T), n, shape, stream_bytes, 3);
        auto pass = [&](auto lane_tag, const char* what) {
            using LANE = typename decltype(lane_tag)::type;
            auto launch = [&](auto masked) {
                constexpr bool MASKED = decltype(masked)::value;
                if (pl.aligned) k_ztable_pass<T, ZT, MASKED, ezt::kU, LANE><<<pl.grid, ezt::kBlock, 0, s>>>(tp, mask, zp, n, n_zones, table, pl.head_policy);
                else k_ztable_pass_cellwise<T, ZT, MASKED, LANE><<<pl.grid, ezt::kBlock, 0, s>>>(tp, mask, zp, n, n_zones, table);
            };
            if (mask) launch(std::true_type{});
            else launch(std::false_type{});
            return check_launch(what);
        };
        if ((st = pass(ecl::cell_tag<ZtLaneA<T>>{}, "zonal_table(pass A)")) != EC_OK) return st;
        if constexpr (KIND == 1)
            if ((st = pass(ecl::cell_tag<ZtLaneB<T>>{}, "zonal_table(pass B)")) != EC_OK) return st;
    }
    k_ztable_finalize<T><<<(static_cast<unsigned>(n_zones) + ezt::kBlock - 1) / ezt::kBlock, ezt::kBlock, 0, s>>>(table, n_zones, n > 0 ? tp : nullptr, records);
    return check_launch("zonal_table(finalize)");
}

static ec_status dispatch_table(int t, const void* p, const uint8_t* mask, int zt, const void* zones, size_t n, int32_t n_zones, ec_moments* records,
                                void* workspace, hipStream_t s) {
    return ecl::with_cell_type(t, [&](auto c) {
        return with_zone_type(zt, [&](auto z) { return launch_table<ecl::cell_t<decltype(c)>, ecl::cell_t<decltype(z)>>(p, mask, zones, n, n_zones, records, workspace, s); });
    }, kTypeChecked);
}

static uint64_t table_max_cells(ec_dtype t) { return stats_kind(t) == 0 ? stats_max_cells(t) : ezt::kMaxCellsKind1; }

// What ec_zonal_table_device refuses before any device work (the order: ec_zonal_table_plan.hpp table_refusal).
static ec_status check_table_args(const char* who, ec_dtype t, const void* p, const uint8_t* mask, ec_dtype zt, const void* zones, size_t n, int32_t n_zones,
                                  const void* out, const void* workspace, bool caller_workspace) {
    const ecv::Refusal r = ezt::table_refusal(n_zones, ecl::size_of(t), stats_kind(t), zt, p, mask, zones, n, table_max_cells(t), out, workspace, caller_workspace);
    return zonal_refused(who, r, t, zt, n, n_zones);
}

// The n_zones records of one call at HOST address recs (records_host).  Arguments checked by the caller.
ec_status zonal_table_records_host(ec_dtype t, const void* p, const uint8_t* mask, ec_dtype zt, const void* zones, size_t n, int32_t n_zones,
                                   ec_moments* recs, ec_stream stream) {
    auto dispatch = [&](ec_moments* recs_dev, void* workspace, hipStream_t s) {
        return dispatch_table(t, p, mask, zt, zones, n, n_zones, recs_dev, workspace, s);
    };
    const size_t ws = (ezt::workspace_bytes(stats_kind(t), n_zones) + 63u) & ~size_t(63);
    return records_host(ws, "hipMemcpyAsync(zonal table records)", n_zones, recs, stream, dispatch);
}

ec_status check_zonal_table_host_args(const char* who, ec_dtype t, const void* p, const uint8_t* mask, ec_dtype zt, const void* zones, size_t n,
                                      int32_t n_zones, const void* stats_out) {
    return check_table_args(who, t, p, mask, zt, zones, n, n_zones, stats_out, nullptr, false);
}

// launch_gather's kernels: the table read where it lies
struct LookupKernels {
    static constexpr const char* what = "zonal_lookup";
    template <typename W, typename ZT, bool MASKOUT>
    static constexpr auto vector = k_zonal_lookup<W, ZT, MASKOUT, ecz::kBroadcastU>;
    template <typename W, typename ZT, bool MASKOUT>
    static constexpr auto cellwise = k_zonal_lookup_cellwise<W, ZT, MASKOUT>;
};

}  // namespace ecd

using namespace ecd;

extern "C" size_t ec_zonal_table_workspace_bytes(ec_dtype t, int32_t n_zones) {
    return ezt::workspace_bytes(stats_kind(t), n_zones);
}

extern "C" ec_status ec_zonal_table_device(ec_dtype t, const void* p, const uint8_t* mask_or_null, ec_dtype zt, const void* zones, size_t n,
                                           int32_t n_zones, void* moments_dev, void* workspace_dev, ec_stream stream) {
    ec_status st = check_table_args("ec_zonal_table_device", t, p, mask_or_null, zt, zones, n, n_zones, moments_dev, workspace_dev, true);
    if (st != EC_OK) return st;
    if ((st = ensure_ready()) != EC_OK) return st;
    return dispatch_table(t, p, mask_or_null, zt, zones, n, n_zones, static_cast<ec_moments*>(moments_dev), workspace_dev, S(stream));
}

extern "C" ec_status ec_zonal_table_compute(ec_dtype t, const void* p, const uint8_t* mask_or_null, ec_dtype zt, const void* zones, size_t n,
                                            int32_t n_zones, void* stats_out, ec_stream stream) {
    ec_status st = check_zonal_table_host_args("ec_zonal_table_compute", t, p, mask_or_null, zt, zones, n, n_zones, stats_out);
    if (st != EC_OK) return st;
    return zonal_compute(n_zones, stats_out,
                         [&](ec_moments* recs) { return zonal_table_records_host(t, p, mask_or_null, zt, zones, n, n_zones, recs, stream); });
}

extern "C" ec_status ec_zonal_lookup(ec_dtype zt, const void* zones, size_t n, int32_t n_zones, ec_dtype t, const void* table_dev, void* dst,
                                     uint8_t* dst_mask_or_null, ec_stream stream) {
    const ecv::Refusal r = ezt::lookup_refusal(n_zones, ecl::size_of(t), zt, zones, table_dev, n, dst, dst_mask_or_null);
    return zonal_gather_call<LookupKernels>("ec_zonal_lookup", r, zt, zones, n, n_zones, t, table_dev, dst, dst_mask_or_null, stream);
}
