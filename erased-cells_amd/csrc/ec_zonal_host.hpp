// ec_zonal_host.hpp — what the host sides of the two zonal families (ec_zonal.hip, ec_zonal_table.hip) share: the dispatch over
// the zone raster's cell type, the refusal's text, the synchronous form over the stream-ordered pool, the fold of the records
// into ec_stats, and the gather (ec_zonal_broadcast, ec_zonal_lookup).  Host code only: what differs between the families comes
// in as a parameter — a workspace size, a dispatch, a pair of kernels, a refusal function — and the kernels are each family's own.
#pragma once

#include <vector>

#include "ec_dispatch.hpp"
#include "ec_runtime.hpp"
#include "ec_stats_fold.hpp"
#include "ec_zonal_plan.hpp"

namespace ecd {

static_assert(EC_U8 == 0 && EC_U16 == 1 && EC_I32 == 6, "ec_zonal_plan.hpp names the zone types by their codes");

// f(cell_tag<ZT>) for the zone type zt (checked before: one of the three)
template <typename F>
static ec_status with_zone_type(int zt, F&& f) {
    switch (zt) {
        case EC_U8: return f(ecl::cell_tag<uint8_t>{});
        case EC_U16: return f(ecl::cell_tag<uint16_t>{});
        case EC_I32: return f(ecl::cell_tag<int32_t>{});
    }
    return kTypeChecked;
}

// EC_OK for no refusal, else the status and text of every zonal entry point's refusal.
inline ec_status zonal_refused(const char* who, const ecv::Refusal& r, ec_dtype t, ec_dtype zt, size_t n, int32_t n_zones) {
    return r ? refused(r, who, "(dtype %d, zones of dtype %d, %zu cells, %d zones)", int(t), int(zt), n, int(n_zones)) : EC_OK;
}

// The n_zones records of one call at HOST address recs: a workspace of `ws` bytes (a multiple of 64) and the records from the
// stream-ordered pool, dispatch(records_dev, workspace, hipStream_t), the download (`copy_what`: its name in an error), the stream
// drained.  Arguments checked by the caller.
template <typename DISPATCH>
static ec_status records_host(size_t ws, const char* copy_what, int32_t n_zones, ec_moments* recs, ec_stream stream, DISPATCH&& dispatch) {
    ec_status st = ensure_ready();
    if (st != EC_OK) return st;
    const size_t out = size_t(n_zones) * sizeof(ec_moments);
    void* block = nullptr;  // the workspace, then the records
    if ((st = ec_alloc_async(&block, ws + out, stream)) != EC_OK) return st;
    ec_moments* recs_dev = reinterpret_cast<ec_moments*>(static_cast<char*>(block) + ws);
    st = dispatch(recs_dev, block, S(stream));
    if (st == EC_OK) st = check_hip(hipMemcpyAsync(recs, recs_dev, out, hipMemcpyDeviceToHost, S(stream)), copy_what);
    const ec_status freed = ec_free_async(block, stream);
    const ec_status synced = check_hip(hipStreamSynchronize(S(stream)), "hipStreamSynchronize");
    return st != EC_OK ? st : freed != EC_OK ? freed : synced;
}

// The records of `shards` calls over the same nz zones (shard-major) to one ec_stats per zone: zone z's records fold in shard order.
inline ec_status fold_zone_records(const ec_moments* recs, int shards, size_t nz, void* stats_out) {
    std::vector<ec_moments> of_zone(static_cast<size_t>(shards));
    ec_stats* out = static_cast<ec_stats*>(stats_out);
    for (size_t z = 0; z < nz; ++z) {
        for (int i = 0; i < shards; ++i) of_zone[static_cast<size_t>(i)] = recs[static_cast<size_t>(i) * nz + z];
        const ec_status st = ec_stats_fold(of_zone.data(), shards, out + z);
        if (st != EC_OK) return st;
    }
    return EC_OK;
}

// The body of ec_zonal_stats_compute and ec_zonal_table_compute: records(recs) is the family's *_records_host of the call.
template <typename RECORDS>
static ec_status zonal_compute(int32_t n_zones, void* stats_out, RECORDS&& records) {
    std::vector<ec_moments> recs(static_cast<size_t>(n_zones));
    const ec_status st = records(recs.data());
    return st != EC_OK ? st : fold_zone_records(recs.data(), 1, recs.size(), stats_out);
}

// dst[i] = table[zones[i]] by the kernels K::vector<W, ZT, MASKOUT> (one workgroup per tile) and K::cellwise<W, ZT, MASKOUT>,
// under the name K::what.
template <typename K, typename W, typename ZT>
static ec_status launch_gather(const void* zones, const void* table, size_t n, int32_t n_zones, void* dst, uint8_t* dst_mask, hipStream_t s) {
    constexpr size_t CPL = ecz::broadcast_cpl(sizeof(W), sizeof(ZT));
    const ZT* zp = static_cast<const ZT*>(zones);
    const W* tab = static_cast<const W*>(table);
    W* out = static_cast<W*>(dst);
    const bool aligned = aligned_to(zones, CPL * sizeof(ZT)) && aligned_to(dst, CPL * sizeof(W)) && (!dst_mask || aligned_to(dst_mask, CPL));
    auto launch = [&](auto maskout) -> ec_status {
        constexpr bool MASKOUT = decltype(maskout)::value;
        if (aligned)
            return split_launch(ecz::broadcast_tiles(n, CPL), K::what, [&](size_t first, unsigned grid) {
                K::template vector<W, ZT, MASKOUT><<<grid, ecz::kBlock, 0, s>>>(zp, tab, n_zones, out, dst_mask, n, first);
            });
        K::template cellwise<W, ZT, MASKOUT><<<grid_capped((n + ecz::kBlock - 1) / ecz::kBlock, 8), ecz::kBlock, 0, s>>>(zp, tab, n_zones, out, dst_mask, n);
        return check_launch(K::what);
    };
    return dst_mask ? launch(std::true_type{}) : launch(std::false_type{});
}

// The body of ec_zonal_broadcast and ec_zonal_lookup: `r` is the family's refusal of the call, K its kernels.
template <typename K>
static ec_status zonal_gather_call(const char* who, const ecv::Refusal& r, ec_dtype zt, const void* zones, size_t n, int32_t n_zones, ec_dtype t,
                                   const void* table_dev, void* dst, uint8_t* dst_mask, ec_stream stream) {
    ec_status st = zonal_refused(who, r, t, zt, n, n_zones);
    if (st != EC_OK || n == 0) return st;
    if ((st = ensure_ready()) != EC_OK) return st;
    return ecl::with_cell_width(ecl::size_of(t), [&](auto w) {
        return with_zone_type(zt, [&](auto z) {
            return launch_gather<K, ecl::cell_t<decltype(w)>, ecl::cell_t<decltype(z)>>(zones, table_dev, n, n_zones, dst, dst_mask, S(stream));
        });
    }, kTypeChecked);
}

}  // namespace ecd
