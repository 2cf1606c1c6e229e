// ec_stats.hip — band statistics (include/erased_cells.h: ec_stats_device, ec_stats_fold, ec_stats_compute): the launcher of
// the stats kernels (ec_stats_kernels.hpp) over the reductions' launch plan, and the host fold (ec_stats_fold.hpp) behind the
// C ABI.  The sharded form is ec_sharded.hip's.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>

#include "ec_lattice.hpp"
#include "ec_runtime.hpp"
#include "ec_stats_fold.hpp"
#include "ec_stats_kernels.hpp"

namespace ecd {

static_assert(sizeof(Moments) <= sizeof(int64_t) * kStatsRecordWords && sizeof(ec_moments) == sizeof(int64_t) * kStatsRecordWords,
              "the stream's scratch is sized in 64-byte records");

// min/max's launch (ec_abi.hip launch_min_max) with the default shape: partials to the stream's scratch and one finalize
// workgroup, or — one workgroup, vector kernel — the record written by that workgroup itself.
template <typename T>
static ec_status launch_stats(const void* p, const uint8_t* mask, size_t n, ec_moments* rec_dev, hipStream_t s) {
    Scratch sc;
    ec_status st = get_scratch(s, &sc);
    if (st != EC_OK) return st;
    const T* tp = static_cast<const T*>(p);
    Moments* partials = reinterpret_cast<Moments*>(sc.dev_stats());
    unsigned grid = 0;
    if (n > 0) {
        constexpr int U = kReduceU, BLOCK = kRBlock;
        // as many workgroups per CU as are resident at once, so that the grid runs as one round (probed once per type)
        static const int resident[2] = {resident_per_cu(k_stats_partials<T, false, U, BLOCK>, BLOCK, 4),
                                        resident_per_cu(k_stats_partials<T, true, U, BLOCK>, BLOCK, 4)};
        const size_t stream_bytes[2] = {n * sizeof(T), mask ? n : 0};
        const ReduceShape shape = {BLOCK, U, resident[mask ? 1 : 0], kBlock, 8};
        const ReducePlan pl = plan_reduction(p, mask ? residue(mask, 16 / sizeof(T)) : 0u, sizeof(T), n, shape, stream_bytes, 2);
        grid = pl.grid;
        ec_moments* direct = pl.aligned && pl.single ? rec_dev : nullptr;
        if (!pl.aligned) {
            if (mask) k_stats_partials_cellwise<T, true><<<grid, kBlock, 0, s>>>(tp, mask, n, partials);
            else k_stats_partials_cellwise<T, false><<<grid, kBlock, 0, s>>>(tp, nullptr, n, partials);
        } else if (mask) {
            k_stats_partials<T, true, U, BLOCK><<<grid, BLOCK, 0, s>>>(tp, mask, n, partials, pl.head_policy, direct);
        } else {
            k_stats_partials<T, false, U, BLOCK><<<grid, BLOCK, 0, s>>>(tp, nullptr, n, partials, pl.head_policy, direct);
        }
        if (direct) return check_launch("stats(single workgroup)");
        st = check_launch("stats(partials)");
        if (st != EC_OK) return st;
    }
    k_stats_finalize<T><<<1, kStatsFinalizeBlock, 0, s>>>(partials, static_cast<int>(grid), n > 0 ? tp : nullptr, rec_dev);
    return check_launch("stats(finalize)");
}

static ec_status dispatch_stats(int t, const void* p, const uint8_t* mask, size_t n, ec_moments* rec_dev, hipStream_t s) {
#define EC_ROW(ID, T) case ID: return launch_stats<T>(p, mask, n, rec_dev, s);
    switch (t) { EC_WITH_CT(EC_ROW) }
#undef EC_ROW
    return set_error(EC_ERR_UNSUPPORTED_TYPE, "stats: bad dtype");
}

// What ec_stats_device refuses before any device work.
static ec_status check_stats_args(const char* who, ec_dtype t, const void* p, size_t n, const void* out) {
    if (!out || (n > 0 && !p)) return set_error(EC_ERR_ARG, "%s: null pointer", who);
    if (!ecl::valid(t)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "%s: bad dtype %d", who, int(t));
    const uint64_t limit = stats_max_cells(t);
    if (limit && n > limit)
        return set_error(EC_ERR_ARG, "%s: %zu cells of dtype %d, more than the %llu one exact record covers: shard it (ec_stats_fold merges the records)",
                         who, n, int(t), static_cast<unsigned long long>(limit));
    return EC_OK;
}

}  // namespace ecd

using namespace ecd;

extern "C" ec_status ec_stats_device(ec_dtype t, const void* p, const uint8_t* mask_or_null, size_t n, void* moments_dev,
                                     ec_stream stream) {
    ec_status st = check_stats_args("ec_stats_device", t, p, n, moments_dev);
    if (st != EC_OK) return st;
    if ((st = ensure_ready()) != EC_OK) return st;
    return dispatch_stats(t, p, mask_or_null, n, static_cast<ec_moments*>(moments_dev), static_cast<hipStream_t>(stream));
}

extern "C" ec_status ec_stats_fold(const void* moments_host, int32_t n_recs, void* stats_out) {
    const ec_moments* recs = static_cast<const ec_moments*>(moments_host);
    if (const char* why = stats_fold_refusal(recs, n_recs, stats_out)) return set_error(EC_ERR_ARG, "ec_stats_fold: %s", why);
    ec_stats* out = static_cast<ec_stats*>(stats_out);
    int64_t keys2[2];
    stats_fold_records(recs, n_recs, out, keys2);
    return ec_min_max_decode(static_cast<ec_dtype>(recs[0].dtype), keys2, &out->min, &out->max);
}

extern "C" ec_status ec_stats_compute(ec_dtype t, const void* p, const uint8_t* mask_or_null, size_t n, void* stats_out,
                                      ec_stream stream) {
    ec_status st = check_stats_args("ec_stats_compute", t, p, n, stats_out);
    if (st != EC_OK) return st;
    if ((st = ensure_ready()) != EC_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    if ((st = get_scratch(s, &sc)) != EC_OK) return st;
    ec_moments rec;
    {
        std::lock_guard<std::mutex> turn(*sc.mu);  // the stream's record slot: host threads sharing the stream take turns
        ec_moments* slot = reinterpret_cast<ec_moments*>(sc.dev_stats_record());
        if ((st = dispatch_stats(t, p, mask_or_null, n, slot, s)) != EC_OK) return st;
        if ((st = check_hip(hipMemcpyAsync(&rec, slot, sizeof rec, hipMemcpyDeviceToHost, s), "hipMemcpyAsync(stats record)")) != EC_OK) return st;
        if ((st = check_hip(hipStreamSynchronize(s), "hipStreamSynchronize")) != EC_OK) return st;
    }
    return ec_stats_fold(&rec, 1, stats_out);
}
