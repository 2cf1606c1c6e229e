// ec_stats.hip — band statistics (include/erased_cells.h: ec_stats_device, ec_stats_fold, ec_stats_compute): the stats
// kernels (ec_stats_kernels.hpp) described to the reductions' launcher and hand-over (ec_reduce_launch.hpp), and the host fold
// (ec_stats_fold.hpp) behind the C ABI.  The sharded form is ec_sharded.hip's.
#include <hip/hip_runtime.h>

#include <cstring>

#include "ec_dispatch.hpp"
#include "ec_lattice.hpp"
#include "ec_reduce_launch.hpp"
#include "ec_runtime.hpp"
#include "ec_stats_fold.hpp"
#include "ec_stats_kernels.hpp"

namespace ecd {

static_assert(sizeof(Moments) <= sizeof(int64_t) * kStatsRecordWords && sizeof(ec_moments) == sizeof(int64_t) * kStatsRecordWords,
              "the stream's scratch is sized in 64-byte records");

// The stats kernels as launch_reduction (ec_reduce_launch.hpp) sees them: a Moments per workgroup in the scratch's stats
// area, the record as the result.  One shape, the reductions' default: "reduce_shape" is min/max's A/B knob.
template <typename T>
struct StatsReduction {
    using Cell = T;
    using Partial = Moments;
    using Out = ec_moments;
    static constexpr ScratchSlot kPartials = kScratchStatsPartials;
    static constexpr const char *kSingle = "stats(single workgroup)", *kPartialsName = "stats(partials)", *kFinalizeName = "stats(finalize)";
    template <bool MASKED, int U, int BLOCK> static auto vector_kernel() { return k_stats_partials<T, MASKED, U, BLOCK>; }
    template <bool MASKED> static auto cellwise_kernel() { return k_stats_partials_cellwise<T, MASKED>; }
    static void finalize(const Moments* partials, int nparts, const T* first_cell_or_null, ec_moments* rec_dev, hipStream_t s) {
        k_stats_finalize<T><<<1, kStatsFinalizeBlock, 0, s>>>(partials, nparts, first_cell_or_null, rec_dev);
    }
};

static ec_status dispatch_stats(int t, const void* p, const uint8_t* mask, size_t n, ec_moments* rec_dev, hipStream_t s) {
    return ecl::with_cell_type(t, [&](auto c) { return launch_reduction<StatsReduction<ecl::cell_t<decltype(c)>>, kReduceU, kRBlock, 4>(p, mask, n, rec_dev, s); },
                               [] { return set_error(EC_ERR_UNSUPPORTED_TYPE, "stats: bad dtype"); });
}

ec_status check_stats_cells(const char* who, int shard, int t, size_t n, const char* advice) {
    const uint64_t limit = stats_max_cells(t);
    if (!limit || n <= limit) return EC_OK;
    const unsigned long long most = limit;
    if (shard < 0) return set_error(EC_ERR_ARG, "%s: %zu cells of dtype %d, more than the %llu one exact record covers: %s", who, n, t, most, advice);
    return set_error(EC_ERR_ARG, "%s: shard %d has %zu cells, more than the %llu one exact record covers: %s", who, shard, n, most, advice);
}

// What ec_stats_device refuses before any device work.
static ec_status check_stats_args(const char* who, ec_dtype t, const void* p, size_t n, const void* out) {
    if (!out || (n > 0 && !p)) return set_error(EC_ERR_ARG, "%s: null pointer", who);
    if (!ecl::valid(t)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "%s: bad dtype %d", who, int(t));
    return check_stats_cells(who, -1, t, n, "shard it (ec_stats_fold merges the records)");
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
    ec_moments rec;
    st = sync_result(s, kResultStatsRecord, &rec, sizeof rec, [&](const Scratch&, int64_t* slot) {
        return dispatch_stats(t, p, mask_or_null, n, reinterpret_cast<ec_moments*>(slot), s);
    });
    if (st != EC_OK) return st;
    return ec_stats_fold(&rec, 1, stats_out);
}
