// ec_stats_fold.hpp — the host side of the band statistics (ec_stats_fold, include/erased_cells.h), in plain C++: nothing from
// HIP or from the rest of this library, so that host/test_stats_fold.cpp can run it alone, sanitizers included.
//
// One ec_moments record is what one launch of the stats kernels (ec_stats_kernels.hpp) leaves behind; this file turns one or
// several of them into {count, min, max, sum, mean, stddev}.  Every floating-point step is one individually rounded f64
// operation in the order the header states: compile with FP contraction off (the pragma below asks for it; the library's
// and the test's command lines pass -ffp-contract=off as well), so a*b+c never becomes an fma and the result is one bit
// pattern on every host.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "erased_cells.h"

#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif

namespace ecd {

static_assert(sizeof(ec_moments) == 64, "one record is one 64-byte line");
static_assert(sizeof(ec_stats) == 64, "ec_stats: u64, two 16-byte values, three doubles");

// 0: exact integer sums, 1: pivoted f64 sums, -1: not a cell type.
inline int stats_kind(int dtype) {
    switch (dtype) {
        case EC_U8: case EC_I8: case EC_U16: case EC_I16: case EC_U32: case EC_I32: return 0;
        case EC_U64: case EC_I64: case EC_F32: case EC_F64: return 1;
    }
    return -1;
}

// Cells one record may cover (0: no limit).  With |x| < 2^b and n cells, n * sum(x^2) < n^2 * 2^(2b) must stay below 2^128 (and
// sum(x)^2 with it): n <= 2^32 for b <= 16 (2^64 * 2^32 = 2^96), n <= 2^31 for b = 32 (2^62 * 2^64 = 2^126).  The sum itself
// is then below 2^31 * 2^32 = 2^63: it fits int64.
inline uint64_t stats_max_cells(int dtype) {
    switch (dtype) {
        case EC_U8: case EC_I8: case EC_U16: case EC_I16: return uint64_t(1) << 32;
        case EC_U32: case EC_I32: return uint64_t(1) << 31;
    }
    return 0;
}

// count, mean, M2 = sum of (x - mean)^2 and sum of the cells folded so far.
struct StatsAcc {
    uint64_t n = 0;
    double mean = 0.0, m2 = 0.0, sum = 0.0;
};

// One record as a StatsAcc (count > 0).
inline StatsAcc stats_of_record(const ec_moments& r) {
    StatsAcc a;
    a.n = r.count;
    const double cnt = static_cast<double>(r.count);
    if (r.kind == 0) {
        // count * S2 - S1 * S1 >= 0 (Cauchy-Schwarz) and below 2^128 under stats_max_cells: exact in unsigned 128-bit arithmetic
        const unsigned __int128 s2 = (static_cast<unsigned __int128>(r.u.i.sq_hi) << 64) | r.u.i.sq_lo;
        const __int128 s1 = r.u.i.sum;
        const unsigned __int128 num = static_cast<unsigned __int128>(r.count) * s2 - static_cast<unsigned __int128>(s1 * s1);
        a.sum = static_cast<double>(r.u.i.sum);
        a.mean = static_cast<double>(r.u.i.sum) / cnt;
        a.m2 = static_cast<double>(num) / cnt;
    } else {
        const double q = r.u.f.s1 / cnt;
        a.mean = r.u.f.pivot + q;
        const double prod = r.u.f.s1 * q;
        a.m2 = r.u.f.s2 - prod;
        if (a.m2 < 0.0) a.m2 = 0.0;  // rounding of a near-constant band; NaN compares false and stays
        const double scaled = r.u.f.pivot * cnt;
        a.sum = scaled + r.u.f.s1;
    }
    return a;
}

// Chan, Golub & LeVeque's pairwise update, a then b.
inline void stats_merge(StatsAcc& a, const StatsAcc& b) {
    if (a.n == 0) { a = b; return; }
    const uint64_t n = a.n + b.n;
    const double na = static_cast<double>(a.n), nb = static_cast<double>(b.n), nn = static_cast<double>(n);
    const double delta = b.mean - a.mean;
    const double wb = nb / nn;
    const double step = delta * wb;
    const double dd = delta * delta;
    const double nab = na * nb;
    const double w = nab / nn;
    const double cross = dd * w;
    const double m2 = a.m2 + b.m2;
    a.mean = a.mean + step;
    a.m2 = m2 + cross;
    a.sum = a.sum + b.sum;
    a.n = n;
}

// nullptr, or why the records cannot be folded.
inline const char* stats_fold_refusal(const ec_moments* recs, int32_t n_recs, const void* out) {
    if (!recs || !out) return "null pointer";
    if (n_recs < 1) return "n_recs < 1";
    for (int32_t i = 0; i < n_recs; ++i) {
        if (recs[i].dtype != recs[0].dtype) return "records of different dtype";
        const int kind = stats_kind(recs[i].dtype);
        if (kind < 0) return "bad dtype";
        if (recs[i].kind != kind) return "a record's kind is not its dtype's";
        const uint64_t limit = stats_max_cells(recs[i].dtype);
        if (limit && recs[i].count > limit) return "a record covers more cells than one exact record may (no launch writes such a record)";
    }
    return nullptr;
}

// The fold itself (arguments already checked).  Integer records are first ADDED, exactly, for as long as the cells they cover
// stay within what one record may cover (stats_max_cells): a raster cut into shards then folds to the very figures of the
// raster scanned whole.  A run that would pass the limit is closed — it enters the Chan merge as one record — and the next
// begins; f64 records enter the merge one by one.  Everything but min / max, which need the library's key decoding; `keys2`
// receives the element-wise MAX of the records' {~key(min), key(max)}.
inline void stats_fold_records(const ec_moments* recs, int32_t n_recs, ec_stats* out, int64_t keys2[2]) {
    StatsAcc acc;
    ec_moments run;  // kind 0: the exact sum of the records since the last merge
    memset(&run, 0, sizeof run);
    const uint64_t limit = stats_max_cells(recs[0].dtype);
    keys2[0] = keys2[1] = INT64_MIN;
    for (int32_t i = 0; i < n_recs; ++i) {
        const ec_moments& r = recs[i];
        // keys of an empty record are the sentinels' — the identity of the MAX merge — so they take part either way
        for (int k = 0; k < 2; ++k)
            if (r.keys2[k] > keys2[k]) keys2[k] = r.keys2[k];
        if (r.count == 0) continue;
        if (r.kind != 0) {
            stats_merge(acc, stats_of_record(r));
        } else if (run.count > 0 && r.count <= limit - run.count) {  // both within the limit: the sums stay inside their words
            run.count += r.count;
            run.u.i.sum += r.u.i.sum;
            run.u.i.sq_lo += r.u.i.sq_lo;
            run.u.i.sq_hi += r.u.i.sq_hi + (run.u.i.sq_lo < r.u.i.sq_lo ? 1u : 0u);
        } else {
            if (run.count > 0) stats_merge(acc, stats_of_record(run));
            run = r;
        }
    }
    if (run.count > 0) stats_merge(acc, stats_of_record(run));
    memset(out, 0, sizeof *out);
    out->count = acc.n;
    if (acc.n == 0) {
        out->sum = 0.0;
        out->mean = out->stddev = static_cast<double>(NAN);
        return;
    }
    out->sum = acc.sum;
    out->mean = acc.mean;
    const double var = acc.m2 / static_cast<double>(acc.n);
    out->stddev = sqrt(var);
}

}  // namespace ecd
