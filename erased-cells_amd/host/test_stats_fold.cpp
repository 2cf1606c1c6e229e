// The host fold of the band statistics (csrc/ec_stats_fold.hpp) on its own: no HIP, nothing of the library linked.  Hand-made
// ec_moments records with known answers — exact integer records up to the accepted cell counts (sq_hi in use, a negative sum),
// empty records alone and between others, the pivoted f64 kind with a raw M2 below zero and with NaN, the Chan merge against
// the one-record answer, the refusals.  Built plain and under the address and undefined-behaviour sanitizers (host/Makefile).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ec_stats_fold.hpp"

using namespace ecd;

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

static ec_moments int_record(int dtype, uint64_t count, __int128 sum, unsigned __int128 sq, int64_t nkmin, int64_t kmax) {
    ec_moments r;
    std::memset(&r, 0, sizeof r);
    r.count = count;
    r.keys2[0] = nkmin;
    r.keys2[1] = kmax;
    r.kind = 0;
    r.dtype = dtype;
    r.u.i.sum = static_cast<int64_t>(sum);
    r.u.i.sq_lo = static_cast<uint64_t>(sq);
    r.u.i.sq_hi = static_cast<uint64_t>(sq >> 64);
    return r;
}
static ec_moments f64_record(int dtype, uint64_t count, double pivot, double s1, double s2) {
    ec_moments r;
    std::memset(&r, 0, sizeof r);
    r.count = count;
    r.keys2[0] = r.keys2[1] = 0;
    r.kind = 1;
    r.dtype = dtype;
    r.u.f.pivot = pivot;
    r.u.f.s1 = s1;
    r.u.f.s2 = s2;
    return r;
}
// the record of `cells` (small integers), min / max keys as the plain values
static ec_moments record_of(int dtype, const std::vector<int64_t>& cells, int64_t sentinel_hi, int64_t sentinel_lo) {
    __int128 s = 0;
    unsigned __int128 q = 0;
    int64_t mn = sentinel_hi, mx = sentinel_lo;
    for (int64_t x : cells) {
        s += x;
        q += static_cast<unsigned __int128>(static_cast<__int128>(x) * x);
        if (x < mn) mn = x;
        if (x > mx) mx = x;
    }
    return int_record(dtype, cells.size(), s, q, ~mn, mx);
}
static uint64_t bits(double d) { uint64_t b; std::memcpy(&b, &d, sizeof b); return b; }

int main() {
    ec_stats out;
    int64_t keys[2];

    {  // 1, 2, 3, 4: mean 2.5, M2 = (4 * 30 - 100) / 4 = 5, population variance 1.25
        const ec_moments r = record_of(EC_U8, {1, 2, 3, 4}, 255, 0);
        CHECK(stats_fold_refusal(&r, 1, &out) == nullptr);
        stats_fold_records(&r, 1, &out, keys);
        CHECK(out.count == 4 && out.sum == 10.0 && out.mean == 2.5 && out.stddev == std::sqrt(1.25));
        CHECK(keys[0] == ~int64_t(1) && keys[1] == 4);
    }
    {  // 2^31 cells of u32::MAX: the sum of squares needs sq_hi, count * S2 - S1^2 is exactly 0 below 2^128
        const uint64_t n = uint64_t(1) << 31, x = 0xFFFFFFFFull;
        const ec_moments r = int_record(EC_U32, n, static_cast<__int128>(n) * x, static_cast<unsigned __int128>(n) * x * x, ~int64_t(x), int64_t(x));
        CHECK(r.u.i.sq_hi != 0);
        stats_fold_records(&r, 1, &out, keys);
        CHECK(out.count == n && out.mean == 4294967295.0 && out.stddev == 0.0 && out.sum == 9223372034707292160.0);
    }
    {  // 2^31 cells of i32::MIN: the most negative sum, -2^62
        const uint64_t n = uint64_t(1) << 31;
        const __int128 x = -(__int128(1) << 31);
        const ec_moments r = int_record(EC_I32, n, x * n, static_cast<unsigned __int128>(x * x) * n, ~int64_t(x), int64_t(x));
        stats_fold_records(&r, 1, &out, keys);
        CHECK(out.mean == -2147483648.0 && out.stddev == 0.0 && out.sum == -4611686018427387904.0);
    }
    {  // half u32::MAX, half 0 over 2^31 cells: variance (MAX / 2)^2, numerator 2^60 * MAX^2 — beyond 2^123
        const uint64_t n = uint64_t(1) << 31, h = n / 2, x = 0xFFFFFFFFull;
        const ec_moments r = int_record(EC_U32, n, static_cast<__int128>(h) * x, static_cast<unsigned __int128>(h) * x * x, ~int64_t(0), int64_t(x));
        stats_fold_records(&r, 1, &out, keys);
        CHECK(out.mean == 2147483647.5 && out.stddev == 2147483647.5);
    }
    {  // empty records: alone, and between others
        const ec_moments e = record_of(EC_I16, {}, 32767, -32768);
        stats_fold_records(&e, 1, &out, keys);
        CHECK(out.count == 0 && out.sum == 0.0 && std::isnan(out.mean) && std::isnan(out.stddev));
        CHECK(keys[0] == ~int64_t(32767) && keys[1] == -32768);
        const ec_moments three[3] = {e, record_of(EC_I16, {-5, 7}, 32767, -32768), e};
        stats_fold_records(three, 3, &out, keys);
        CHECK(out.count == 2 && out.mean == 1.0 && out.stddev == 6.0 && out.sum == 2.0 && keys[0] == ~int64_t(-5) && keys[1] == 7);
    }
    {  // the merge against the one-record answer on integers small enough for every step to be exact
        const std::vector<int64_t> a = {2, 4, 4, 4}, b = {5, 5, 7, 9}, all = {2, 4, 4, 4, 5, 5, 7, 9};
        const ec_moments two[2] = {record_of(EC_U16, a, 65535, 0), record_of(EC_U16, b, 65535, 0)};
        const ec_moments one = record_of(EC_U16, all, 65535, 0);
        ec_stats whole;
        stats_fold_records(&one, 1, &whole, keys);
        stats_fold_records(two, 2, &out, keys);
        CHECK(whole.mean == 5.0 && whole.stddev == 2.0);
        CHECK(out.count == 8 && out.mean == whole.mean && out.stddev == whole.stddev && out.sum == whole.sum && keys[0] == ~int64_t(2) && keys[1] == 9);
    }
    {  // integer records are added exactly before anything is merged: the cut, and its order, do not show
        const std::vector<int64_t> a = {21821, 41110, 30000}, b = {2827, 54382}, c = {19097, 34578, 1, 65535}, all = {21821, 41110, 30000, 2827, 54382, 19097, 34578, 1, 65535};
        const ec_moments abc[3] = {record_of(EC_U16, a, 65535, 0), record_of(EC_U16, b, 65535, 0), record_of(EC_U16, c, 65535, 0)};
        const ec_moments cba[3] = {abc[2], abc[1], abc[0]};
        const ec_moments one = record_of(EC_U16, all, 65535, 0);
        ec_stats whole, rev;
        stats_fold_records(&one, 1, &whole, keys);
        stats_fold_records(abc, 3, &out, keys);
        stats_fold_records(cba, 3, &rev, keys);
        CHECK(bits(out.mean) == bits(whole.mean) && bits(out.stddev) == bits(whole.stddev) && out.sum == whole.sum && out.count == 9);
        CHECK(bits(rev.mean) == bits(whole.mean) && bits(rev.stddev) == bits(whole.stddev));
        // past what one u32 record may cover the run closes: 2^31 cells of 1000, then 8 more cells, merged as two
        const ec_moments big[3] = {int_record(EC_U32, uint64_t(1) << 31, (__int128(1) << 31) * 1000, (static_cast<unsigned __int128>(1) << 31) * 1000000, ~int64_t(1000), 1000),
                                   record_of(EC_U32, {7, 9, 11, 9, 9}, 0xFFFFFFFFll, 0), record_of(EC_U32, {1, 2, 3}, 0xFFFFFFFFll, 0)};
        stats_fold_records(big, 3, &out, keys);
        CHECK(out.count == (uint64_t(1) << 31) + 8 && out.sum == 2147483648000.0 + 51.0 && out.mean < 1000.0 && out.mean > 999.99999 && keys[0] == ~int64_t(1) && keys[1] == 1000);
    }
    {  // kind 1: mean = pivot + s1 / n; a raw M2 below zero is rounding of a constant band and becomes 0; NaN stays NaN
        ec_moments r = f64_record(EC_F64, 4, 1e9, 10.0, 30.0);
        stats_fold_records(&r, 1, &out, keys);
        CHECK(out.mean == 1e9 + 2.5 && out.stddev == std::sqrt(1.25) && out.sum == 4e9 + 10.0);
        r = f64_record(EC_F32, 3, 0.0, 0.3, 0.03 - 1e-17);  // s2 - s1 * (s1 / 3) < 0
        CHECK(r.u.f.s2 - r.u.f.s1 * (r.u.f.s1 / 3.0) < 0.0);
        stats_fold_records(&r, 1, &out, keys);
        CHECK(out.stddev == 0.0 && bits(out.stddev) == 0);
        r = f64_record(EC_F64, 2, 0.0, NAN, NAN);
        stats_fold_records(&r, 1, &out, keys);
        CHECK(out.count == 2 && std::isnan(out.mean) && std::isnan(out.stddev) && std::isnan(out.sum));
    }
    {  // refusals
        ec_moments r[2] = {record_of(EC_U8, {1}, 255, 0), record_of(EC_U8, {2}, 255, 0)};
        CHECK(stats_fold_refusal(nullptr, 1, &out) != nullptr && stats_fold_refusal(r, 1, nullptr) != nullptr);
        CHECK(stats_fold_refusal(r, 0, &out) != nullptr && stats_fold_refusal(r, -3, &out) != nullptr);
        CHECK(stats_fold_refusal(r, 2, &out) == nullptr);
        r[1].dtype = EC_I8;
        CHECK(stats_fold_refusal(r, 2, &out) != nullptr);  // mixed dtypes
        r[1].dtype = EC_U8;
        r[1].kind = 1;
        CHECK(stats_fold_refusal(r, 2, &out) != nullptr);  // kind 1 is not u8's
        r[0].dtype = r[1].dtype = 10;
        r[1].kind = 0;
        CHECK(stats_fold_refusal(r, 2, &out) != nullptr);  // no such cell type
        r[0] = record_of(EC_U32, {1}, 0xFFFFFFFFll, 0);
        r[0].count = (uint64_t(1) << 31) + 1;  // beyond what an exact u32 record may cover: its sums could leave their words
        CHECK(stats_fold_refusal(r, 1, &out) != nullptr);
        r[0].count = uint64_t(1) << 31;
        CHECK(stats_fold_refusal(r, 1, &out) == nullptr);
        CHECK(stats_kind(EC_U64) == 1 && stats_kind(EC_I32) == 0 && stats_kind(EC_F32) == 1 && stats_kind(-1) == -1);
        CHECK(stats_max_cells(EC_U8) == (uint64_t(1) << 32) && stats_max_cells(EC_I32) == (uint64_t(1) << 31) && stats_max_cells(EC_F64) == 0);
    }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
