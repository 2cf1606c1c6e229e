// ec_zonal_table_kernels.hpp — zonal statistics over a per-zone table in GLOBAL memory (gfx950): the device side of
// ec_zonal_table_device and ec_zonal_lookup (include/erased_cells.h).  The LDS family (ec_zonal_kernels.hpp) keeps a workgroup's
// tables on chip and stops at 256 zones; here the table is the caller's workspace (ec_zonal_table_plan.hpp: one entry of 64-bit
// words per zone) and EVERY accumulator is an integer under an agent-scope atomic — add, signed max, unsigned max, or — so no
// order of arrival, launch shape or fold before the atomic can change a bit of the result.
//
// Launches; phases meet only at launch boundaries (no flag, ticket or wait between workgroups, no float atomic):
//   k_ztable_init       the identity of every word (the keys' is not zero)
//   k_ztable_pass_a     count, the two keys, kind 0: sum and squares in two carry-free limbs; kind 1: the unsigned max of |d|'s bits
//                       (magnitude and class in one word) and the OR of the infinity flags
//   k_ztable_pass_b     kind 1 only: the zone's maximum read back, k and k2 derived (cached in the lane while its id stays), t and
//                       the truncated w added into T1 and T2 (ec_zonal_table_cell.hpp)
//   k_ztable_finalize   one lane per zone: the record, with the 128-bit -> f64 conversion, rounded once
// Passes A and B run in the reductions' frame as k_zonal_partials does (ec_zonal_kernels.hpp), ZtLane the visitor: the cell-wise
// pass is zonal_walk_cellwise; the tiled pass KEEPS A TILE LOOP OF ITS OWN in front of the shared zonal_walk_edges.  Under the shared
// zonal_walk, with the group's scan as a member of the lane, its masked pass A kernels for 1-byte values parked SGPRs in VGPR lanes
// and one timed row fell behind the parent (profiles/zonal/frame.md).
//
// Aggregation before the atomic (ZtLane).  A lane keeps ONE running entry for ONE zone and flushes it when its id changes: a zone
// that fills a lane's groups costs that lane one flush a launch.  Before a 16-byte group in which any lane leaves its zone, and at
// the end of the kernel, the wave flushes together: a wave whose lanes hold at most kFewIds zones between them serves them a round
// each (wave_rounds, as the first family does): the zone's lanes fold by shuffles, one lane issues one set of atomics (the giant
// zone, a wave inside a coherent zone, a wave across the edges of a few) — and a wave of many ids flushes lane by lane.
// What an entry holds is the pass's: ZtLaneA, ZtLaneB.
#pragma once

#include "ec_zonal_kernels.hpp"
#include "ec_zonal_table_cell.hpp"
#include "ec_zonal_table_plan.hpp"

namespace ecd {

static_assert(ezt::kBlock == kBlock, "the plan header restates the workgroup of the cell-wise kernels");

using ztword = unsigned long long;

__device__ __forceinline__ void zt_add(ztword* w, uint64_t v) {
    if (v) __hip_atomic_fetch_add(w, static_cast<ztword>(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void zt_smax(ztword* w, int64_t v) {
    __hip_atomic_fetch_max(reinterpret_cast<long long*>(w), static_cast<long long>(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void zt_umax(ztword* w, uint64_t v) {
    if (v) __hip_atomic_fetch_max(w, static_cast<ztword>(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void zt_or(ztword* w, uint64_t v) {
    if (v) __hip_atomic_fetch_or(w, static_cast<ztword>(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t zt_xor_u64(uint64_t v, int off) { return static_cast<uint64_t>(__shfl_xor(static_cast<ztword>(v), off, 64)); }
__device__ __forceinline__ int64_t zt_xor_i64(int64_t v, int off) { return static_cast<int64_t>(__shfl_xor(static_cast<long long>(v), off, 64)); }

template <typename T>
__device__ __forceinline__ int64_t zt_not_min_identity() { return ~order_key<T>(Limits<T>::hi); }
template <typename T>
__device__ __forceinline__ int64_t zt_max_identity() { return order_key<T>(Limits<T>::lo); }

// The whole wave, converged: true iff the lanes that hold something (`has`) hold at most ezt::kFewIds distinct zones between them.
// A round per id (the first lane not yet served, the ballot of the lanes that hold its zone) without folding anything yet.
__device__ __forceinline__ bool zt_few_ids(bool has, int32_t cur) {
    uint64_t rest = __builtin_amdgcn_ballot_w64(has);
#pragma unroll
    for (int r = 0; r < ezt::kFewIds; ++r) {
        if (rest == 0) return true;
        const int32_t zid = __builtin_amdgcn_readlane(cur, __builtin_ctzll(rest));
        rest &= ~__builtin_amdgcn_ballot_w64(has && cur == zid);
    }
    return rest == 0;
}

// Pass A's entry.  Bounds: a lane's share of n <= 2^32 cells; every word is a partial sum of the zone's total, which the plan
// header bounds within its word.
template <typename T>
struct ZtLaneA {
    using cell_type = T;
    static constexpr int KIND = StatsKind<T>::value;
    static constexpr int W = ezt::words(KIND);
    uint64_t cnt;
    int64_t not_min, max;
    uint64_t a, b, c;  // kind 0: sum, squares lo, squares hi; kind 1: max |d| bits, flags, unused

    __device__ __forceinline__ void reset() {
        cnt = 0;
        not_min = zt_not_min_identity<T>();
        max = zt_max_identity<T>();
        a = b = c = 0;
    }
    __device__ __forceinline__ bool has() const { return cnt != 0; }
    __device__ __forceinline__ void enter(const ztword*, int32_t) {}
    __device__ __forceinline__ void add(T x, double pivot) {
        const int64_t key = order_key<T>(x);
        ++cnt;
        not_min = ~key > not_min ? ~key : not_min;
        max = key > max ? key : max;
        if constexpr (KIND == 0) {
            const int64_t w = static_cast<int64_t>(x);
            const uint64_t q = static_cast<uint64_t>(w) * static_cast<uint64_t>(w);  // |x| <= 2^32: x * x < 2^64 + 1, and 2^64 only for -2^32, no cell type's
            a += static_cast<uint64_t>(w);
            b += q & 0xFFFFFFFFull;
            c += q >> 32;
        } else {
            const double d = static_cast<double>(x) - pivot;
            const uint64_t ab = ezt::abs_bits(d);
            a = ab > a ? ab : a;
            b |= ezt::inf_flag(d);
        }
    }
    __device__ __forceinline__ void atomics(ztword* table, int32_t z) const {
        ztword* e = table + size_t(z) * W;
        zt_add(e + ezt::kCount, cnt);
        zt_smax(e + ezt::kNotMin, not_min);
        zt_smax(e + ezt::kMax, max);
        if constexpr (KIND == 0) {
            zt_add(e + ezt::kSum, a);
            zt_add(e + ezt::kSq0, b);
            zt_add(e + ezt::kSq1, c);
        } else {
            zt_umax(e + ezt::kDmax, a);
            zt_or(e + ezt::kFlags, b);
        }
    }
    // the whole wave, converged: every lane's entry folded with the other lanes' by shuffles (same bits in every lane)
    __device__ __forceinline__ void fold() {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            cnt += zt_xor_u64(cnt, off);
            const int64_t om = zt_xor_i64(not_min, off), ox = zt_xor_i64(max, off);
            not_min = om > not_min ? om : not_min;
            max = ox > max ? ox : max;
            const uint64_t oa = zt_xor_u64(a, off), ob = zt_xor_u64(b, off);
            if constexpr (KIND == 0) {
                a += oa;
                b += ob;
                c += zt_xor_u64(c, off);
            } else {
                a = oa > a ? oa : a;
                b |= ob;
            }
        }
    }
};

// Pass B's entry (kind 1): the running T1 and T2 of the lane's zone, whose units are cached while the id stays.
template <typename T>
struct ZtLaneB {
    using cell_type = T;
    static constexpr int W = ezt::words(1);
    bool any;
    ezt::ZoneUnits u{false, false, 0, 0};
    ezt::Limbs t1, t2;

    __device__ __forceinline__ void reset() {
        any = false;
        t1 = ezt::Limbs{0, 0};
        t2 = ezt::Limbs{0, 0};
    }
    __device__ __forceinline__ bool has() const { return any; }
    __device__ __forceinline__ void enter(const ztword* table, int32_t z) {
        u = ezt::zone_units(table[size_t(z) * W + ezt::kDmax]);  // written by pass A, a launch ago; nothing writes it now
    }
    __device__ __forceinline__ void add(T x, double pivot) {
        if (!u.sum1) return;  // a zone of NaN or infinities: the flags decide
        const double d = static_cast<double>(x) - pivot;
        any = true;
        ezt::limbs_add(t1, ezt::trunc_units(d, u.k1));
        if (u.sum2) ezt::limbs_add(t2, ezt::trunc_units(d * d, u.k2));
    }
    __device__ __forceinline__ void atomics(ztword* table, int32_t z) const {
        ztword* e = table + size_t(z) * W;
        zt_add(e + ezt::kT1Lo, t1.lo);
        zt_add(e + ezt::kT1Hi, static_cast<uint64_t>(t1.hi));
        zt_add(e + ezt::kT2Lo, t2.lo);
        zt_add(e + ezt::kT2Hi, static_cast<uint64_t>(t2.hi));
    }
    __device__ __forceinline__ void fold() {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            t1.lo += zt_xor_u64(t1.lo, off);
            t1.hi += zt_xor_i64(t1.hi, off);
            t2.lo += zt_xor_u64(t2.lo, off);
            t2.hi += zt_xor_i64(t2.hi, off);
        }
    }
};

// A lane of a pass, the visitor of zonal_walk_edges and zonal_walk_cellwise: the running entry `e` (ENTRY: ZtLaneA<T> or ZtLaneB<T>) of zone `cur`.
template <typename ENTRY>
struct ZtLane {
    using T = typename ENTRY::cell_type;
    ztword* table;
    double pivot;
    int32_t n_zones;
    int32_t cur;
    ENTRY e;

    __device__ __forceinline__ void init(ztword* t, double pv, int32_t nz) {
        table = t;
        pivot = pv;
        n_zones = nz;
        cur = -1;
        e.reset();
    }
    __device__ __forceinline__ void flush() {
        if (e.has()) e.atomics(table, cur);
        e.reset();
    }
    // one cell; `valid`: it belongs to zone z (in range, shown)
    __device__ __forceinline__ void cell(bool valid, T x, int32_t z) {
        if (!valid) return;
        if (z != cur) {
            flush();
            cur = z;
            e.enter(table, z);
        }
        e.add(x, pivot);
    }
    // the walk's cell: `in`: the lane has one; `m`: its mask byte, 1 without a mask
    __device__ __forceinline__ void cell(bool in, T x, uint8_t m, int32_t z) { cell(in && m != 0 && zone_in_range(z, n_zones), x, z); }
    // the whole wave, converged, before a group: `leaving` — this lane's next cell belongs to another zone than the one it holds.
    // Where any lane leaves, the wave flushes together, so that a wave that crosses a zone's edge as one adds one folded entry.
    __device__ __forceinline__ void before_group(bool leaving) {
        if (__builtin_amdgcn_ballot_w64(leaving && e.has()) != 0) finish();
    }
    // The whole wave, converged: at the end of the kernel, and wherever a lane leaves its zone.  A wave of few zones (one: the giant
    // zone, a wave inside a coherent zone; two to kFewIds: a wave across zones' edges) serves them a round each — the lanes of the
    // zone fold, every other lane SELECTED to the identity, and lane `first` issues the atomics; a wave of many flushes lane by lane.
    __device__ __forceinline__ void finish() {
        const bool has = e.has();
        if (!zt_few_ids(has, cur)) {
            flush();
            return;
        }
        wave_rounds(has, cur, [&](int32_t zid, bool member, int first) {  // wave-uniform: at most kFewIds rounds
            ENTRY f = e;
            if (!member) f.reset();
            f.fold();
            if (static_cast<int>(threadIdx.x & (kWave - 1)) == first) f.atomics(table, zid);
        });
        e.reset();
    }
};

// One pass over the cells in k_zonal_partials' frame; LANE is ZtLaneA<T> or ZtLaneB<T>.  `head`: the cells peeled so that the value
// loads start 16-byte aligned; the bits above bit 7 are not looked at: every load is nt.  The tile loop is zonal_walk's, written out, with
// the lane's part of a group in it: the first-valid-id scan, before_group, the cells.
template <typename T, typename ZT, bool MASKED, int U, typename LANE>
__global__ __launch_bounds__(ezt::kBlock) void k_ztable_pass(const T* __restrict__ p, const uint8_t* __restrict__ mask, const ZT* __restrict__ zones,
                                                             size_t n, int32_t n_zones, ztword* table, unsigned head) {
    ZtLane<LANE> lane;
    lane.init(table, stats_pivot<T>(p), n_zones);  // the FIRST cell of the buffer, before the peel moves p
    head &= 0xffu;
    p += head;
    zones += head;
    if constexpr (MASKED) mask += head;
    n -= head;
    constexpr int CPL = 16 / sizeof(T);
    using TV = cells<T, CPL>;
    using MV = cells<uint8_t, CPL>;
    using ZV = cells<ZT, CPL>;
    const size_t ngroups = n / CPL;
    constexpr size_t TILE = size_t(ezt::kBlock) * U;
    const size_t ntiles = (ngroups + TILE - 1) / TILE;
    for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const size_t base = tile * TILE + threadIdx.x;
        TV x[U] = {};
        MV m[U] = {};
        ZV z[U] = {};
        bool in[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const size_t g = base + size_t(j) * ezt::kBlock;
            in[j] = g < ngroups;
            if (in[j]) {
                x[j] = load_cells<true, T, CPL>(p + g * CPL);
                z[j] = load_cells<true, ZT, CPL>(zones + g * CPL);
                if constexpr (MASKED) m[j] = load_cells<true, uint8_t, CPL>(mask + g * CPL);
            }
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
            int32_t first = lane.cur;  // the zone of the group's first cell that counts
            bool found = false;
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                const int32_t zk = zone_id(z[j][k]);
                const bool valid = in[j] && (!MASKED || m[j][k] != 0) && zone_in_range(zk, n_zones);
                first = valid && !found ? zk : first;
                found = found || valid;
            }
            lane.before_group(first != lane.cur);
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                const int32_t zk = zone_id(z[j][k]);
                lane.cell(in[j] && (!MASKED || m[j][k] != 0) && zone_in_range(zk, n_zones), x[j][k], zk);
            }
        }
    }
    zonal_walk_edges<T, ZT, MASKED>(p, mask, zones, ngroups * CPL, n, head, lane);
    lane.finish();  // every lane of every wave arrives
}

// Same pass, cell-wise loads: any alignment (the plan's other outcome, "unaligned_vector" off).
template <typename T, typename ZT, bool MASKED, typename LANE>
__global__ __launch_bounds__(ezt::kBlock) void k_ztable_pass_cellwise(const T* __restrict__ p, const uint8_t* __restrict__ mask,
                                                                      const ZT* __restrict__ zones, size_t n, int32_t n_zones, ztword* table) {
    ZtLane<LANE> lane;
    lane.init(table, stats_pivot<T>(p), n_zones);
    zonal_walk_cellwise<T, ZT, MASKED>(p, mask, zones, n, lane);
    lane.finish();
}

// The identity of every word of the table: total_words = n_zones * words(kind) < 2^28.
template <typename T>
__global__ __launch_bounds__(ezt::kBlock) void k_ztable_init(ztword* __restrict__ table, uint32_t total_words) {
    constexpr uint32_t W = ezt::words(StatsKind<T>::value);
    const uint32_t stride = gridDim.x * ezt::kBlock;
    for (uint32_t i = blockIdx.x * ezt::kBlock + threadIdx.x; i < total_words; i += stride) {
        const uint32_t w = i % W;
        table[i] = w == ezt::kNotMin ? static_cast<ztword>(zt_not_min_identity<T>()) : w == ezt::kMax ? static_cast<ztword>(zt_max_identity<T>()) : 0ull;
    }
}

// One lane per zone: entry z to record z.  first_cell_or_null: for the call's pivot (null: n == 0, pivot 0.0).
template <typename T>
__global__ __launch_bounds__(ezt::kBlock) void k_ztable_finalize(const ztword* __restrict__ table, int32_t n_zones, const T* __restrict__ first_cell_or_null,
                                                                 ec_moments* __restrict__ records) {
    constexpr int KIND = StatsKind<T>::value;
    constexpr int W = ezt::words(KIND);
    const uint32_t z = blockIdx.x * ezt::kBlock + threadIdx.x;
    if (z >= static_cast<uint32_t>(n_zones)) return;
    const ztword* e = table + size_t(z) * W;
    ec_moments* out = records + z;
    out->count = e[ezt::kCount];
    out->keys2[0] = static_cast<int64_t>(e[ezt::kNotMin]);
    out->keys2[1] = static_cast<int64_t>(e[ezt::kMax]);
    out->kind = KIND;
    out->dtype = ecl::dtype_of<T>::value;
    if constexpr (KIND == 0) {
        const uint64_t lo = e[ezt::kSq0], hi = e[ezt::kSq1];
        const uint64_t sq_lo = lo + (hi << 32);
        out->u.i.sum = static_cast<int64_t>(e[ezt::kSum]);
        out->u.i.sq_lo = sq_lo;
        out->u.i.sq_hi = (hi >> 32) + (sq_lo < lo ? 1u : 0u);
    } else {
        double s1, s2;
        ezt::zone_sums(e[ezt::kDmax], e[ezt::kFlags], e[ezt::kT1Lo], static_cast<int64_t>(e[ezt::kT1Hi]), e[ezt::kT2Lo], static_cast<int64_t>(e[ezt::kT2Hi]),
                       &s1, &s2);
        out->u.f.pivot = first_cell_or_null ? stats_pivot<T>(first_cell_or_null) : 0.0;
        out->u.f.s1 = s1;
        out->u.f.s2 = s2;
    }
    out->reserved = 0;
}

// ---- ec_zonal_lookup: zonal_gather (ec_zonal_kernels.hpp) without ec_zonal_broadcast's staging: the table is read where it
// lies, with plain (cacheable) loads — a table of 2^24 cells does not fit a workgroup, and the L2 serves the re-reads.
template <typename W, typename ZT, bool MASKOUT, int U>
__global__ __launch_bounds__(kBlock) void k_zonal_lookup(const ZT* __restrict__ zones, const W* __restrict__ table, int32_t n_zones,
                                                         W* __restrict__ dst, uint8_t* __restrict__ dst_mask, size_t n, size_t first_tile) {
    zonal_gather<W, ZT, MASKOUT, U>(zones, table, n_zones, dst, dst_mask, n, first_tile);
}

template <typename W, typename ZT, bool MASKOUT>
__global__ __launch_bounds__(kBlock) void k_zonal_lookup_cellwise(const ZT* __restrict__ zones, const W* __restrict__ table, int32_t n_zones,
                                                                  W* __restrict__ dst, uint8_t* __restrict__ dst_mask, size_t n) {
    zonal_gather_cellwise<W, ZT, MASKOUT>(zones, table, n_zones, dst, dst_mask, n);
}

}  // namespace ecd
