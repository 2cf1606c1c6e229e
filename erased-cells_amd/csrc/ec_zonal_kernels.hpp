// ec_zonal_kernels.hpp — per-zone band statistics and the way back (gfx950): the device side of ec_zonal_stats_device and
// ec_zonal_broadcast (include/erased_cells.h).  A reduction whose destination is data-dependent: cell i goes to the record
// of zone zones[i].
//
// The frame is the reductions' (ec_reduce_plan.hpp), walked by zonal_walk (below, shared with the table family): the
// launch shape of reduce_plan(), a read-only stream at 16 B of values per lane with the zone ids (and mask bytes) of the same
// cells beside them, every load nt, the peeled head and the ragged tail folded cell by cell by workgroup 0, a cell-wise kernel
// for "unaligned_vector" off.  ZoneScan is the walk's visitor; what it leaves is this family's: one Moments per workgroup AND ZONE
// in the caller's workspace, one finalize workgroup per zone over block_fold — or, with a one-workgroup grid, the records
// written by that workgroup itself.  What is folded is ec_stats_kernels.hpp's: CellMoments, FoldMoments, write_record.
//
// The destination.  A workgroup keeps its tables in LDS (ec_zonal_plan.hpp lds_layout).  No cell goes to a table on its own:
//   1. A lane keeps ONE running record (ZoneScan::acc) for ONE zone (ZoneScan::cur).  While every lane of the wave sees, in its
//      next 16-byte group, nothing but its own current zone (or ids that belong to no zone), the cells are folded in the lane
//      and nothing else happens: on a spatially coherent zone raster that is nearly every group.
//   2. Otherwise the wave flushes — the lanes' records go to the tables by wave_scatter — and folds the group slot by slot:
//      wave_scatter over the 64 cells of a slot.
//   wave_scatter serves the DISTINCT ids of the wave's lanes a round each (wave_rounds): the contributions of the lanes that
//   hold the id folded by wave_fold with every other lane SELECTED to the identity (never multiplied by 0), and lane 0 adds the
//   result to the table entry.
// Kind 1 sums live in one {s1, s2} table per wave that only its wave touches, with plain LDS reads and writes.  So the order
// of the additions is fixed: the wave's own program order, lanes by wave_fold's butterfly, then waves in wave order (the
// workgroup's epilogue), then workgroups in workgroup order (the finalize fold).  No float atomics: the records are a pure
// function of the cells, the zones and the launch plan.  The count, the two keys and the kind 0 sums are integers; their
// tables are one per workgroup, under integer LDS atomics — exact in any order.
//
// Overflow.  n is bounded as for ec_stats_device (stats_max_cells).  A lane's running record is CellMoments, whose bounds
// (ec_stats_kernels.hpp) are stated for a lane's share of n / 256 cells — the share of a lane here.  The tables' bounds stand
// beside them in ZoneScan.
#pragma once

#include "ec_lattice.hpp"
#include "ec_map_kernels.hpp"
#include "ec_stats_kernels.hpp"
#include "ec_zonal_plan.hpp"

namespace ecd {

static_assert(sizeof(Moments) == ecz::kPartialBytes && sizeof(ec_moments) == ecz::kRecordBytes, "the workspace is sized in Moments");
static_assert(ecz::kBlock == kBlock && ecz::kWave == kWave, "the plan header restates the workgroup of the cell-wise kernels");

// ---- The frame both zonal families share (this one: tables in LDS; ec_zonal_table_kernels.hpp: a table in global memory): the zone
// ids, the walk over the cells, the rounds over a wave's distinct ids, the gather dst[i] = table[zones[i]].  What a family does with
// a cell is its visitor's; nothing in the frame knows the families.

// zone ids are u8, u16 (never negative) or i32; a cell belongs to zone z iff 0 <= z < n_zones
template <typename ZT>
__device__ __forceinline__ int32_t zone_id(ZT z) { return static_cast<int32_t>(z); }
__device__ __forceinline__ bool zone_in_range(int32_t z, int32_t n_zones) { return static_cast<uint32_t>(z) < static_cast<uint32_t>(n_zones); }

// The whole wave, converged: f(zid, member, first) once for each DISTINCT id among the lanes that hold something (`has`; lane l
// holds z) — the id of the first lane not yet served (readlane), `member`: this lane holds it, `first`: that lane.  Rounds =
// distinct ids.  Which lane then issues anything is the caller's.
template <typename F>
__device__ __forceinline__ void wave_rounds(bool has, int32_t z, F&& f) {
    uint64_t rest = __builtin_amdgcn_ballot_w64(has);
    while (rest) {
        const int first = __builtin_ctzll(rest);
        const int32_t zid = __builtin_amdgcn_readlane(z, first);
        const bool member = has && z == zid;
        rest &= ~__builtin_amdgcn_ballot_w64(member);
        f(zid, member, first);
    }
}

// The edges of the walk below, by workgroup 0, a cell per lane: the ragged tail [first_cell, n) of the peeled streams and the `head`
// cells in front of them.  visitor.cell(in, x, m, z) is called by whole waves, converged: the loop bounds are the workgroup's; a lane
// past the end gets in == false, and its dummy load is at `first`, an address inside the buffer.
template <typename T, typename ZT, bool MASKED, typename V>
__device__ __forceinline__ void zonal_walk_edges(const T* __restrict__ p, const uint8_t* __restrict__ mask, const ZT* __restrict__ zones, size_t first_cell,
                                                 size_t n, unsigned head, V& visitor) {
    if (blockIdx.x != 0) return;
    for (size_t first = first_cell; first < n; first += ecz::kBlock) {
        const size_t i = first + threadIdx.x;
        const bool in = i < n;
        const size_t at = in ? i : first;
        visitor.cell(in, ld_cell(p + at), MASKED ? ld_cell(mask + at) : uint8_t(1), zone_id(ld_cell(zones + at)));
    }
    for (unsigned first = 0; first < head; first += ecz::kBlock) {
        const unsigned h = first + threadIdx.x;
        const bool in = h < head;
        const ptrdiff_t at = -static_cast<ptrdiff_t>(in ? h : first) - 1;
        visitor.cell(in, ld_cell(p + at), MASKED ? ld_cell(mask + at) : uint8_t(1), zone_id(ld_cell(zones + at)));
    }
}

// The walk of one workgroup over the values p, their zone ids and (MASKED) mask bytes, in the reductions' frame: the grid-stride
// tiles of reduce_plan(), U 16-byte groups of values per lane with the ids and mask bytes of the same cells beside them, every load
// nt; then zonal_walk_edges.  `head`: the cells peeled so that the value loads start 16-byte aligned (reduce_head); the bits above
// bit 7 (the launch's load policy) are not looked at.
// Every visitor.group<MASKED, CPL, ZT>(in, x, m, z) and visitor.cell(in, x, m, z) is called by whole waves, converged: the loop
// bounds are the workgroup's; a lane past the end gets in == false, and its dummy load is at `first`, inside the buffer.
template <typename T, typename ZT, bool MASKED, int U, typename V>
__device__ __forceinline__ void zonal_walk(const T* __restrict__ p, const uint8_t* __restrict__ mask, const ZT* __restrict__ zones, size_t n, unsigned head,
                                           V& visitor) {
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
    constexpr size_t TILE = size_t(ecz::kBlock) * U;
    const size_t ntiles = (ngroups + TILE - 1) / TILE;
    for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const size_t base = tile * TILE + threadIdx.x;
        TV x[U] = {};
        MV m[U] = {};
        ZV z[U] = {};
        bool in[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const size_t g = base + size_t(j) * ecz::kBlock;
            in[j] = g < ngroups;
            if (in[j]) {
                x[j] = load_cells<true, T, CPL>(p + g * CPL);
                z[j] = load_cells<true, ZT, CPL>(zones + g * CPL);
                if constexpr (MASKED) m[j] = load_cells<true, uint8_t, CPL>(mask + g * CPL);
            }
        }
#pragma unroll
        for (int j = 0; j < U; ++j) visitor.template group<MASKED, CPL, ZT>(in[j], x[j], m[j], z[j]);
    }
    zonal_walk_edges<T, ZT, MASKED>(p, mask, zones, ngroups * CPL, n, head, visitor);
}

// Same walk, cell-wise loads: any alignment (the plan's other outcome, "unaligned_vector" off).
template <typename T, typename ZT, bool MASKED, typename V>
__device__ __forceinline__ void zonal_walk_cellwise(const T* __restrict__ p, const uint8_t* __restrict__ mask, const ZT* __restrict__ zones, size_t n,
                                                    V& visitor) {
    const size_t stride = size_t(gridDim.x) * ecz::kBlock;
    for (size_t first = size_t(blockIdx.x) * ecz::kBlock; first < n; first += stride) {
        const size_t i = first + threadIdx.x;
        const bool in = i < n;
        const size_t at = in ? i : first;
        visitor.cell(in, p[at], MASKED ? mask[at] : uint8_t(1), zone_id(zones[at]));
    }
}

// ---- The gather dst[i] = tab[zones[i]], bits copied by cell width W, mask byte 1; an id that belongs to no zone gives all-zero
// bits and mask byte 0.  The map kernels' frame (k_map, ec_map_kernels.hpp: one workgroup per tile of U groups per lane, two
// fronts, nt loads and stores, the ragged tail by workgroup 0).  `tab`: the n_zones cells wherever the kernel keeps them.
template <typename W, typename ZT, bool MASKOUT>
__device__ __forceinline__ void zonal_gather_cell(const ZT* __restrict__ zones, const W* tab, int32_t n_zones, W* __restrict__ dst,
                                                  uint8_t* __restrict__ dst_mask, size_t i) {
    const int32_t zk = zone_id(ld_cell(zones + i));
    const bool ok = zone_in_range(zk, n_zones);
    st_cell<W>(ok ? tab[ok ? zk : 0] : W(0), dst + i);
    if constexpr (MASKOUT) st_cell<uint8_t>(ok ? 1 : 0, dst_mask + i);
}

template <typename W, typename ZT, bool MASKOUT, int U>
__device__ __forceinline__ void zonal_gather(const ZT* __restrict__ zones, const W* tab, int32_t n_zones, W* __restrict__ dst,
                                             uint8_t* __restrict__ dst_mask, size_t n, size_t first_tile) {
    constexpr int CPL = 16 / max_of<sizeof(W), sizeof(ZT)>::value;
    using DV = vec<W, CPL>;
    using MV = vec<uint8_t, CPL>;
    const size_t ngroups = n / CPL;
    constexpr size_t TILE = size_t(kBlock) * U;
    const size_t base = two_front_tile(first_tile) * TILE + threadIdx.x;
    cells<ZT, CPL> z[U] = {};
#pragma unroll
    for (int j = 0; j < U; ++j) {
        const size_t g = base + size_t(j) * kBlock;
        if (g < ngroups) z[j] = load_cells<true, ZT, CPL>(zones + g * CPL);
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
        const size_t g = base + size_t(j) * kBlock;
        if (g >= ngroups) continue;
        DV o;
        MV m;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int32_t zk = zone_id(z[j][k]);
            const bool ok = zone_in_range(zk, n_zones);
            o[k] = ok ? tab[ok ? zk : 0] : W(0);
            m[k] = ok ? 1 : 0;
        }
        nt_store(o, reinterpret_cast<DV*>(dst) + g);
        if constexpr (MASKOUT) mask_store(m, reinterpret_cast<MV*>(dst_mask) + g);
    }
    if (first_group(first_tile))
        for (size_t i = ngroups * CPL + threadIdx.x; i < n; i += kBlock) zonal_gather_cell<W, ZT, MASKOUT>(zones, tab, n_zones, dst, dst_mask, i);
}

template <typename W, typename ZT, bool MASKOUT>
__device__ __forceinline__ void zonal_gather_cellwise(const ZT* __restrict__ zones, const W* tab, int32_t n_zones, W* __restrict__ dst,
                                                      uint8_t* __restrict__ dst_mask, size_t n) {
    const size_t stride = size_t(gridDim.x) * kBlock;
    for (size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) zonal_gather_cell<W, ZT, MASKOUT>(zones, tab, n_zones, dst, dst_mask, i);
}

// ---- This family

// The first cell of a lane's group, and the group moved up by one cell: the slot loop of ZoneScan::group stays a loop (one copy
// of wave_scatter per group, not one per slot) without indexing registers by a loop variable.
template <typename T, int N>
__device__ __forceinline__ T pop_front(cells<T, N>& c) {
    const T first = c[0];
    if constexpr (sizeof(T) == 1) {
        if constexpr (N <= 4) c.v = static_cast<typename cells<T, N>::rep>(c.v >> 8);
        else if constexpr (N == 8) c.v = typename cells<T, N>::rep{(c.v[0] >> 8) | (c.v[1] << 24), c.v[1] >> 8};
        else c.v = typename cells<T, N>::rep{(c.v[0] >> 8) | (c.v[1] << 24), (c.v[1] >> 8) | (c.v[2] << 24), (c.v[2] >> 8) | (c.v[3] << 24), c.v[3] >> 8};
    } else {
        if constexpr (N == 2) c.v = __builtin_shufflevector(c.v, c.v, 1, 0);
        else if constexpr (N == 4) c.v = __builtin_shufflevector(c.v, c.v, 1, 2, 3, 0);
        else if constexpr (N == 8) c.v = __builtin_shufflevector(c.v, c.v, 1, 2, 3, 4, 5, 6, 7, 0);
        else c.v = __builtin_shufflevector(c.v, c.v, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 0);
    }
    return first;
}

template <typename T>
struct ZoneScan {
    static constexpr int KIND = StatsKind<T>::value;
    // the workgroup's tables, n_zones entries each (whole-launch bounds: a grid may be one workgroup)
    unsigned long long* count;  // <= n <= 2^32
    long long* kmin;            // order keys
    long long* kmax;
    unsigned long long* sum;    // kind 0: two's complement, |sum| <= n * max|x| < 2^63
    unsigned long long* sq_lo;  // kind 0: wraps; every wrap is seen by the add that caused it and carried into sq_hi
    uint32_t* sq_hi;            // kind 0: sum of squares < 2^96, so sq_hi < 2^32
    double* s1;                 // kind 1: THIS WAVE's table
    double* s2;
    int32_t n_zones;
    double pivot;
    int32_t cur;                // the zone of `acc`, -1: none yet
    CellMoments<T, false> acc;  // the lane's running record: at most n / 256 + 32 cells (bounds: ec_stats_kernels.hpp)

    // every thread of the workgroup; ends in a barrier
    __device__ __forceinline__ void init(unsigned char* lds, int32_t nz, double c) {
        const ecz::LdsLayout l = ecz::lds_layout(nz, KIND);
        count = reinterpret_cast<unsigned long long*>(lds + l.off_count);
        kmin = reinterpret_cast<long long*>(lds + l.off_kmin);
        kmax = reinterpret_cast<long long*>(lds + l.off_kmax);
        sum = reinterpret_cast<unsigned long long*>(lds + l.off_sum);
        sq_lo = reinterpret_cast<unsigned long long*>(lds + l.off_sq_lo);
        sq_hi = reinterpret_cast<uint32_t*>(lds + l.off_sq_hi);
        double* all_s1 = reinterpret_cast<double*>(lds + l.off_s1);
        double* all_s2 = reinterpret_cast<double*>(lds + l.off_s2);
        n_zones = nz;
        pivot = c;
        const Moments id = moments_identity<T>();
        for (int z = threadIdx.x; z < nz; z += ecz::kBlock) {
            count[z] = 0;
            kmin[z] = id.kmin;
            kmax[z] = id.kmax;
            if constexpr (KIND == 0) {
                sum[z] = 0;
                sq_lo[z] = 0;
                sq_hi[z] = 0;
            } else {
#pragma unroll
                for (int w = 0; w < ecz::kWaves; ++w) all_s1[w * nz + z] = all_s2[w * nz + z] = 0.0;
            }
        }
        const int wave = threadIdx.x / kWave;
        s1 = all_s1 + wave * nz;
        s2 = all_s2 + wave * nz;
        cur = -1;
        acc.init();
        __syncthreads();
    }

    // lane 0 of a wave: the fold of the wave's members of zone z into the tables
    __device__ __forceinline__ void add_to_tables(int32_t z, const Moments& c) {
        __hip_atomic_fetch_add(count + z, static_cast<unsigned long long>(c.count), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_min(kmin + z, static_cast<long long>(c.kmin), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_max(kmax + z, static_cast<long long>(c.kmax), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if constexpr (KIND == 0) {
            __hip_atomic_fetch_add(sum + z, static_cast<unsigned long long>(c.a), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const unsigned long long b = c.b;
            const unsigned long long old = __hip_atomic_fetch_add(sq_lo + z, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const uint32_t carry = old + b < old ? 1u : 0u;  // this add wrapped the low word
            __hip_atomic_fetch_add(sq_hi + z, static_cast<uint32_t>(c.c) + carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
            s1[z] += bits_f64(c.a);  // this wave's table: plain read and write, program order
            s2[z] += bits_f64(c.b);
        }
    }

    // The whole wave, converged.  Lane l contributes `mine` to zone z iff valid; z is in range wherever valid is set.
    __device__ __forceinline__ void wave_scatter(bool valid, int32_t z, const Moments& mine) {
        const Moments id = moments_identity<T>();
        wave_rounds(valid, z, [&](int32_t zid, bool member, int) {
            Moments c;
            c.count = member ? mine.count : id.count;
            c.kmin = member ? mine.kmin : id.kmin;
            c.kmax = member ? mine.kmax : id.kmax;
            c.a = member ? mine.a : id.a;
            c.b = member ? mine.b : id.b;
            c.c = member ? mine.c : id.c;
            c = wave_fold(c, FoldMoments<KIND>{});
            if ((threadIdx.x & (kWave - 1)) == 0) add_to_tables(zid, c);
        });
    }

    // The whole wave, converged: the lanes' running records to the tables.
    __device__ __forceinline__ void flush() {
        if (__builtin_amdgcn_ballot_w64(cur >= 0) == 0) return;
        wave_scatter(cur >= 0, cur, acc.partial());
        cur = -1;
        acc.init();
    }

    __device__ __forceinline__ Moments one_cell(bool valid, T x) const {
        CellMoments<T, false> one;
        one.init();
        if (valid) one.add(x, pivot);
        return one.partial();
    }

    // The whole wave, converged: one cell per lane (`in`: the lane has one).  `m`: its mask byte, 1 without a mask.
    __device__ __forceinline__ void cell(bool in, T x, uint8_t m, int32_t z) {
        const bool valid = in && m != 0 && zone_in_range(z, n_zones);
        const bool stays = !valid || cur < 0 || cur == z;
        if (__builtin_amdgcn_ballot_w64(!stays) == 0) {
            if (valid) {
                cur = z;
                acc.add(x, pivot);
            }
        } else {
            flush();
            wave_scatter(valid, z, one_cell(valid, x));
        }
    }

    // The whole wave, converged: one 16-byte group of values per lane (`in`: the lane has one) with its ids and mask bytes.
    template <bool MASKED, int CPL, typename ZT>
    __device__ __forceinline__ void group(bool in, const cells<T, CPL>& x, const cells<uint8_t, CPL>& m, const cells<ZT, CPL>& z) {
        const int32_t z0 = zone_id(z[0]);
        bool uniform = true;
#pragma unroll
        for (int k = 1; k < CPL; ++k) uniform = uniform && zone_id(z[k]) == z0;
        const bool counts = in && zone_in_range(z0, n_zones);  // with `uniform`: the group's cells are zone z0's
        const bool stays = !in || (uniform && (!counts || cur < 0 || cur == z0));
        if (__builtin_amdgcn_ballot_w64(!stays) == 0) {
            if (counts) {
                cur = z0;
#pragma unroll
                for (int k = 0; k < CPL; ++k)
                    if (!MASKED || m[k]) acc.add(x[k], pivot);
            }
        } else {
            flush();
            cells<T, CPL> xs = x;
            cells<uint8_t, CPL> ms = m;
            cells<ZT, CPL> zs = z;
#pragma unroll 1
            for (int k = 0; k < CPL; ++k) {  // slot by slot
                const T xk = pop_front(xs);
                const bool shown = !MASKED || pop_front(ms) != 0;
                const int32_t zk = zone_id(pop_front(zs));
                const bool valid = in && shown && zone_in_range(zk, n_zones);
                wave_scatter(valid, zk, one_cell(valid, xk));
            }
        }
    }

    // After a barrier behind the last flush: the workgroup's Moments of zone z, the waves' kind 1 sums in wave order.
    __device__ __forceinline__ Moments result(int z) const {
        Moments r;
        r.count = count[z];
        r.kmin = kmin[z];
        r.kmax = kmax[z];
        if constexpr (KIND == 0) {
            r.a = sum[z];
            r.b = sq_lo[z];
            r.c = sq_hi[z];
        } else {
            const int wave = threadIdx.x / kWave;
            const double* w1 = s1 - wave * n_zones;  // wave 0's tables
            const double* w2 = s2 - wave * n_zones;
            double a = w1[z], b = w2[z];
#pragma unroll
            for (int w = 1; w < ecz::kWaves; ++w) {
                a += w1[w * n_zones + z];
                b += w2[w * n_zones + z];
            }
            r.a = f64_bits(a);
            r.b = f64_bits(b);
            r.c = 0;
        }
        return r;
    }

    // every thread of the workgroup: the tables to the workspace, or (a one-workgroup grid) the records themselves
    __device__ __forceinline__ void write_out(Moments* __restrict__ partials, ec_moments* __restrict__ records_if_single) {
        flush();
        __syncthreads();
        for (int z = threadIdx.x; z < n_zones; z += ecz::kBlock) {
            const Moments r = result(z);
            if (records_if_single) write_record<T>(records_if_single + z, r, pivot);
            else partials[ecz::partial_index(z, blockIdx.x, gridDim.x)] = r;
        }
    }
};

// partials[partial_index(z, b, grid)] = the Moments of zone z in workgroup b's cells, over zonal_walk (`head`: its peel).
// records_if_single != nullptr (one-workgroup grid): the workgroup writes the n_zones records itself.
template <typename T, typename ZT, bool MASKED, int U>
__global__ __launch_bounds__(ecz::kBlock) void k_zonal_partials(const T* __restrict__ p, const uint8_t* __restrict__ mask,
                                                                 const ZT* __restrict__ zones, size_t n, int32_t n_zones,
                                                                 Moments* __restrict__ partials, unsigned head,
                                                                 ec_moments* __restrict__ records_if_single) {
    extern __shared__ __attribute__((aligned(16))) unsigned char zonal_lds[];
    ZoneScan<T> scan;
    scan.init(zonal_lds, n_zones, stats_pivot<T>(p));  // the FIRST cell of the buffer, before the walk's peel
    zonal_walk<T, ZT, MASKED, U>(p, mask, zones, n, head, scan);
    scan.write_out(partials, records_if_single);
}

// Same reduction, cell-wise loads: any alignment (the plan's other outcome, "unaligned_vector" off).
template <typename T, typename ZT, bool MASKED>
__global__ __launch_bounds__(ecz::kBlock) void k_zonal_partials_cellwise(const T* __restrict__ p, const uint8_t* __restrict__ mask,
                                                                          const ZT* __restrict__ zones, size_t n, int32_t n_zones,
                                                                          Moments* __restrict__ partials,
                                                                          ec_moments* __restrict__ records_if_single) {
    extern __shared__ __attribute__((aligned(16))) unsigned char zonal_lds[];
    ZoneScan<T> scan;
    scan.init(zonal_lds, n_zones, stats_pivot<T>(p));
    zonal_walk_cellwise<T, ZT, MASKED>(p, mask, zones, n, scan);
    scan.write_out(partials, records_if_single);
}

// Workgroup z folds zone z's partials in workgroup order (a thread takes every 256th, then block_fold: k_stats_finalize's
// fold) and writes record z; nparts == 0 (n == 0) writes the empty records.  first_cell_or_null: for the pivot.
template <typename T>
__global__ __launch_bounds__(kStatsFinalizeBlock) void k_zonal_finalize(const Moments* __restrict__ partials, int nparts,
                                                                         const T* __restrict__ first_cell_or_null,
                                                                         ec_moments* __restrict__ records) {
    const FoldMoments<StatsKind<T>::value> op;
    const int z = blockIdx.x;
    partials += ecz::partial_index(z, 0u, static_cast<unsigned>(nparts));
    Moments acc = moments_identity<T>();
#pragma unroll 4
    for (int i = threadIdx.x; i < nparts; i += kStatsFinalizeBlock) acc = op(acc, partials[i]);
    if (block_fold<kStatsFinalizeBlock>(acc, op)) write_record<T>(records + z, acc, first_cell_or_null ? stats_pivot<T>(first_cell_or_null) : 0.0);
}

// ---- ec_zonal_broadcast: zonal_gather (above) with the table staged in LDS first (2 KiB at the most, loaded nt
// like every other access: the L2 serves the workgroups' re-reads all the same).
template <typename W, typename ZT, bool MASKOUT, int U>
__global__ __launch_bounds__(kBlock) void k_zonal_broadcast(const ZT* __restrict__ zones, const W* __restrict__ table, int32_t n_zones,
                                                            W* __restrict__ dst, uint8_t* __restrict__ dst_mask, size_t n, size_t first_tile) {
    __shared__ W tab[ecz::kMaxZones];
    for (int z = threadIdx.x; z < n_zones; z += kBlock) tab[z] = ld_cell(table + z);
    __syncthreads();
    zonal_gather<W, ZT, MASKOUT, U>(zones, tab, n_zones, dst, dst_mask, n, first_tile);
}

template <typename W, typename ZT, bool MASKOUT>
__global__ __launch_bounds__(kBlock) void k_zonal_broadcast_cellwise(const ZT* __restrict__ zones, const W* __restrict__ table,
                                                                     int32_t n_zones, W* __restrict__ dst, uint8_t* __restrict__ dst_mask,
                                                                     size_t n) {
    __shared__ W tab[ecz::kMaxZones];
    for (int z = threadIdx.x; z < n_zones; z += kBlock) tab[z] = ld_cell(table + z);
    __syncthreads();
    zonal_gather_cellwise<W, ZT, MASKOUT>(zones, tab, n_zones, dst, dst_mask, n);
}

}  // namespace ecd
