// ec_zonal_plan.hpp — what the host side and the kernels of the zonal statistics (include/erased_cells.h: ec_zonal_stats_device,
// ec_zonal_broadcast) share, in plain C++: the launch constants, the refusals and their order, the size of the caller's
// workspace and the layout of a workgroup's tables in LDS.
//
// Self-contained: no HIP include and nothing from this library but ec_reduce_plan.hpp (kMaxReduceBlocks) and ec_refusal.hpp, so
// that host/test_zonal_plan.cpp runs these very functions under the address and undefined-behaviour sanitizers.  The functions
// the kernels call are constexpr: hipcc compiles a constexpr function for both sides.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "ec_reduce_plan.hpp"
#include "ec_refusal.hpp"

namespace ecz {

constexpr int32_t kMaxZones = 256;     // EC_ZONAL_MAX_ZONES
constexpr int kBlock = 256;            // threads of a workgroup of the zonal kernels, vector and cell-wise
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
constexpr int kU = 4;                  // 16-byte value loads in flight per lane of a tile
constexpr int kPerCu = 4;              // workgroups per CU: 4 x 22 KiB of LDS at 256 zones, under the 160 KiB of a CU
constexpr size_t kPartialBytes = 48;   // one Moments (ec_reduce_kernels.hpp) per workgroup and zone
constexpr size_t kRecordBytes = 64;    // one ec_moments

constexpr bool valid_zones(int32_t n_zones) { return n_zones >= 1 && n_zones <= kMaxZones; }

// ec_zonal_workspace_bytes: a partial per zone for every workgroup a reduction can launch (reduce_cap never passes
// kMaxReduceBlocks).  Depends on n_zones only.
constexpr size_t workspace_bytes(int32_t n_zones) {
    return valid_zones(n_zones) ? size_t(n_zones) * size_t(ecd::kMaxReduceBlocks) * kPartialBytes : 0;
}

// Where workgroup `block` of a grid of `grid` leaves its partial of zone z, in partials from the start of the workspace:
// zone-major, so that the finalize workgroup of zone z reads `grid` consecutive partials in workgroup order.
constexpr size_t partial_index(int32_t z, unsigned block, unsigned grid) { return size_t(z) * grid + block; }

// The tables of one workgroup, in bytes from the start of its dynamic LDS; every table has n_zones entries.
//   count, kmin, kmax   8 bytes each: the cells counted and the two order keys — one table per workgroup, integer LDS atomics
//   kind 0:  sum, sq_lo 8 bytes each, sq_hi 4 bytes — one table per workgroup, integer LDS atomics (the carry of sq_lo is
//            read off the value the atomic returns)
//   kind 1:  s1, s2     8 bytes each, ONE TABLE PER WAVE (kWaves of them, wave w's entry z at off + (w * n_zones + z) * 8):
//            only the owning wave touches its table, with plain reads and writes — no float atomics
// At 256 zones: 6 KiB + 5 KiB (kind 0) or 6 KiB + 16 KiB (kind 1).
struct LdsLayout {
    uint32_t off_count, off_kmin, off_kmax;
    uint32_t off_sum, off_sq_lo, off_sq_hi;  // kind 0 (kind 1: all equal to off_s1, unused)
    uint32_t off_s1, off_s2;                 // kind 1 (kind 0: equal to bytes, unused)
    uint32_t bytes;
};

constexpr LdsLayout lds_layout(int32_t n_zones, int kind) {
    LdsLayout l{};
    const uint32_t z = uint32_t(n_zones);
    l.off_count = 0;
    l.off_kmin = z * 8;
    l.off_kmax = z * 16;
    uint32_t at = z * 24;
    if (kind == 0) {
        l.off_sum = at;
        l.off_sq_lo = at + z * 8;
        l.off_sq_hi = at + z * 16;
        at += z * 20;
        at = (at + 7u) & ~7u;
        l.off_s1 = l.off_s2 = at;
    } else {
        l.off_sum = l.off_sq_lo = l.off_sq_hi = at;
        l.off_s1 = at;
        l.off_s2 = at + z * 8 * kWaves;
        at += z * 16 * kWaves;
    }
    l.bytes = at;
    return l;
}

constexpr bool valid_zone_type(int zt) { return zt == 0 /* EC_U8 */ || zt == 1 /* EC_U16 */ || zt == 6 /* EC_I32 */; }
constexpr size_t zone_size(int zt) { return zt == 0 ? 1 : zt == 1 ? 2 : zt == 6 ? 4 : 0; }

// The head of all four refusals of the two zonal families (this header, ec_zonal_table_plan.hpp), in the header's order: n_zones
// against the family's cap (`zones_ok`, the cap's text passed in), the two types, a null pointer (`null_pointer`: the caller's own
// test, it knows which pointers the call needs).  cell_size: bytes of a value cell, 0 for a bad t.
inline ecv::Refusal refusal_head(bool zones_ok, const char* cap_text, size_t cell_size, int zt, bool null_pointer) {
    if (!zones_ok) return {cap_text};
    if (cell_size == 0) return {"bad dtype", true};
    if (!valid_zone_type(zt)) return {"the zone raster's type is not EC_U8, EC_U16 or EC_I32", true};
    if (null_pointer) return {"null pointer"};
    return {};
}

// The tail of a statistics call: the records and the workspace against the values, the mask and the zone ids, then each other.
inline ecv::Refusal stats_overlap_refusal(const void* out, size_t out_bytes, const void* workspace, size_t ws, const void* p, const void* mask,
                                          const void* zones, size_t n, size_t cell_size, int zt) {
    const ecv::Span rec{out, out_bytes}, work{workspace, ws}, values{p, n * cell_size}, valid{mask, n}, ids{zones, n * zone_size(zt)};
    const ecv::OverlapRow rows[] = {{rec, values, "the records overlap an input"},  {work, values, "the workspace overlaps an input"},
                                    {rec, valid, "the records overlap an input"},   {work, valid, "the workspace overlaps an input"},
                                    {rec, ids, "the records overlap an input"},     {work, ids, "the workspace overlaps an input"},
                                    {rec, work, "the records overlap the workspace"}};
    return {ecv::first_overlap(rows)};
}

// Why ec_zonal_stats_device refuses a call, or nothing.  The order is the header's: refusal_head, n above the bound of one exact
// record (max_cells, 0 = none: stats_max_cells), an output overlapping an input.  caller_workspace false (the forms that take
// their workspace from the library's pool): `workspace` is not looked at, and `out` is host memory (out_bytes 0).
inline ecv::Refusal stats_refusal(int32_t n_zones, size_t cell_size, int zt, const void* p, const void* mask, const void* zones, size_t n,
                                  uint64_t max_cells, const void* out, size_t out_bytes, const void* workspace, bool caller_workspace) {
    const bool null_pointer = !out || (caller_workspace && !workspace) || (n > 0 && (!p || !zones));
    if (const ecv::Refusal r = refusal_head(valid_zones(n_zones), "n_zones is not within 1 .. EC_ZONAL_MAX_ZONES (256)", cell_size, zt, null_pointer)) return r;
    if (max_cells && n > max_cells) return {"more cells than one exact record covers: shard it (ec_stats_fold merges the records)"};
    return stats_overlap_refusal(out, out_bytes, workspace, caller_workspace ? workspace_bytes(n_zones) : 0, p, mask, zones, n, cell_size, zt);
}

// The tiles of an ec_zonal_broadcast launch: groups of cpl cells, kBlock * u groups per workgroup, one workgroup per tile.
constexpr int kBroadcastU = 2;
constexpr uint64_t kMaxTiles = 0x7fffffffull;
constexpr size_t broadcast_cpl(size_t cell_size, size_t zone_bytes) { return 16 / (cell_size > zone_bytes ? cell_size : zone_bytes); }
constexpr uint64_t broadcast_tiles(uint64_t n, size_t cpl) {
    return (n / cpl + uint64_t(kBlock) * kBroadcastU - 1) / (uint64_t(kBlock) * kBroadcastU);
}

// Why a gather (ec_zonal_broadcast, ec_zonal_lookup) refuses a call, or nothing; same order.  n == 0 passes whatever the pointers are.
inline ecv::Refusal gather_refusal(bool zones_ok, const char* cap_text, int32_t n_zones, size_t cell_size, int zt, const void* zones, const void* table,
                                   size_t n, const void* dst, const void* dst_mask) {
    if (const ecv::Refusal r = refusal_head(zones_ok, cap_text, cell_size, zt, n > 0 && (!zones || !table || !dst))) return r;
    if (n == 0) return {};
    if (broadcast_tiles(n, broadcast_cpl(cell_size, zone_size(zt))) > kMaxTiles) return {"more than 2^31 - 1 tiles"};
    const ecv::Span out{dst, n * cell_size}, out_mask{dst_mask, n}, ids{zones, n * zone_size(zt)}, tab{table, size_t(n_zones) * cell_size};
    const ecv::OverlapRow rows[] = {{out, ids, "dst overlaps an input (the operation is not in-place)"}, {out_mask, ids, "dst_mask overlaps an input"},
                                    {out, tab, "dst overlaps an input (the operation is not in-place)"}, {out_mask, tab, "dst_mask overlaps an input"},
                                    {out, out_mask, "dst_mask overlaps dst"}};
    return {ecv::first_overlap(rows)};
}

inline ecv::Refusal broadcast_refusal(int32_t n_zones, size_t cell_size, int zt, const void* zones, const void* table, size_t n, const void* dst,
                                      const void* dst_mask) {
    return gather_refusal(valid_zones(n_zones), "n_zones is not within 1 .. EC_ZONAL_MAX_ZONES (256)", n_zones, cell_size, zt, zones, table, n, dst, dst_mask);
}

}  // namespace ecz
