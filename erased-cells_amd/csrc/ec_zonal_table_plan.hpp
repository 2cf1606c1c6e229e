// ec_zonal_table_plan.hpp — what the host side and the kernels of the zonal table family (include/erased_cells.h:
// ec_zonal_table_device, ec_zonal_table_compute, ec_zonal_lookup) share, in plain C++: the cap, the launch constants, the layout
// of the per-zone table in the caller's workspace, the refusals and their order.
//
// Self-contained like ec_zonal_plan.hpp, whose zone types, broadcast tiling and the refusals' shared head and overlap tail it
// reuses: no HIP include.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "ec_zonal_plan.hpp"

namespace ezt {

constexpr int32_t kMaxZones = 1 << 24;  // EC_ZONAL_TABLE_MAX_ZONES: 2^24 records are 1 GiB; every byte offset stays below 2^32
constexpr int kBlock = 256;             // threads of a workgroup of every kernel of the family
constexpr int kU = 4;                   // 16-byte value loads in flight per lane of a tile (passes A and B)
constexpr int kPerCu = 8;               // workgroups per CU of passes A and B (no LDS).  NOT the resident count for every instantiation:
                                        // pass A holds up to 152 VGPRs for 1-byte values (3 workgroups a CU resident), so such a grid
                                        // runs in several rounds; nothing depends on one round, and the atomics bind, not the loads
constexpr int kFewIds = 4;              // a wave that holds at most this many zones folds them a round each before its atomics
constexpr uint64_t kMaxCellsKind1 = uint64_t(1) << 32;  // |T| < 2^63 * 2^32: the two limbs hold it

// The table: one entry of 64-bit words per zone, entry z at word z * words(kind).  All words are accumulated by agent-scope
// integer atomics: adds, signed max, unsigned max, or.
//   word 0   count                      add
//   word 1   ~key(min)                  signed max     identity ~key(T::MAX)
//   word 2   key(max)                   signed max     identity key(T::MIN)
//   kind 0:  3 sum (two's complement)   add
//            4, 5 squares, lo and hi limb              add
//   kind 1:  3 max of |d|'s bits        unsigned max
//            4 infinity flags           or
//            5, 6 T1 lo and hi limb; 7, 8 T2 lo and hi limb   add
//            9 unused (the entry is a multiple of 16 bytes)
enum : int { kCount = 0, kNotMin = 1, kMax = 2, kSum = 3, kSq0 = 4, kSq1 = 5, kDmax = 3, kFlags = 4, kT1Lo = 5, kT1Hi = 6, kT2Lo = 7, kT2Hi = 8 };
constexpr int words(int kind) { return kind == 0 ? 6 : 10; }

constexpr bool valid_zones(int32_t n_zones) { return n_zones >= 1 && n_zones <= kMaxZones; }

// ec_zonal_table_workspace_bytes.  kind: 0 or 1 (ecd::stats_kind of the value type), anything else a bad type.
constexpr size_t workspace_bytes(int kind, int32_t n_zones) {
    return valid_zones(n_zones) && (kind == 0 || kind == 1) ? size_t(n_zones) * size_t(words(kind)) * 8u : 0;
}

// Why ec_zonal_table_device refuses a call, or nothing; ec_zonal_stats_device's order and shared pieces (ecz::stats_refusal) with
// this family's cap, the kind's bound on n (max_cells) and the alignment of the records and the workspace before their overlaps.
// caller_workspace false (the forms that take workspace and records from the library's pool): `workspace` is not looked at and
// `out` is host memory of any alignment.
inline ecv::Refusal table_refusal(int32_t n_zones, size_t cell_size, int kind, int zt, const void* p, const void* mask, const void* zones, size_t n,
                                  uint64_t max_cells, const void* out, const void* workspace, bool caller_workspace) {
    const bool null_pointer = !out || (caller_workspace && !workspace) || (n > 0 && (!p || !zones));
    if (const ecv::Refusal r = ecz::refusal_head(valid_zones(n_zones), "n_zones is not within 1 .. EC_ZONAL_TABLE_MAX_ZONES (16777216)", cell_size, zt,
                                                 null_pointer))
        return r;
    if (n > max_cells) return {kind == 0 ? "more cells than one exact record covers: shard it (ec_stats_fold merges the records)"
                                          : "more than 2^32 cells: the truncated sums are bounded for 2^32 (shard it)"};
    if (!caller_workspace) return {};
    if (ecv::misaligned(out, 16)) return {"the records are not 16-byte aligned"};
    if (ecv::misaligned(workspace, 16)) return {"the workspace is not 16-byte aligned"};
    return ecz::stats_overlap_refusal(out, size_t(n_zones) * ecz::kRecordBytes, workspace, workspace_bytes(kind, n_zones), p, mask, zones, n, cell_size, zt);
}

// Why ec_zonal_lookup refuses a call, or nothing: ecz::broadcast_refusal with this family's cap.
inline ecv::Refusal lookup_refusal(int32_t n_zones, size_t cell_size, int zt, const void* zones, const void* table, size_t n, const void* dst,
                                   const void* dst_mask) {
    return ecz::gather_refusal(valid_zones(n_zones), "n_zones is not within 1 .. EC_ZONAL_TABLE_MAX_ZONES (16777216)", n_zones, cell_size, zt, zones,
                               table, n, dst, dst_mask);
}

}  // namespace ezt
