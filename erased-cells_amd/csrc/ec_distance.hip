// ec_distance.hip — ec_distance and ec_distance_workspace_bytes (include/erased_cells.h): the exact Euclidean distance transform of
// a mask.  The refusals (distance_refusal, ec_distance_line.hpp: before any device work and before the library asks for a device), the
// workspace — the caller's, or a block of the library's stream-ordered pool that goes back on the same stream — and the two launches: the column
// sweeps, then the row scans (ec_distance_kernels.hpp over ec_distance_line.hpp).
#include <hip/hip_runtime.h>

#include "ec_distance_kernels.hpp"
#include "ec_lattice.hpp"
#include "ec_runtime.hpp"

namespace ecd {

static_assert(EC_DISTANCE_MAX_SIDE == kDistMaxSide, "ec_distance_line.hpp restates the C ABI's limit");
static_assert(EC_DISTANCE_UNLIMITED == kDistNone, "no d2 reaches the sentinel, so UNLIMITED admits every real one");

template <typename OUT>
static void launch_rows(unsigned grid, const uint16_t* g, uint32_t cols, uint32_t rows, uint32_t max_sq, uint16_t* s, uint16_t* t, void* dst,
                        uint8_t* dst_mask, hipStream_t st) {
    OUT* out = static_cast<OUT*>(dst);
    if (dst && dst_mask) k_distance_rows<OUT, true, true><<<grid, kDistLines, 0, st>>>(g, cols, rows, max_sq, s, t, out, dst_mask);
    else if (dst) k_distance_rows<OUT, true, false><<<grid, kDistLines, 0, st>>>(g, cols, rows, max_sq, s, t, out, dst_mask);
    else k_distance_rows<OUT, false, true><<<grid, kDistLines, 0, st>>>(g, cols, rows, max_sq, s, t, out, dst_mask);
}

static ec_status launch_distance(const uint8_t* mask, uint32_t cols, uint32_t rows, uint32_t max_sq, int out_type, void* dst, uint8_t* dst_mask,
                                 void* workspace, hipStream_t st) {
    const DistWorkspace w = dist_workspace(cols, rows);
    char* base = static_cast<char*>(workspace);
    uint16_t* g = reinterpret_cast<uint16_t*>(base);
    uint16_t* s = reinterpret_cast<uint16_t*>(base + w.off_s);
    uint16_t* t = reinterpret_cast<uint16_t*>(base + w.off_t);
    k_distance_columns<<<unsigned(dist_waves(cols)), kDistLines, 0, st>>>(mask, cols, rows, g);
    ec_status e = check_launch("distance(columns)");
    if (e != EC_OK) return e;
    const unsigned grid = unsigned(dist_waves(rows));
    if (out_type == EC_U32) launch_rows<uint32_t>(grid, g, cols, rows, max_sq, s, t, dst, dst_mask, st);
    else launch_rows<double>(grid, g, cols, rows, max_sq, s, t, dst, dst_mask, st);
    return check_launch("distance(rows)");
}

}  // namespace ecd

using namespace ecd;

extern "C" size_t ec_distance_workspace_bytes(uint64_t cols, uint64_t rows) { return dist_workspace_bytes(cols, rows); }

extern "C" ec_status ec_distance(const uint8_t* mask, uint64_t cols, uint64_t rows, uint32_t max_sq, ec_dtype out_type, void* dst_or_null,
                                 uint8_t* dst_mask_or_null, void* workspace_dev_or_null, ec_stream stream) {
    const size_t out_size = out_type == EC_U32 ? 4 : out_type == EC_F64 ? 8 : 0;
    if (const ecv::Refusal r = distance_refusal(mask, cols, rows, ecl::valid(out_type), out_size, dst_or_null, dst_mask_or_null, workspace_dev_or_null))
        return refused(r, "ec_distance", "(%llu x %llu cells, out_type %d)", static_cast<unsigned long long>(cols), static_cast<unsigned long long>(rows),
                       int(out_type));
    const ec_status st = ensure_ready();
    if (st != EC_OK) return st;
    return with_workspace(workspace_dev_or_null, dist_workspace_bytes(cols, rows), stream, [&](void* workspace) {
        return launch_distance(mask, uint32_t(cols), uint32_t(rows), max_sq, int(out_type), dst_or_null, dst_mask_or_null, workspace, S(stream));
    });
}
