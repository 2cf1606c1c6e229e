// ec_distance.hip — ec_distance and ec_distance_workspace_bytes (include/erased_cells.h): the exact Euclidean distance transform of
// a mask.  The refusals and their order (before any device work and before the library asks for a device), the workspace — the
// caller's, or a block of the library's stream-ordered pool that goes back on the same stream — and the two launches: the column
// sweeps, then the row scans (ec_distance_kernels.hpp over ec_distance_line.hpp).
#include <hip/hip_runtime.h>

#include "ec_distance_kernels.hpp"
#include "ec_lattice.hpp"
#include "ec_runtime.hpp"

namespace ecd {

static_assert(EC_DISTANCE_MAX_SIDE == kDistMaxSide, "ec_distance_line.hpp restates the C ABI's limit");
static_assert(EC_DISTANCE_UNLIMITED == kDistNone, "no d2 reaches the sentinel, so UNLIMITED admits every real one");

static bool dist_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
    if (!a || !b || abytes == 0 || bbytes == 0) return false;
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bbytes && y < x + abytes;
}

// Why ec_distance refuses a call, or null; the order is the header's.  *bad_type: EC_ERR_UNSUPPORTED_TYPE, else EC_ERR_ARG.
static const char* distance_refusal(const uint8_t* mask, uint64_t cols, uint64_t rows, int out_type, const void* dst, const uint8_t* dst_mask,
                                    const void* workspace, bool* bad_type) {
    *bad_type = false;
    if (!dist_valid_side(cols) || !dist_valid_side(rows)) return "cols and rows must be within 1 .. EC_DISTANCE_MAX_SIDE";
    if (!ecl::valid(out_type)) {
        *bad_type = true;
        return "bad out_type";
    }
    if (out_type != EC_U32 && out_type != EC_F64) return "out_type is neither EC_U32 nor EC_F64";
    if (!mask) return "null mask";
    if (!dst && !dst_mask) return "dst and dst_mask are both NULL";
    const size_t cell = out_type == EC_U32 ? 4 : 8, n = size_t(cols * rows), ws = dist_workspace_bytes(cols, rows);
    if (reinterpret_cast<uintptr_t>(dst) % cell != 0) return "dst is not aligned to its cell type";
    if (dist_overlap(dst, n * cell, mask, n)) return "dst overlaps the mask";
    if (dist_overlap(dst_mask, n, mask, n)) return "dst_mask overlaps the mask";
    if (dist_overlap(workspace, ws, mask, n)) return "the workspace overlaps the mask";
    if (dist_overlap(dst, n * cell, dst_mask, n)) return "dst_mask overlaps dst";
    if (dist_overlap(workspace, ws, dst, n * cell)) return "the workspace overlaps dst";
    if (dist_overlap(workspace, ws, dst_mask, n)) return "the workspace overlaps dst_mask";
    return nullptr;
}

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
    bool bad_type = false;
    if (const char* why = distance_refusal(mask, cols, rows, int(out_type), dst_or_null, dst_mask_or_null, workspace_dev_or_null, &bad_type))
        return set_error(bad_type ? EC_ERR_UNSUPPORTED_TYPE : EC_ERR_ARG, "ec_distance: %s (%llu x %llu cells, out_type %d)", why,
                         static_cast<unsigned long long>(cols), static_cast<unsigned long long>(rows), int(out_type));
    ec_status st = ensure_ready();
    if (st != EC_OK) return st;
    if (workspace_dev_or_null)
        return launch_distance(mask, uint32_t(cols), uint32_t(rows), max_sq, int(out_type), dst_or_null, dst_mask_or_null, workspace_dev_or_null, S(stream));
    void* block = nullptr;  // from the pool, and back to it behind the two kernels on the same stream: the call stays asynchronous
    if ((st = ec_alloc_async(&block, dist_workspace_bytes(cols, rows), stream)) != EC_OK) return st;
    st = launch_distance(mask, uint32_t(cols), uint32_t(rows), max_sq, int(out_type), dst_or_null, dst_mask_or_null, block, S(stream));
    const ec_status freed = ec_free_async(block, stream);
    return st != EC_OK ? st : freed;
}
