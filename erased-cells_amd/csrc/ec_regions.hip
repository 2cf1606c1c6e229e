// ec_regions.hip — ec_regions and ec_regions_workspace_bytes (include/erased_cells.h): connected-component labels and the sieve of a
// raster.  The refusals (regions_refusal, ec_regions_cell.hpp: before any device work and before the library asks for a device), the
// workspace — the caller's, or a block of the library's stream-ordered pool that goes back on the same stream — and the launches: tiles, seams,
// flatten and count, then as far as the call needs them the block sums, their scan, the dense numbers and the store
// (ec_regions_kernels.hpp over ec_regions_cell.hpp).
#include <hip/hip_runtime.h>

#include "ec_dispatch.hpp"
#include "ec_lattice.hpp"
#include "ec_regions_kernels.hpp"
#include "ec_runtime.hpp"

namespace ecd {

static_assert(EC_REGIONS_MAX_SIDE == kRegMaxSide, "ec_regions_cell.hpp restates the C ABI's limit");

struct RegCall {
    const void* src;
    const uint8_t* src_mask;
    uint32_t cols, rows;
    bool eight, dense;
    uint32_t need;  // min_cells as a u32: no region has 2^32 cells
    int32_t* dst;
    uint8_t* dst_mask;
    uint64_t* n_regions;
};

template <typename W>
static ec_status launch_regions(const RegCall& c, void* workspace, hipStream_t st) {
    const RegWorkspace w = reg_workspace(c.cols, c.rows);
    char* base = static_cast<char*>(workspace);
    uint32_t* parent = reinterpret_cast<uint32_t*>(base);
    uint32_t* count = reinterpret_cast<uint32_t*>(base + w.off_count);
    uint32_t* sums = reinterpret_cast<uint32_t*>(base + w.off_sums);
    uint32_t* sizes = c.need > 1 ? count : nullptr;  // without a sieve no size is counted
    const RegRaster<W> r{static_cast<const W*>(c.src), c.src_mask, c.cols, c.rows};
    const uint32_t n = c.cols * c.rows, tiles_x = uint32_t(reg_tiles(c.cols, kRegTileW));
    const unsigned tiles = unsigned(tiles_x * reg_tiles(c.rows, kRegTileH));
    const unsigned per_cell = unsigned((n + kRegThreads - 1) / kRegThreads), blocks = unsigned(reg_scan_blocks(n));
    ec_status e;
    k_regions_tiles<W><<<tiles, kRegThreads, 0, st>>>(r, tiles_x, c.eight, parent, sizes);
    if ((e = check_launch("regions(tiles)")) != EC_OK) return e;
    if (tiles > 1) {
        k_regions_seams<W><<<tiles, kRegSeamLanes, 0, st>>>(r, tiles_x, c.eight, parent);
        if ((e = check_launch("regions(seams)")) != EC_OK) return e;
    }
    k_regions_flatten<<<per_cell, kRegThreads, 0, st>>>(c.src_mask, n, parent, sizes);
    if ((e = check_launch("regions(flatten)")) != EC_OK) return e;
    if (c.dense || c.n_regions) {
        k_regions_sums<<<blocks, kRegThreads, 0, st>>>(c.src_mask, parent, count, n, c.need, sums);
        if ((e = check_launch("regions(sums)")) != EC_OK) return e;
        k_regions_scan<<<1, kRegThreads, 0, st>>>(sums, blocks, c.n_regions);
        if ((e = check_launch("regions(scan)")) != EC_OK) return e;
    }
    if (!c.dst && !c.dst_mask) return EC_OK;
    const bool numbered = c.dense && c.dst;  // the sieve-only form asks "kept", not "which"
    if (numbered) {
        k_regions_number<<<blocks, kRegThreads, 0, st>>>(c.src_mask, parent, count, n, c.need, sums);
        if ((e = check_launch("regions(number)")) != EC_OK) return e;
    }
    const unsigned quads = unsigned((size_t(n) + 4u * kRegThreads - 1) / (4u * kRegThreads));
    if (c.dst && c.dst_mask) k_regions_store<true, true><<<quads, kRegThreads, 0, st>>>(c.src_mask, parent, count, n, numbered, c.need, c.dst, c.dst_mask);
    else if (c.dst) k_regions_store<true, false><<<quads, kRegThreads, 0, st>>>(c.src_mask, parent, count, n, numbered, c.need, c.dst, c.dst_mask);
    else k_regions_store<false, true><<<quads, kRegThreads, 0, st>>>(c.src_mask, parent, count, n, numbered, c.need, c.dst, c.dst_mask);
    return check_launch("regions(store)");
}

static ec_status dispatch_regions(int t, const RegCall& c, void* workspace, hipStream_t st) {
    return ecl::with_cell_width(c.src ? ecl::size_of(t) : 1, [&](auto w) { return launch_regions<ecl::cell_t<decltype(w)>>(c, workspace, st); }, kTypeChecked);
}

}  // namespace ecd

using namespace ecd;

extern "C" size_t ec_regions_workspace_bytes(uint64_t cols, uint64_t rows) { return reg_workspace_bytes(cols, rows); }

extern "C" ec_status ec_regions(ec_dtype t, const void* src_or_null, const uint8_t* src_mask_or_null, uint64_t cols, uint64_t rows, int32_t connectivity,
                                int32_t numbering, uint64_t min_cells, int32_t* dst_or_null, uint8_t* dst_mask_or_null, uint64_t* n_regions_dev_or_null,
                                void* workspace_dev_or_null, ec_stream stream) {
    const bool known_numbering = numbering == EC_REGIONS_ROOT || numbering == EC_REGIONS_DENSE;
    if (const ecv::Refusal r = regions_refusal(ecl::size_of(t), src_or_null, src_mask_or_null, cols, rows, connectivity, known_numbering, dst_or_null,
                                               dst_mask_or_null, n_regions_dev_or_null, workspace_dev_or_null))
        return refused(r, "ec_regions", "(%llu x %llu cells, dtype %d, connectivity %d, numbering %d)", static_cast<unsigned long long>(cols),
                       static_cast<unsigned long long>(rows), int(t), int(connectivity), int(numbering));
    const ec_status st = ensure_ready();
    if (st != EC_OK) return st;
    const RegCall call{src_or_null, src_mask_or_null, uint32_t(cols), uint32_t(rows), connectivity == 8, numbering == EC_REGIONS_DENSE,
                       min_cells > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(min_cells), dst_or_null, dst_mask_or_null, n_regions_dev_or_null};
    return with_workspace(workspace_dev_or_null, reg_workspace_bytes(cols, rows), stream,
                          [&](void* workspace) { return dispatch_regions(int(t), call, workspace, S(stream)); });
}
