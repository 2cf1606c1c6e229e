// ec_regions.hip — ec_regions and ec_regions_workspace_bytes (include/erased_cells.h): connected-component labels and the sieve of a
// raster.  The refusals and their order (before any device work and before the library asks for a device), the workspace — the
// caller's, or a block of the library's stream-ordered pool that goes back on the same stream — and the launches: tiles, seams,
// flatten and count, then as far as the call needs them the block sums, their scan, the dense numbers and the store
// (ec_regions_kernels.hpp over ec_regions_cell.hpp).
#include <hip/hip_runtime.h>

#include "ec_dispatch.hpp"
#include "ec_lattice.hpp"
#include "ec_regions_kernels.hpp"
#include "ec_runtime.hpp"

namespace ecd {

static_assert(EC_REGIONS_MAX_SIDE == kRegMaxSide, "ec_regions_cell.hpp restates the C ABI's limit");

static bool reg_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
    if (!a || !b || abytes == 0 || bbytes == 0) return false;
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bbytes && y < x + abytes;
}

// Why ec_regions refuses a call, or null; the order is the header's.  *bad_type: EC_ERR_UNSUPPORTED_TYPE, else EC_ERR_ARG.
static const char* regions_refusal(int t, const void* src, const uint8_t* src_mask, uint64_t cols, uint64_t rows, int32_t connectivity,
                                   int32_t numbering, const void* dst, const uint8_t* dst_mask, const void* n_regions, const void* workspace,
                                   bool* bad_type) {
    *bad_type = false;
    if (!reg_valid_side(cols) || !reg_valid_side(rows)) return "cols and rows must be within 1 .. EC_REGIONS_MAX_SIDE";
    if (src && !ecl::valid(t)) {
        *bad_type = true;
        return "bad cell type";
    }
    if (connectivity != 4 && connectivity != 8) return "connectivity is neither 4 nor 8";
    if (numbering != EC_REGIONS_ROOT && numbering != EC_REGIONS_DENSE) return "numbering is neither EC_REGIONS_ROOT nor EC_REGIONS_DENSE";
    if (!src && !src_mask) return "src and src_mask are both NULL";
    if (!dst && !dst_mask && !n_regions) return "dst, dst_mask and n_regions are all NULL";
    const size_t cell = src ? ecl::size_of(t) : 1, n = size_t(cols * rows), ws = reg_workspace_bytes(cols, rows);
    if (reinterpret_cast<uintptr_t>(src) % cell != 0) return "src is not aligned to its cell type";
    if (reinterpret_cast<uintptr_t>(dst) % 4 != 0) return "dst is not aligned to its cell type";
    if (reinterpret_cast<uintptr_t>(n_regions) % 8 != 0) return "n_regions is not aligned to 8 bytes";
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return "the workspace is not aligned to 16 bytes";
    struct Span {
        const void* p;
        size_t bytes;
        const char* on_src;
        const char* on_mask;
    };
    const Span outs[] = {{dst, n * 4, "dst overlaps src", "dst overlaps src_mask"},
                         {dst_mask, n, "dst_mask overlaps src", "dst_mask overlaps src_mask"},
                         {n_regions, 8, "n_regions overlaps src", "n_regions overlaps src_mask"},
                         {workspace, ws, "the workspace overlaps src", "the workspace overlaps src_mask"}};
    for (const Span& o : outs) {
        if (reg_overlap(o.p, o.bytes, src, n * cell)) return o.on_src;
        if (reg_overlap(o.p, o.bytes, src_mask, n)) return o.on_mask;
    }
    if (reg_overlap(dst, n * 4, dst_mask, n)) return "dst_mask overlaps dst";
    if (reg_overlap(n_regions, 8, dst, n * 4)) return "n_regions overlaps dst";
    if (reg_overlap(n_regions, 8, dst_mask, n)) return "n_regions overlaps dst_mask";
    if (reg_overlap(workspace, ws, dst, n * 4)) return "the workspace overlaps dst";
    if (reg_overlap(workspace, ws, dst_mask, n)) return "the workspace overlaps dst_mask";
    if (reg_overlap(workspace, ws, n_regions, 8)) return "the workspace overlaps n_regions";
    return nullptr;
}

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
    bool bad_type = false;
    if (const char* why = regions_refusal(int(t), src_or_null, src_mask_or_null, cols, rows, connectivity, numbering, dst_or_null, dst_mask_or_null,
                                          n_regions_dev_or_null, workspace_dev_or_null, &bad_type))
        return set_error(bad_type ? EC_ERR_UNSUPPORTED_TYPE : EC_ERR_ARG, "ec_regions: %s (%llu x %llu cells, dtype %d, connectivity %d, numbering %d)", why,
                         static_cast<unsigned long long>(cols), static_cast<unsigned long long>(rows), int(t), int(connectivity), int(numbering));
    ec_status st = ensure_ready();
    if (st != EC_OK) return st;
    const RegCall call{src_or_null, src_mask_or_null, uint32_t(cols), uint32_t(rows), connectivity == 8, numbering == EC_REGIONS_DENSE,
                       min_cells > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(min_cells), dst_or_null, dst_mask_or_null, n_regions_dev_or_null};
    if (workspace_dev_or_null) return dispatch_regions(int(t), call, workspace_dev_or_null, S(stream));
    void* block = nullptr;  // from the pool, and back to it behind the kernels on the same stream: the call stays asynchronous
    if ((st = ec_alloc_async(&block, reg_workspace_bytes(cols, rows), stream)) != EC_OK) return st;
    st = dispatch_regions(int(t), call, block, S(stream));
    const ec_status freed = ec_free_async(block, stream);
    return st != EC_OK ? st : freed;
}
