// ec_regions_cell.hpp — what one cell does in each phase of ec_regions (include/erased_cells.h): connected-component labelling by
// union-find after Komura (2015) and Playne & Hawick (2018).
//
//   parent[]   one u32 per cell.  parent[i] <= i AT ALL TIMES, and parent[i] is a cell of i's region; a cell with parent[i] == i is a
//              root.  Every chain i, parent[i], parent[parent[i]], .. therefore strictly decreases and ends at a root.  Only a
//              root's entry is lowered by a join (reg_unite), to a cell of a region that is being joined to it, and any other only to a cell
//              above it in its chain (reg_find), so the least cell of a region is a root from the first phase to the last: when all unions are done it is the only one — the rule's ROOT.
//   tiles      a tile of tile_w x tile_h cells is labelled on its own (reg_tile_links: the joins of a cell to its left and upper
//              neighbours INSIDE the tile), which leaves parent[i] = the least cell of i's piece of the tile.
//   seams      the cells of a tile's last column and last row then join across the tile's right and lower edge (reg_seam_unite).
//              This is the one phase in which workgroups meet, and reg_unite's argument is written at it.
//   flatten, count, number, store   per cell; reg_label is the cell as it is stored.
//
// The accesses to parent[] go through a policy P — P::load(i), P::fetch_min(i, v) returning the value before, P::lower(i, v) — so the same
// functions run on LDS words (tiles), on agent-scope atomics (seams), on plain loads (after the seams) and, in
// host/test_regions_cell.cpp, on plain words and on std::atomic under threads.  Every loop counts its steps for that program; the
// kernels drop the counts.
//
// Also here, because the host and the tests need them without a device: the launch constants, the layout of the workspace and the
// call's refusals (over ec_refusal.hpp).
//
// Self-contained like ec_distance_line.hpp: no HIP runtime include.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "ec_order_key.hpp"  // EC_HD
#include "ec_refusal.hpp"

namespace ecd {

constexpr uint32_t kRegMaxSide = 32768;  // EC_REGIONS_MAX_SIDE: cols * rows <= 2^30, so a cell index, a size and a label fit a u32
constexpr int kRegTileW = 32;            // a tile: one workgroup of the tile kernel, kRegTileW x kRegTileH cells
constexpr int kRegTileH = 32;
constexpr int kRegThreads = 256;         // lanes of a workgroup of every kernel but the seams'
constexpr int kRegSeamLanes = 64;        // the seam kernel: one wave per tile, a lane per cell of its last row and last column
constexpr int kRegScanCells = 2048;      // cells per workgroup of the two kernels that count and number roots: 8 a lane
constexpr uint32_t kRegLinkW = 1, kRegLinkN = 2, kRegLinkNW = 4, kRegLinkNE = 8;  // reg_tile_links

static_assert(kRegTileW + kRegTileH - 1 <= kRegSeamLanes, "a lane per border cell");
static_assert(kRegScanCells % kRegThreads == 0, "whole cells per lane");

// The workspace, in bytes from its 16-byte-aligned start:
//   parent   cols * rows u32                                                                          at 0
//   count    cols * rows u32: at a root the region's size, later its dense number (0: dropped)         at off_count
//   sums     one u32 per kRegScanCells cells: kept roots of that block, then their exclusive scan      at off_sums
struct RegWorkspace {
    size_t off_count, off_sums, bytes;
};
constexpr size_t reg_pad16(size_t b) { return (b + 15u) & ~size_t(15); }
constexpr bool reg_valid_side(uint64_t v) { return v >= 1 && v <= kRegMaxSide; }
constexpr size_t reg_tiles(uint64_t side, int tile) { return size_t((side + uint64_t(tile) - 1) / uint64_t(tile)); }
constexpr size_t reg_scan_blocks(uint64_t n) { return size_t((n + kRegScanCells - 1) / kRegScanCells); }
constexpr RegWorkspace reg_workspace(uint64_t cols, uint64_t rows) {
    const size_t plane = reg_pad16(size_t(cols) * size_t(rows) * 4u);
    return RegWorkspace{plane, 2u * plane, 2u * plane + reg_pad16(reg_scan_blocks(cols * rows) * 4u)};
}
constexpr size_t reg_workspace_bytes(uint64_t cols, uint64_t rows) {
    return reg_valid_side(cols) && reg_valid_side(rows) ? reg_workspace(cols, rows).bytes : 0;
}

// ---- the refusals ---------------------------------------------------------------------------------------------------------------
// Why ec_regions refuses a call, or nothing; the order is the header's, the overlaps output-major.  cell_size: bytes of a cell of
// src's type, 0 for a bad code (looked at only with a src); known_numbering: it is one of the two.  Pointers are compared, never dereferenced.
inline ecv::Refusal regions_refusal(size_t cell_size, const void* src, const void* src_mask, uint64_t cols, uint64_t rows, int32_t connectivity,
                                    bool known_numbering, const void* dst, const void* dst_mask, const void* n_regions, const void* workspace) {
    if (!reg_valid_side(cols) || !reg_valid_side(rows)) return {"cols and rows must be within 1 .. EC_REGIONS_MAX_SIDE"};
    if (src && cell_size == 0) return {"bad cell type", true};
    if (connectivity != 4 && connectivity != 8) return {"connectivity is neither 4 nor 8"};
    if (!known_numbering) return {"numbering is neither EC_REGIONS_ROOT nor EC_REGIONS_DENSE"};
    if (!src && !src_mask) return {"src and src_mask are both NULL"};
    if (!dst && !dst_mask && !n_regions) return {"dst, dst_mask and n_regions are all NULL"};
    if (ecv::misaligned(src, src ? cell_size : 1)) return {"src is not aligned to its cell type"};
    if (ecv::misaligned(dst, 4)) return {"dst is not aligned to its cell type"};
    if (ecv::misaligned(n_regions, 8)) return {"n_regions is not aligned to 8 bytes"};
    if (ecv::misaligned(workspace, 16)) return {"the workspace is not aligned to 16 bytes"};
    const size_t n = size_t(cols * rows);
    const ecv::Span cells{src, n * cell_size}, valid{src_mask, n}, out{dst, n * 4}, out_mask{dst_mask, n}, count{n_regions, 8},
        work{workspace, reg_workspace_bytes(cols, rows)};
    const ecv::OverlapRow overlaps[] = {{out, cells, "dst overlaps src"},
                                       {out, valid, "dst overlaps src_mask"},
                                       {out_mask, cells, "dst_mask overlaps src"},
                                       {out_mask, valid, "dst_mask overlaps src_mask"},
                                       {count, cells, "n_regions overlaps src"},
                                       {count, valid, "n_regions overlaps src_mask"},
                                       {work, cells, "the workspace overlaps src"},
                                       {work, valid, "the workspace overlaps src_mask"},
                                       {out, out_mask, "dst_mask overlaps dst"},
                                       {count, out, "n_regions overlaps dst"},
                                       {count, out_mask, "n_regions overlaps dst_mask"},
                                       {work, out, "the workspace overlaps dst"},
                                       {work, out_mask, "the workspace overlaps dst_mask"},
                                       {work, count, "the workspace overlaps n_regions"}};
    return {ecv::first_overlap(overlaps)};
}

// ---- the raster -----------------------------------------------------------------------------------------------------------------
// W: the unsigned word of the cell's width — equality is equality of bits.  src == nullptr: the mask form, every valid cell equal.
template <typename W>
struct RegRaster {
    const W* src;
    const uint8_t* mask;
    uint32_t cols, rows;
    EC_HD bool valid(size_t i) const { return !mask || mask[i] != 0; }
    EC_HD bool joined(size_t i, size_t j) const { return valid(i) && valid(j) && (!src || src[i] == src[j]); }  // i, j: neighbours
};

// ---- union-find -----------------------------------------------------------------------------------------------------------------
// The root above i as far as the loads show it.  The index strictly decreases (a value that does not is taken for a root, so that a
// corrupt array gives wrong cells, never a spin): at most i + 1 steps of two loads.  A stale load returns an EARLIER parent[i]: still a
// cell of the region and still <= i, so the result is a cell of i's region that was a root at some time — not necessarily now.
// On the way every entry passed is lowered to its grandparent (P::lower: a fetch_min, or nothing where the words are read-only), so
// that the chains the seams build over many tiles stay short for the lanes that come after.  That touches no root — an entry seen
// below its index never is one again — and keeps the chain's cells joined: the grandparent was above the parent when it was loaded.
template <typename P>
EC_HD uint32_t reg_find(P& p, uint32_t i, uint32_t& loads) {
    for (;;) {
        const uint32_t up = p.load(i);
        ++loads;
        if (up >= i) return i;
        const uint32_t over = p.load(up);
        ++loads;
        if (over < up) p.lower(i, over);
        i = up;
    }
}

// Join the regions of a and b.  Playne & Hawick's loop: find both roots; lower the larger root's entry to the smaller with ONE
// fetch_min; what the fetch_min RETURNS decides.
//   old == b   b was a root at that instant and now hangs under a: joined.
//   old <  b   b was no root any more — the find was stale, or another lane won.  parent[b] is now min(old, a).  Where that is a,
//              the link b -> old has just been overwritten, and where it is still old, a has no link yet: in both cases `a` and
//              `old` must still be joined, and this lane owes it.  So it goes on with (a, old).
// Correctness rests only on these returned values: every link that was ever written and then overwritten left its overwriter
// with the duty to restore it between smaller cells, the duties end (below), and when all lanes have returned, the chains hold
// every join that was asked for.  A stale load in reg_find costs a further round, never an answer.
// Termination: a round that does not return replaces a or b by a smaller cell (a find never goes up; old < b), so a + b strictly
// decreases: at most a + b + 1 rounds, whatever other lanes do.  No lane waits for another.
// Returns its rounds.
template <typename P>
EC_HD uint32_t reg_unite(P& p, uint32_t a, uint32_t b, uint32_t& loads) {
    uint32_t rounds = 0;
    for (;;) {
        ++rounds;
        a = reg_find(p, a, loads);
        b = reg_find(p, b, loads);
        if (a == b) return rounds;
        if (a > b) {
            const uint32_t s = a;
            a = b;
            b = s;
        }
        const uint32_t old = p.fetch_min(b, a);
        if (old >= b) return rounds;  // == b; above it only in a corrupt array
        b = old;
    }
}
constexpr uint64_t reg_find_bound(uint32_t i) { return 2 * (uint64_t(i) + 1); }  // loads
constexpr uint64_t reg_unite_bound(uint32_t a, uint32_t b) { return uint64_t(a) + uint64_t(b) + 1; }

// ---- tiles ----------------------------------------------------------------------------------------------------------------------
// The joins of cell (y, x) to its left, upper, upper-left and upper-right neighbour where that neighbour lies in the SAME tile.
// Every pair of neighbours inside a tile is the link of exactly one of its two cells.
template <typename W>
EC_HD uint32_t reg_tile_links(const RegRaster<W>& r, uint32_t y, uint32_t x, uint32_t tile_w, uint32_t tile_h, bool eight) {
    const size_t i = size_t(y) * r.cols + x;
    if (!r.valid(i)) return 0;
    const bool left = x % tile_w != 0, up = y % tile_h != 0, right = (x + 1) % tile_w != 0 && x + 1 < r.cols;
    uint32_t links = 0;
    if (left && r.joined(i, i - 1)) links |= kRegLinkW;
    if (up && r.joined(i, i - r.cols)) links |= kRegLinkN;
    if (eight && up && left && r.joined(i, i - r.cols - 1)) links |= kRegLinkNW;
    if (eight && up && right && r.joined(i, i - r.cols + 1)) links |= kRegLinkNE;
    return links;
}

// ---- seams ----------------------------------------------------------------------------------------------------------------------
// Cell (y, x) of a tile's last column or last row joins across the seams it touches.  A pair of neighbours in different tiles:
//   side by side, or one below the other        the left / upper cell is on its tile's last column / row and makes the join;
//   diagonal (y, x) - (y + 1, x + 1)            crosses a seam iff (y, x) is on a last column or a last row: (y, x) makes it —
//                                               into the tile to the right, below, or the CORNER tile;
//   anti-diagonal (y, x) - (y + 1, x - 1)       crosses iff y is a last row — (y, x) makes it, downwards — or x - 1 is a last
//                                               column: then (y + 1, x - 1) makes it, upwards.  (Both where both hold: harmless.)
// Returns the most rounds one of its joins took.
template <typename P, typename W>
EC_HD uint32_t reg_seam_unite(P& p, const RegRaster<W>& r, uint32_t y, uint32_t x, uint32_t tile_w, uint32_t tile_h, bool eight,
                              uint32_t& loads) {
    const uint32_t cols = r.cols;
    const bool has_right = x + 1 < cols, has_below = y + 1 < r.rows;
    const bool right = (x + 1) % tile_w == 0 && has_right;   // a seam to the right of this cell
    const bool below = (y + 1) % tile_h == 0 && has_below;   // a seam below it
    const uint32_t i = y * cols + x;
    if (!(right || below) || !r.valid(i)) return 0;
    uint32_t most = 0;
    auto join = [&](uint32_t j) {
        if (!r.joined(i, j)) return;
        const uint32_t rounds = reg_unite(p, i, j, loads);
        most = rounds > most ? rounds : most;
    };
    if (right) join(i + 1);
    if (below) join(i + cols);
    if (eight) {
        if (has_right && has_below) join(i + cols + 1);
        if (below && x > 0) join(i + cols - 1);
        if (right && y > 0) join(i - cols + 1);
    }
    return most;
}

// ---- the cell as it is stored ---------------------------------------------------------------------------------------------------
// size: the region's cell count (any value where need <= 1); need: min_cells clamped to a u32 (no region has 2^32 cells)
EC_HD bool reg_kept(uint32_t size, uint32_t need) { return need <= 1 || size >= need; }
// at_root: the region's size (root numbering) or its dense number, 0 for a dropped region (dense numbering).  0: no region.
EC_HD uint32_t reg_label(bool valid, uint32_t root, uint32_t at_root, bool dense, uint32_t need) {
    if (!valid) return 0;
    if (dense) return at_root;
    return reg_kept(at_root, need) ? root + 1 : 0;
}

}  // namespace ecd
