// ec_distance_line.hpp — the two line scans of ec_distance (include/erased_cells.h): the exact Euclidean distance transform of
// Meijster, Roerdink and Hesselink (2000), all in integers.
//
//   columns   g(y, x) = the distance along column x from (y, x) to the nearest target of that column, kDistInf if it has none:
//             distance_column_down then distance_column_up, over one column.
//   rows      d2(y, x) = min over the columns i with g(y, i) != kDistInf of (x - i)^2 + g(y, i)^2: the lower envelope of those
//             parabolas, built left to right on a stack (distance_row_forward) and read right to left (distance_row_backward).
//
// Both scans take plain pointers and strides and carry their state in a small struct, so a caller may run a line in pieces — the
// kernels (ec_distance_kernels.hpp) run a row tile by tile out of LDS — and get what one call over the whole line gives.  Every loop
// is bounded by a count the caller passes or by the stack's depth: a corrupt stack gives wrong cells, never a spin.
//
// Also here, because the host and the tests need them without a device: the launch constants, the layout of the workspace and the
// call's refusals (over ec_refusal.hpp).
//
// Self-contained like ec_focal_rank_cell.hpp and ec_order_key.hpp: no HIP runtime include; host/test_distance_line.cpp runs these
// very functions under a plain C++ compiler and the address and undefined-behaviour sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "ec_order_key.hpp"  // EC_HD
#include "ec_refusal.hpp"

#if defined(__clang__)
#define EC_DIST_UNROLL _Pragma("unroll")
#else
#define EC_DIST_UNROLL
#endif

namespace ecd {

constexpr uint32_t kDistMaxSide = 32768;   // EC_DISTANCE_MAX_SIDE
constexpr uint16_t kDistInf = 0xFFFF;      // g of a column without a target (a real g is at most kDistMaxSide - 1)
constexpr uint32_t kDistNone = 0xFFFFFFFFu;  // d2 of a row without a parabola: no target anywhere (a real d2 is below 2^31)
constexpr int kDistLines = 64;     // lines per wave: a lane owns a column (column kernel) or a row (row kernel); one wave per workgroup
constexpr int kDistTile = 64;      // side of the staging tiles of the row kernel: kDistLines rows by kDistTile columns
constexpr int kDistChunk = 8;      // rows whose loads a lane of the column kernel keeps in flight
constexpr int kDistGPitch = kDistTile + 2;   // u16 cells between two rows of the g tile in LDS: 33 dwords, odd, so the column-wise
                                             // reads of 32 lanes fall on 32 banks
constexpr int kDistDPitch = kDistTile + 1;   // u32 cells between two rows of the result tile: 65 dwords, likewise

// The workspace, in bytes from its 16-byte-aligned start:
//   g       cols * rows u16, row-major                                   at 0
//   s, t    the stacks of the row scans, u16 each: a wave of kDistLines rows has cols entries per row, entry q of the row of lane l
//           at [wave][q][l] — a push or a pop of the whole wave is one 128-byte access              at off_s and off_t
struct DistWorkspace {
    size_t off_s, off_t, bytes;
};
constexpr size_t dist_pad16(size_t b) { return (b + 15u) & ~size_t(15); }
constexpr bool dist_valid_side(uint64_t v) { return v >= 1 && v <= kDistMaxSide; }
constexpr size_t dist_waves(uint64_t lines) { return size_t((lines + kDistLines - 1) / kDistLines); }
constexpr DistWorkspace dist_workspace(uint64_t cols, uint64_t rows) {
    const size_t g = dist_pad16(size_t(cols) * size_t(rows) * 2u);
    const size_t stack = dist_pad16(dist_waves(rows) * size_t(kDistLines) * size_t(cols) * 2u);
    return DistWorkspace{g, g + stack, g + 2u * stack};
}
constexpr size_t dist_workspace_bytes(uint64_t cols, uint64_t rows) {
    return dist_valid_side(cols) && dist_valid_side(rows) ? dist_workspace(cols, rows).bytes : 0;
}

// ---- the refusals ------------------------------------------------------------------------------------------------------------
// Why ec_distance refuses a call, or nothing; the order is the header's, the overlaps output-major.  known_type: out_type is a
// cell type's code; out_size: 4 for EC_U32, 8 for EC_F64, 0 for every other.  Pointers are compared, never dereferenced.
inline ecv::Refusal distance_refusal(const void* mask, uint64_t cols, uint64_t rows, bool known_type, size_t out_size, const void* dst,
                                     const void* dst_mask, const void* workspace) {
    if (!dist_valid_side(cols) || !dist_valid_side(rows)) return {"cols and rows must be within 1 .. EC_DISTANCE_MAX_SIDE"};
    if (!known_type) return {"bad out_type", true};
    if (out_size == 0) return {"out_type is neither EC_U32 nor EC_F64"};
    if (!mask) return {"null mask"};
    if (!dst && !dst_mask) return {"dst and dst_mask are both NULL"};
    if (ecv::misaligned(dst, out_size)) return {"dst is not aligned to its cell type"};
    const size_t n = size_t(cols * rows);
    const ecv::Span in{mask, n}, out{dst, n * out_size}, out_mask{dst_mask, n}, work{workspace, dist_workspace_bytes(cols, rows)};
    const ecv::OverlapRow overlaps[] = {{out, in, "dst overlaps the mask"},
                                        {out_mask, in, "dst_mask overlaps the mask"},
                                        {work, in, "the workspace overlaps the mask"},
                                        {out, out_mask, "dst_mask overlaps dst"},
                                        {work, out, "the workspace overlaps dst"},
                                        {work, out_mask, "the workspace overlaps dst_mask"}};
    return {ecv::first_overlap(overlaps)};
}

// ---- columns -----------------------------------------------------------------------------------------------------------------
// One step of a sweep: the distance carried past a cell that is a target (0), or is none (one more, kDistInf staying kDistInf).
EC_HD uint32_t dist_carry(uint32_t d, bool target) { return target ? 0u : (d == kDistInf ? uint32_t(kDistInf) : d + 1u); }

// Down: g[y] = the distance to the nearest target at or above y in this column.  mask / g: the column's first cell; mstride /
// gstride: cells between two rows.  The loads of a chunk do not depend on the carry and are issued together.
EC_HD void distance_column_down(const uint8_t* mask, size_t mstride, uint32_t rows, uint16_t* g, size_t gstride) {
    uint32_t d = kDistInf;
    for (uint32_t y0 = 0; y0 < rows; y0 += kDistChunk) {
        uint8_t b[kDistChunk];
        EC_DIST_UNROLL
        for (int k = 0; k < kDistChunk; ++k) b[k] = y0 + uint32_t(k) < rows ? mask[size_t(y0 + k) * mstride] : uint8_t(0);
        EC_DIST_UNROLL
        for (int k = 0; k < kDistChunk; ++k) {
            if (y0 + uint32_t(k) < rows) {
                d = dist_carry(d, b[k] != 0);
                g[size_t(y0 + k) * gstride] = uint16_t(d);
            }
        }
    }
}

// Up: g[y] = min(g[y], the distance to the nearest target at or below y).  A target is where the down sweep left 0.
EC_HD void distance_column_up(uint16_t* g, size_t gstride, uint32_t rows) {
    uint32_t d = kDistInf;
    for (uint32_t done = 0; done < rows; done += kDistChunk) {
        const uint32_t top = rows - done;  // this chunk: rows top - 1, top - 2, ..
        uint16_t v[kDistChunk];
        EC_DIST_UNROLL
        for (int k = 0; k < kDistChunk; ++k) v[k] = uint32_t(k) < top ? g[size_t(top - 1 - k) * gstride] : kDistInf;
        EC_DIST_UNROLL
        for (int k = 0; k < kDistChunk; ++k) {
            if (uint32_t(k) < top) {
                d = dist_carry(d, v[k] == 0);
                if (d < v[k]) g[size_t(top - 1 - k) * gstride] = uint16_t(d);
            }
        }
    }
}

// ---- rows --------------------------------------------------------------------------------------------------------------------
// The stack of one row.  Entry q is the parabola of column s[q], the lowest of all from column t[q] on; t[0] == 0.  The entries
// live at S[q * qstride] and T[q * qstride]; the top one is also held here, so that a push stores and only a pop loads.
struct DistEnvelope {
    int32_t q = -1;    // index of the top entry, -1: empty
    uint32_t s = 0;    // top: its column,
    uint32_t t = 0;    //      where it starts to be the lowest,
    uint32_t g2 = 0;   //      g(s)^2
};

EC_HD uint32_t dist_f(uint32_t x, uint32_t i, uint32_t g2) {  // the parabola of column i at x: below 2^31
    const uint32_t dx = x > i ? x - i : i - x;
    return dx * dx + g2;
}

// the top entry from memory after q changed; grow: g of this row, one cell per column (grow[i * growstride])
EC_HD void dist_reload(DistEnvelope& e, const uint16_t* S, const uint16_t* T, size_t qstride, const uint16_t* grow, size_t growstride) {
    if (e.q < 0) return;
    e.s = S[size_t(e.q) * qstride];
    e.t = T[size_t(e.q) * qstride];
    const uint32_t g = grow[size_t(e.s) * growstride];
    e.g2 = g * g;
}

// Forward over the columns x0 .. x0 + n - 1 of a row of `cols` columns, g[k * gstride] being g of column x0 + k.
EC_HD void distance_row_forward(DistEnvelope& e, const uint16_t* g, size_t gstride, uint32_t x0, uint32_t n, uint32_t cols, uint16_t* S,
                                uint16_t* T, size_t qstride, const uint16_t* grow, size_t growstride) {
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t gu = g[size_t(k) * gstride];
        if (gu == kDistInf) continue;  // no parabola
        const uint32_t u = x0 + k, gu2 = gu * gu;
        while (e.q >= 0 && dist_f(e.t, e.s, e.g2) > dist_f(e.t, u, gu2)) {  // u is lower where the top starts: the top is nowhere lowest
            --e.q;
            dist_reload(e, S, T, qstride, grow, growstride);
        }
        uint32_t w = 0;
        if (e.q >= 0) {
            // the first column at which u is strictly lower than the top i: 1 + floor((u^2 - i^2 + g(u)^2 - g(i)^2) / (2 (u - i)));
            // the numerator is not negative after the pops
            const int64_t num = int64_t(u) * u - int64_t(e.s) * e.s + int64_t(gu2) - int64_t(e.g2);
            const int64_t sep = 1 + num / (2 * (int64_t(u) - int64_t(e.s)));
            if (sep >= int64_t(cols)) continue;  // never the lowest inside the row
            w = uint32_t(sep);
        }
        ++e.q;
        e.s = u;
        e.t = w;
        e.g2 = gu2;
        S[size_t(e.q) * qstride] = uint16_t(u);
        T[size_t(e.q) * qstride] = uint16_t(w);
    }
}

// Backward over the columns x0 + n - 1 .. x0: out[k * ostride] = d2 of column x0 + k, kDistNone on an empty stack.  The pieces of a
// row come in descending x0.
EC_HD void distance_row_backward(DistEnvelope& e, uint32_t x0, uint32_t n, uint32_t* out, size_t ostride, const uint16_t* S, const uint16_t* T,
                                 size_t qstride, const uint16_t* grow, size_t growstride) {
    for (uint32_t k = n; k-- > 0;) {
        const uint32_t u = x0 + k;
        if (e.q < 0) {
            out[size_t(k) * ostride] = kDistNone;
            continue;
        }
        out[size_t(k) * ostride] = dist_f(u, e.s, e.g2);
        if (u == e.t) {
            --e.q;
            dist_reload(e, S, T, qstride, grow, growstride);
        }
    }
}

// ---- the cell as it is stored --------------------------------------------------------------------------------------------------
EC_HD bool dist_valid(uint32_t d2, uint32_t max_sq) { return d2 != kDistNone && d2 <= max_sq; }

}  // namespace ecd
