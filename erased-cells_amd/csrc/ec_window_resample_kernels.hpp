// ec_window_resample_kernels.hpp — a window of a raster resident in HBM, cut out at another size by AVERAGE or BILINEAR resampling
// (gfx950): k_window_resample<T, MASKED>, beside k_window_nearest (ec_window_kernels.hpp).  Unlike the copies there it does arithmetic,
// so it is typed by cell TYPE.  The rule is the one stated at ec_window_resample in include/erased_cells.h: integer weights, individually
// rounded f64 steps in a fixed order (the translation unit is built with -ffp-contract=off: no FMA), one right answer per cell.
//
// ONE BODY FOR BOTH ALGORITHMS.  Along one axis an output index j owns a run of `total` weight units that starts `f` units into window
// cell `c` and is cut at every cell border, `den` units per cell:
//     average   (win, out divided by their gcd)  den = out,      total = win,      c * den + f = j * win
//     bilinear                                   den = 2 * out,  total = 2 * out,  c * den + f = (2 j + 1) * win + out,  cells shifted by -1
// so the taps are (c, min(den - f, total)), (c + 1, ...), ... until `total` is spent: the overlaps of an average, and for bilinear
// (k - 1, 2 out - f), (k, f) with the second tap absent when f = 0.  Cells are clamped into the window (a no-op for the average).  The
// host fills ResampleAxis; the kernel never learns which algorithm it runs.  From j to j + 1 the run start moves by `num` units = q cells
// and r units, so a lane divides once per axis for its slot's first cell and steps the others (tap_at / tap_step, as axis_at / axis_step).
//
// OUTPUT SIDE: the shape of the other window kernels — 256-thread workgroups, one workgroup per tile of kWindowTileSlots 16-byte
// value slots, two fronts, the lane map and the row-end cursor of ec_window_kernels.hpp (lane_row_col, RowCursor), nt_store for a whole
// value slot, cell-wise stores for the last partial slot.  The mask byte of an output cell is a by-product of its value (wsum != 0), so
// the lane that owns a value slot also owns the 16 / W mask bytes of the same cells and writes them as ONE mask_store of that width
// (16, 8, 4, 2 bytes: neighbouring lanes write neighbouring bytes) — SlotMask and slot_store_pair of ec_tile.hpp, which the focal
// kernels end their slots with too; a lane map of its own for the mask stream, as the copies have, would walk every footprint twice.
// SOURCE SIDE: cell loads under the launch's cache_plan bits.  A footprint row is a run of at most 65 cells and neighbouring lanes' runs
// are neighbours or overlap, so a line is wanted several times within a workgroup; whether it stays cacheable is the host's call.
// Slots and cells are walked by loops that are NOT unrolled, so that the code stays small (ten types x masked or not x the policy arms);
// what that costs beside a cell's taps (up to 65 x 65 of them) is not measured.  First timings of tools/window_bench.py rows (f)-(h):
// profiles/window/frame.md; what bounds the kernel is not looked into there.
#pragma once

#include "ec_cast_cell.hpp"
#include "ec_window_kernels.hpp"

namespace ecd {

struct ResampleAxis {
    uint64_t num, add;  // run start of output index j, in units: j * num + add
    uint64_t den;       // units per window cell
    uint64_t total;     // units per output index (the axis weight of a footprint)
    uint64_t bias;      // cells the run is shifted towards the origin (bilinear: 1)
    uint64_t last;      // win - 1: cells are clamped into [0, last]
    uint64_t q, r;      // num = q * den + r
    uint64_t c0, f0;    // the state at j = 0
};
struct TapPos {
    uint64_t c, f;
};
__device__ __forceinline__ TapPos tap_at(const ResampleAxis& a, uint64_t j) {
    const uint64_t t = j * a.num + a.add, c = t / a.den;  // no overflow: checked by the host
    return TapPos{c, t - c * a.den};
}
__device__ __forceinline__ TapPos tap_first(const ResampleAxis& a) { return TapPos{a.c0, a.f0}; }
__device__ __forceinline__ void tap_step(const ResampleAxis& a, TapPos& p) {
    p.c += a.q;
    p.f += a.r;
    if (p.f >= a.den) {
        p.f -= a.den;
        ++p.c;
    }
}
__device__ __forceinline__ uint64_t tap_cell(const ResampleAxis& a, uint64_t c) {
    const uint64_t s = c < a.bias ? 0 : c - a.bias;
    return s < a.last ? s : a.last;
}

// r as a cell of type T: f64 as it is, f32 rounded to nearest even, integers rounded half away from zero by ONE f64 add and a
// truncation, then saturated as Rust's `as` saturates (the 64-bit types compare in f64 before the cast): round_cell, the one
// definition of the rule (ec_cast_cell.hpp), which ec_cast's EC_CAST_ROUND shares.
template <typename T>
__device__ __forceinline__ T resample_cell_of(double r) { return round_cell<T>(r); }

template <bool NT, typename T>
__device__ __forceinline__ T resample_load(const T* p) {
    if constexpr (NT) return ld_cell(p);
    else return *p;
}

// One output cell: the footprint whose first taps are x and y, rows outer, columns inner, both ascending.  *valid: its weight is not 0.
// BITS: the launch's load policy (bit 0 = values cacheable, bit 1 = mask bytes cacheable).  A masked-out cell is loaded and not used:
// the select keeps the lanes of a wave together, and what the cell holds — a NaN included — leaves no trace.
template <typename T, bool MASKED, unsigned BITS>
__device__ __forceinline__ T resample_footprint(const T* __restrict__ win, const uint8_t* __restrict__ mwin, uint64_t pitch,
                                                const ResampleAxis& ax, const ResampleAxis& ay, TapPos x, TapPos y, bool* valid) {
    double acc = 0.0;
    uint64_t wsum = 0;
    uint64_t yc = y.c, yf = y.f;
#pragma unroll 1
    for (uint64_t yleft = ay.total; yleft != 0;) {
        const uint64_t ycap = ay.den - yf, wy = ycap < yleft ? ycap : yleft;
        const uint64_t row = tap_cell(ay, yc) * pitch;
        double racc = 0.0;
        uint64_t rw = 0;
        uint64_t xc = x.c, xf = x.f;
#pragma unroll 1
        for (uint64_t xleft = ax.total; xleft != 0;) {
            const uint64_t xcap = ax.den - xf, wx = xcap < xleft ? xcap : xleft;
            const uint64_t at = row + tap_cell(ax, xc);
            const double term = static_cast<double>(wx) * to_f64(resample_load<!(BITS & 1u)>(win + at));
            const double next = racc + term;
            if constexpr (MASKED) {
                const bool on = resample_load<!(BITS & 2u)>(mwin + at) != 0;
                racc = on ? next : racc;
                rw += on ? wx : 0;
            } else {
                racc = next;
                rw += wx;
            }
            xleft -= wx;
            ++xc;
            xf = 0;
        }
        const double yterm = static_cast<double>(wy) * racc;
        acc = acc + yterm;
        wsum += wy * rw;  // at most total_x * total_y: fits, checked by the host
        yleft -= wy;
        ++yc;
        yf = 0;
    }
    *valid = wsum != 0;
    if (wsum == 0) return T(0);
    return resample_cell_of<T>(acc / static_cast<double>(wsum));
}

// Launch arguments: WindowArgs (g: pitch and origin of the raster side, w and n of the OUTPUT), the two axes, and `cellwise_stores`:
// set when the "unaligned_vector" knob is off and an output pointer is not 16-byte aligned — every slot is then stored cell by cell.
struct ResampleArgs {
    WindowArgs w;
    ResampleAxis ax, ay;
    unsigned cellwise_stores;
    uint64_t first_tile;  // this launch covers the tiles [first_tile, first_tile + gridDim.x) of the output (split_launch, ec_runtime.hpp)
};

template <typename T, bool MASKED>
__global__ __launch_bounds__(kBlock) void k_window_resample(ResampleArgs a) {
    constexpr int W = sizeof(T), CPL = 16 / W, SLOTS = kWindowTileSlots;
    constexpr uint32_t SPAN = uint32_t(SLOTS) * CPL;
    using C = typename width_cell<W>::type;
    const WindowGeom& g = a.w.g;
    const uint64_t first = uint64_t(two_front_tile(a.first_tile)) * SPAN;
    if (first >= g.n) return;
    const uint64_t row0 = first / g.w, col0 = first - row0 * g.w;  // wave-uniform, once per workgroup
    const T* __restrict__ win = static_cast<const T*>(a.w.in) + g.origin;
    const uint8_t* __restrict__ mwin = MASKED ? a.w.in_mask + g.origin : nullptr;
    C* __restrict__ dst = static_cast<C*>(a.w.out);
    uint8_t* __restrict__ dmask = a.w.out_mask;
    if constexpr (MASKED) __builtin_assume(dmask != nullptr);  // both masks or neither (check_window): slot_store_pair's test folds away
    policy_arms<MASKED ? 2 : 1>(a.w.cacheable, [&](auto bits) {
#pragma unroll 1
        for (uint32_t s = threadIdx.x; s < uint32_t(SLOTS); s += kBlock) {
            const uint32_t off = s * CPL;
            const uint64_t c0 = first + off;
            if (c0 >= g.n) break;
            const RowCol rc = lane_row_col<SPAN>(row0, col0, off, g.w);
            const uint32_t cells = g.n - c0 < uint64_t(CPL) ? uint32_t(g.n - c0) : uint32_t(CPL);
            const bool whole = cells == uint32_t(CPL) && !a.cellwise_stores;
            TapPos y = tap_at(a.ay, rc.row), x = tap_at(a.ax, rc.col);
            RowCursor at{rc.col, g.w};
            uint64_t lo = 0, hi = 0;  // the slot's 16 value bytes, packed by shifts: k is a loop counter here, an array would go to scratch
            SlotMask m;
#pragma unroll 1
            for (uint32_t k = 0; k < cells; ++k) {
                bool valid;
                const T v = resample_footprint<T, MASKED, decltype(bits)::value>(win, mwin, g.pitch, a.ax, a.ay, x, y, &valid);
                const C c = __builtin_bit_cast(C, v);
                if (whole) {
                    const uint32_t sh = (k * 8 * W) & 63u;
                    if (k * W < 8) lo |= uint64_t(c) << sh;
                    else hi |= uint64_t(c) << sh;
                    if constexpr (MASKED) m.put(k, valid);
                } else {
                    st_cell(c, dst + c0 + k);
                    if constexpr (MASKED) st_cell(uint8_t(valid), dmask + c0 + k);
                }
                tap_step(a.ax, x);
                at.next([&] {
                    x = tap_first(a.ax);
                    tap_step(a.ay, y);
                });
            }
            if (whole) slot_store_pair<CPL>(u32x4{uint32_t(lo), uint32_t(lo >> 32), uint32_t(hi), uint32_t(hi >> 32)}, m, dst, MASKED ? dmask : nullptr, c0);
        }
    });
}

}  // namespace ecd
