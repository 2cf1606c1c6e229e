// ec_compare_kernels.hpp — per-cell order predicates as masks, and the pick of cells by a mask (gfx950): the Fns of
// ec_compare, ec_compare_scalar, ec_select and ec_masked_select on the k_map skeleton (ec_map_kernels.hpp).
//
// The compiler notes of DESIGN §9 apply as in every map kernel: 1-byte streams travel as words (cells<T, N> / load_cells), the
// two VALUE operands take the launch's load policy (kIn0, kIn1 -> cache_plan -> policy_arms), mask inputs are loaded `nt`,
// the mask output leaves with mask_store (`nt`), selected values with nt_store / st_cell.  Every load is unconditional.
#pragma once

#include "ec_compare_cell.hpp"
#include "ec_map_kernels.hpp"

namespace ecd {

// NMASK mask streams of one group, ANDed; mask bytes are 0 / 1 (src/masked/mask.rs:10-12)
template <int NMASK, int CPL>
struct MaskIn {
    cells<uint8_t, CPL> m[NMASK > 0 ? NMASK : 1];
    __device__ __forceinline__ uint8_t valid(int k) const {
        if constexpr (NMASK == 0) return 1;
        else if constexpr (NMASK == 1) return m[0][k];
        else return m[0][k] & m[1][k];
    }
};

// ---- ec_compare: out_mask[i] = rel(CellValue(l[i]).cmp(CellValue(r[i]))) (src/value.rs:248-271), ANDed with the NMASK masks
// given — a cell that is not valid satisfies no predicate (the masked-operator rule, src/masked/masked_buffer.rs:326-335).
// One mask is one mask, whichever operand it belongs to: NMASK = 0, 1, 2.
template <typename L, typename R, int NMASK>
struct CompareFn {
    static constexpr int CPL = 16 / max_of<sizeof(L), sizeof(R)>::value;
    static constexpr size_t kIn0 = sizeof(L), kIn1 = sizeof(R);
    using MV = vec<uint8_t, CPL>;
    struct In { cells<L, CPL> l; cells<R, CPL> r; MaskIn<NMASK, CPL> m; };
    const L* __restrict__ l;
    const R* __restrict__ r;
    const uint8_t* m0;
    const uint8_t* m1;
    uint8_t* out;
    uint32_t rel;
    template <bool NT0, bool NT1>
    __device__ __forceinline__ In load(size_t g) const {
        In in;
        in.l = load_cells<NT0, L, CPL>(l + g * CPL);
        in.r = load_cells<NT1, R, CPL>(r + g * CPL);
        if constexpr (NMASK >= 1) in.m.m[0] = load_cells<true, uint8_t, CPL>(m0 + g * CPL);
        if constexpr (NMASK >= 2) in.m.m[1] = load_cells<true, uint8_t, CPL>(m1 + g * CPL);
        return in;
    }
    __device__ __forceinline__ void store(size_t g, const In& in) const {
        MV o;
#pragma unroll
        for (int k = 0; k < CPL; ++k) o[k] = cell_cmp<L, R>(in.l[k], in.r[k], rel) & in.m.valid(k);
        mask_store(o, reinterpret_cast<MV*>(out) + g);
    }
    __device__ __forceinline__ void cell(size_t i) const {
        uint8_t v = cell_cmp<L, R>(ld_cell(l + i), ld_cell(r + i), rel);
        if constexpr (NMASK >= 1) v &= ld_cell(m0 + i);
        if constexpr (NMASK >= 2) v &= ld_cell(m1 + i);
        st_cell<uint8_t>(v, out + i);
    }
};

// ---- ec_compare_scalar: the same with r[i] replaced by a scalar.  Typed by (L, UT) with UT = union(L, the scalar's type): the
// host converts the scalar to UT once (CellValue::convert, src/value.rs:74-98 — always a widening), the kernel converts the
// cell; union(L, UT) == UT, so cell_cmp<L, UT> compares exactly what cell_cmp<L, S> would.  41 (L, UT) pairs instead of 100.
template <typename L, typename UT, int NMASK>
struct CompareScalarFn {
    static_assert(ecl::union_of(ecl::dtype_of<L>::value, ecl::dtype_of<UT>::value) == ecl::dtype_of<UT>::value, "UT is a union with L");
    static constexpr int CPL = 16 / sizeof(L);
    static constexpr size_t kIn0 = sizeof(L), kIn1 = 0;
    using MV = vec<uint8_t, CPL>;
    struct In { cells<L, CPL> l; MaskIn<NMASK, CPL> m; };
    const L* __restrict__ l;
    const uint8_t* m0;
    uint8_t* out;
    UT rhs;
    uint32_t rel;
    template <bool NT0, bool NT1>
    __device__ __forceinline__ In load(size_t g) const {
        In in;
        in.l = load_cells<NT0, L, CPL>(l + g * CPL);
        if constexpr (NMASK >= 1) in.m.m[0] = load_cells<true, uint8_t, CPL>(m0 + g * CPL);
        return in;
    }
    __device__ __forceinline__ void store(size_t g, const In& in) const {
        MV o;
#pragma unroll
        for (int k = 0; k < CPL; ++k) o[k] = cell_cmp<L, UT>(in.l[k], rhs, rel) & in.m.valid(k);
        mask_store(o, reinterpret_cast<MV*>(out) + g);
    }
    __device__ __forceinline__ void cell(size_t i) const {
        uint8_t v = cell_cmp<L, UT>(ld_cell(l + i), rhs, rel);
        if constexpr (NMASK >= 1) v &= ld_cell(m0 + i);
        st_cell<uint8_t>(v, out + i);
    }
};

// ---- ec_select: out[i] = sel[i] ? a[i] : b[i], cells moved by width W (cloud fill, compositing; the two-buffer form of
// to_vec_with_nodata, src/masked/masked_buffer.rs:143-148).  MASKED: also out_mask[i] = sel[i] ? amask[i] : bmask[i].
// No __restrict__: out may be a or b (the in-place patch) and out_mask one of the masks, for the reason MaskBin may run in
// place — every lane loads a group and stores the same group.
template <typename W, bool MASKED>
struct SelectFn {
    static constexpr int CPL = 16 / sizeof(W);
    static constexpr size_t kIn0 = sizeof(W), kIn1 = sizeof(W);
    using SV = vec<W, CPL>;
    using MV = vec<uint8_t, CPL>;
    struct In { cells<W, CPL> a, b; cells<uint8_t, CPL> s, am, bm; };
    const W* a;
    const W* b;
    const uint8_t* sel;
    const uint8_t* amask;
    const uint8_t* bmask;
    W* out;
    uint8_t* out_mask;
    template <bool NT0, bool NT1>
    __device__ __forceinline__ In load(size_t g) const {
        In in;
        in.a = load_cells<NT0, W, CPL>(a + g * CPL);
        in.b = load_cells<NT1, W, CPL>(b + g * CPL);
        in.s = load_cells<true, uint8_t, CPL>(sel + g * CPL);
        if constexpr (MASKED) {
            in.am = load_cells<true, uint8_t, CPL>(amask + g * CPL);
            in.bm = load_cells<true, uint8_t, CPL>(bmask + g * CPL);
        }
        return in;
    }
    __device__ __forceinline__ void store(size_t g, const In& in) const {
        SV o;
#pragma unroll
        for (int k = 0; k < CPL; ++k) o[k] = in.s[k] ? in.a[k] : in.b[k];
        nt_store(o, reinterpret_cast<SV*>(out) + g);
        if constexpr (MASKED) {
            MV m;
#pragma unroll
            for (int k = 0; k < CPL; ++k) m[k] = in.s[k] ? in.am[k] : in.bm[k];
            mask_store(m, reinterpret_cast<MV*>(out_mask) + g);
        }
    }
    __device__ __forceinline__ void cell(size_t i) const {
        const W x = ld_cell(a + i), y = ld_cell(b + i);  // unconditional, as in MaskSelectFn
        const uint8_t s = ld_cell(sel + i);
        if constexpr (MASKED) {
            const uint8_t xm = ld_cell(amask + i), ym = ld_cell(bmask + i);
            st_cell<uint8_t>(s ? xm : ym, out_mask + i);
        }
        st_cell<W>(s ? x : y, out + i);
    }
};

}  // namespace ecd
