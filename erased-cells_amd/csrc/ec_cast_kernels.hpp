// ec_cast_kernels.hpp — a buffer's cells in a storage cell type (gfx950): the Fns of ec_cast and ec_cast_scaled on the k_map
// skeleton (ec_map_kernels.hpp).  The per-cell functions are ec_cast_cell.hpp.
//
// These are the Fns whose STORED stream may be narrower than the loaded one (ConvertFn only widens).  The shape is the one
// MaskFromNodataFn<8-byte W> already has per lane (8 B in, 1 B out): CPL = 16 / the widest cell of the pair, so the wider stream
// moves 16 B per lane per access and the narrower one CPL * width bytes (2, 4 or 8), lane-contiguous — a wave's store is one
// contiguous span of 128, 256 or 512 bytes.  One group per store: what a lane gathering several groups into one wider store
// would gain is not measured (tools/cast_bench.py has the rows to measure it against).
// The compiler notes of DESIGN §9 apply as in every map kernel: 1-byte streams are loaded as words (cells<T, N> / load_cells),
// the source takes the launch's load policy (kIn0 -> cache_plan -> policy_arms), as does the mask of ec_cast_scaled (kIn1, as in
// MaskSelectFn); converted cells leave with cast_store (below) / st_cell.  Every load is unconditional: a masked-out cell is loaded and
// not used, and what it holds — a NaN included — leaves no trace.
#pragma once

#include "ec_cast_cell.hpp"
#include "ec_map_kernels.hpp"

namespace ecd {

// The store of a group of converted cells.  The library's VALUE store is nt_store (`sc1 nt`, write-through: ec_device.hpp), which pays
// where the output is most of a launch's bytes; a destination NARROWER than the source is the minority of them, and there `nt`
// alone — the store of the mask outputs — measured better, as ec_device.hpp records for those: u16 -> u8 1.012 -> 1.000 (EC_CAST_AS
// 1.045 -> 0.997) of ec_mask_from_nodata on the same bytes, f64 -> i16 418 -> 411 µs, f64 -> u8 and f64 -> f32 unchanged; but masked
// ec_cast_scaled f64 -> i16 442 -> 459 µs, so the masked form keeps the write-through store (profiles/cast/cast.md).
template <bool NT_ONLY, typename V>
__device__ __forceinline__ void cast_store(V v, V* p) {
    if constexpr (NT_ONLY) mask_store(v, p);
    else nt_store(v, p);
}

// ---- ec_cast: dst[i] = cast_round<S, D>(src[i]) (ROUND) or cast_as<S, D>(src[i]).  Instantiated for the 59 pairs ec_convert
// refuses; with both modes only where they differ (an integer destination).
template <typename S, typename D, bool ROUND>
struct CastFn {
    static constexpr int CPL = 16 / max_of<sizeof(S), sizeof(D)>::value;
    static constexpr size_t kIn0 = sizeof(S), kIn1 = 0;
    using DV = vec<D, CPL>;
    using In = cells<S, CPL>;
    const S* __restrict__ src;
    D* __restrict__ dst;
    static __device__ __forceinline__ D one(S v) {
        if constexpr (ROUND) return cast_round<S, D>(v);
        else return cast_as<S, D>(v);
    }
    template <bool NT0, bool NT1>
    __device__ __forceinline__ In load(size_t g) const { return load_cells<NT0, S, CPL>(src + g * CPL); }
    __device__ __forceinline__ void store(size_t g, const In& x) const {
        DV o;
#pragma unroll
        for (int k = 0; k < CPL; ++k) o[k] = one(x[k]);
        cast_store<(sizeof(D) < sizeof(S))>(o, reinterpret_cast<DV*>(dst) + g);
    }
    __device__ __forceinline__ void cell(size_t i) const { st_cell(one(ld_cell(src + i)), dst + i); }
};

// ---- ec_cast_scaled: dst[i] = mask[i] ? scaled<S, D>(src[i], scale, offset) : nodata — to_vec_with_nodata
// (src/masked/masked_buffer.rs:137-152) for a type the buffer does not fit into, in one launch.
template <typename S, typename D, bool MASKED>
struct CastScaledFn {
    static constexpr int CPL = 16 / max_of<sizeof(S), sizeof(D)>::value;
    static constexpr size_t kIn0 = sizeof(S), kIn1 = MASKED ? 1 : 0;
    using DV = vec<D, CPL>;
    struct In { cells<S, CPL> x; cells<uint8_t, CPL> m; };
    const S* __restrict__ src;
    const uint8_t* __restrict__ mask;
    D* __restrict__ dst;
    double scale, offset;
    D nd;
    template <bool NT0, bool NT1>
    __device__ __forceinline__ In load(size_t g) const {
        In in;
        in.x = load_cells<NT0, S, CPL>(src + g * CPL);
        if constexpr (MASKED) in.m = load_cells<NT1, uint8_t, CPL>(mask + g * CPL);
        return in;
    }
    __device__ __forceinline__ void store(size_t g, const In& in) const {
        DV o;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const D y = scaled<S, D>(in.x[k], scale, offset);
            if constexpr (MASKED) o[k] = in.m[k] ? y : nd;
            else o[k] = y;
        }
        cast_store<(sizeof(D) < sizeof(S)) && !MASKED>(o, reinterpret_cast<DV*>(dst) + g);
    }
    __device__ __forceinline__ void cell(size_t i) const {
        const D y = scaled<S, D>(ld_cell(src + i), scale, offset);  // unconditional, as in MaskSelectFn
        if constexpr (MASKED) st_cell<D>(ld_cell(mask + i) ? y : nd, dst + i);
        else st_cell<D>(y, dst + i);
    }
};

}  // namespace ecd
