// ec_abi.hip — the extern "C" compute surface of liberased_cells_hip.so (include/erased_cells.h):
// the type lattice and the type-erased dispatch of every kernel family except the four binary ops
// (ec_binop_*.hip) and the fused chains (ec_fused*.hip).  Devices, memory, streams: ec_runtime.hip.
//
// There is no CPU fallback anywhere in this library: without a HIP device every
// compute entry point returns EC_ERR_HIP / EC_ERR_NOT_INITIALIZED.
#include <hip/hip_runtime.h>


#include <cfloat>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "ec_dispatch.hpp"
#include "ec_lattice.hpp"
#include "ec_map_kernels.hpp"
#include "ec_map_launch.hpp"
#include "ec_reduce_kernels.hpp"
#include "ec_reduce_launch.hpp"
#include "ec_runtime.hpp"

namespace ecd {

static_assert(kMaxReduceBlocks <= kFinalizeMaxParts, "the finalize kernels read at most kFinalizeMaxParts partials");

// first difference and mask counts: the default shape, its cell-wise branch inside the same kernel
constexpr ReduceShape kScanShape = {kRBlock, kReduceU, 4, kRBlock, 4};

// ------------------------------------------------------------------ convert
template <typename Sx, typename Dx>
static ec_status launch_convert(const void* src, void* dst, size_t n, hipStream_t s) {
    if constexpr (ecl::can_fit_into(ecl::dtype_of<Sx>::value, ecl::dtype_of<Dx>::value) &&
                  ecl::dtype_of<Sx>::value != ecl::dtype_of<Dx>::value) {
        ConvertFn<Sx, Dx> fn{static_cast<const Sx*>(src), static_cast<Dx*>(dst)};
        return launch_map(fn, n, aligned16(src, dst, dst), s, "convert");
    } else {
        (void)src; (void)dst; (void)n; (void)s;
        return set_error(EC_ERR_ARG, "convert: pair not instantiated");
    }
}

static ec_status dispatch_convert(int st, const void* src, int dt, void* dst, size_t n, hipStream_t s) {
    return ecl::with_cell_types(st, dt, [&](auto sc, auto dc) { return launch_convert<ecl::cell_t<decltype(sc)>, ecl::cell_t<decltype(dc)>>(src, dst, n, s); },
                                [] { return set_error(EC_ERR_UNSUPPORTED_TYPE, "convert: bad dtype"); });
}

// ------------------------------------------------------------------ min/max
template <typename T>
struct MinMaxReduction {
    using Cell = T;
    using Partial = int64_t;  // partials[2 * b], [2 * b + 1]: workgroup b's key pair
    using Out = int64_t;      // {~key(min), key(max)}
    static constexpr ScratchSlot kPartials = kScratchPartials;
    static constexpr const char *kSingle = "min_max(single workgroup)", *kPartialsName = "min_max(partials)", *kFinalizeName = "min_max(finalize)";
    template <bool MASKED, int U, int BLOCK> static auto vector_kernel() { return k_min_max_partials<T, MASKED, U, BLOCK>; }
    template <bool MASKED> static auto cellwise_kernel() { return k_min_max_partials_cellwise<T, MASKED>; }
    static void finalize(const int64_t* partials, int nparts, const T*, int64_t* keys2_dev, hipStream_t s) {
        // sentinels (T::MAX, T::MIN): src/buffer.rs:170, finite for floats (src/ctype.rs:158-179)
        k_min_max_finalize<<<1, kFinalizeBlock, 0, s>>>(partials, nparts, order_key<T>(Limits<T>::hi), order_key<T>(Limits<T>::lo), keys2_dev);
    }
};

template <typename T>
static ec_status launch_min_max(const void* p, const uint8_t* mask, size_t n, int64_t* keys2_dev, hipStream_t s) {
    using R = MinMaxReduction<T>;
    // launch shape: 512 threads x 8 loads in flight, 4 workgroups per CU by default; "reduce_shape" selects the A/B alternatives
    switch (tuning().reduce_shape) {
        case 1: return launch_reduction<R, 16, 512, 4>(p, mask, n, keys2_dev, s);
        case 2: return launch_reduction<R, 8, 256, 8>(p, mask, n, keys2_dev, s);
        case 3: return launch_reduction<R, 8, 1024, 2>(p, mask, n, keys2_dev, s);
        case 4: return launch_reduction<R, 4, 512, 4>(p, mask, n, keys2_dev, s);
        default: return launch_reduction<R, kReduceU, kRBlock, 4>(p, mask, n, keys2_dev, s);
    }
}

static ec_status dispatch_min_max(int t, const void* p, const uint8_t* mask, size_t n, int64_t* keys2_dev, hipStream_t s) {
    return ecl::with_cell_type(t, [&](auto c) { return launch_min_max<ecl::cell_t<decltype(c)>>(p, mask, n, keys2_dev, s); },
                               [] { return set_error(EC_ERR_UNSUPPORTED_TYPE, "min_max: bad dtype"); });
}

template <typename T>
static void decode_keys(const int64_t keys2[2], ec_value* mn, ec_value* mx) {
    ecl::put_value<T>(mn, ecl::dtype_of<T>::value, key_value<T>(~keys2[0]));
    ecl::put_value<T>(mx, ecl::dtype_of<T>::value, key_value<T>(keys2[1]));
}

}  // namespace ecd

using namespace ecd;

// =================================================================== lattice
extern "C" ec_dtype ec_union(ec_dtype a, ec_dtype b) {
    return (ecl::valid(a) && ecl::valid(b)) ? static_cast<ec_dtype>(ecl::union_of(a, b)) : static_cast<ec_dtype>(EC_F64);
}
extern "C" int32_t ec_can_fit_into(ec_dtype src, ec_dtype dst) {
    return ecl::valid(src) && ecl::valid(dst) && ecl::can_fit_into(src, dst);
}
extern "C" size_t ec_size_of(ec_dtype t) { return ecl::size_of(t); }
extern "C" ec_dtype ec_neg_result_type(ec_dtype t) { return static_cast<ec_dtype>(ecl::neg_result(t)); }

using ecl::put_value;
using ecl::value_as;

extern "C" ec_status ec_min_value(ec_dtype t, ec_value* out) {
    if (!out) return set_error(EC_ERR_ARG, "ec_min_value: null out");
    return ecl::with_cell_type(t, [&](auto c) -> ec_status { using T = ecl::cell_t<decltype(c)>; put_value<T>(out, t, Limits<T>::lo); return EC_OK; },
                               [&] { return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_min_value: bad dtype %d", int(t)); });
}
extern "C" ec_status ec_max_value(ec_dtype t, ec_value* out) {
    if (!out) return set_error(EC_ERR_ARG, "ec_max_value: null out");
    return ecl::with_cell_type(t, [&](auto c) -> ec_status { using T = ecl::cell_t<decltype(c)>; put_value<T>(out, t, Limits<T>::hi); return EC_OK; },
                               [&] { return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_max_value: bad dtype %d", int(t)); });
}
extern "C" ec_status ec_nodata_default(ec_dtype t, ec_value* out) {
    if (!out) return set_error(EC_ERR_ARG, "ec_nodata_default: null out");
    if (t == EC_F32) { put_value<uint32_t>(out, t, 0x7fc00000u); return EC_OK; }           // f32::NAN
    if (t == EC_F64) { put_value<uint64_t>(out, t, 0x7ff8000000000000ull); return EC_OK; }  // f64::NAN
    return ec_min_value(t, out);                                                            // <int>::MIN
}

extern "C" double ec_value_to_f64(const ec_value* v) {
    if (!v) return 0.0;
    return ecl::with_cell_type(v->dtype, [&](auto c) { return static_cast<double>(value_as<ecl::cell_t<decltype(c)>>(*v)); }, 0.0);
}

extern "C" ec_status ec_value_convert(const ec_value* v, ec_dtype dst, ec_value* out) {
    if (!v || !out) return set_error(EC_ERR_ARG, "ec_value_convert: null argument");
    if (!ecl::valid(v->dtype) || !ecl::valid(dst)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_value_convert: bad dtype");
    if (!ecl::can_fit_into(v->dtype, dst)) return set_narrowing(v->dtype, dst);  // value.rs:79-81
    if (v->dtype == dst) { *out = *v; return EC_OK; }                            // value.rs:83-85
    return ecl::with_cell_types(v->dtype, dst, [&](auto sc, auto dc) -> ec_status {
        using Dx = ecl::cell_t<decltype(dc)>;
        put_value<Dx>(out, dst, static_cast<Dx>(value_as<ecl::cell_t<decltype(sc)>>(*v)));
        return EC_OK;
    }, [] { return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_value_convert: bad dtype"); });
}

extern "C" ec_status ec_shard_range(uint64_t n_rows, uint64_t n_cols, uint32_t shard, uint32_t n_shards,
                                    uint64_t* cell_offset, uint64_t* cell_len) {
    if (!cell_offset || !cell_len || n_shards == 0 || shard >= n_shards)
        return set_error(EC_ERR_ARG, "ec_shard_range: shard %u of %u", shard, n_shards);
    const uint64_t q = n_rows / n_shards, rem = n_rows % n_shards;
    const uint64_t row0 = uint64_t(shard) * q + (shard < rem ? shard : rem);
    const uint64_t rows = q + (shard < rem ? 1 : 0);
    *cell_offset = row0 * n_cols;
    *cell_len = rows * n_cols;
    return EC_OK;
}

// =================================================================== arithmetic
#define EC_REQUIRE_INIT()               \
    do {                                \
        ec_status st_ = ensure_ready();  \
        if (st_ != EC_OK) return st_;   \
    } while (0)

extern "C" ec_status ec_binop(ec_op op, ec_dtype lt, const void* l, ec_dtype rt, const void* r, size_t n, double* out,
                              ec_stream stream) {
    EC_REQUIRE_INIT();
    if (n == 0) return EC_OK;
    if (!l || !r || !out) return set_error(EC_ERR_ARG, "ec_binop: null pointer");
    switch (op) {
        case EC_ADD: return dispatch_binop<EC_ADD>(lt, l, rt, r, n, out, S(stream));
        case EC_SUB: return dispatch_binop<EC_SUB>(lt, l, rt, r, n, out, S(stream));
        case EC_MUL: return dispatch_binop<EC_MUL>(lt, l, rt, r, n, out, S(stream));
        case EC_DIV: return dispatch_binop<EC_DIV>(lt, l, rt, r, n, out, S(stream));
    }
    return set_error(EC_ERR_ARG, "ec_binop: bad op %d", int(op));
}

extern "C" ec_status ec_binop_scalar(ec_op op, ec_dtype lt, const void* l, size_t n, const ec_value* rhs, double* out,
                                     ec_stream stream) {
    EC_REQUIRE_INIT();
    if (!rhs || !ecl::valid(rhs->dtype)) return set_error(EC_ERR_ARG, "ec_binop_scalar: bad rhs");
    if (n == 0) return EC_OK;
    if (!l || !out) return set_error(EC_ERR_ARG, "ec_binop_scalar: null pointer");
    // unify + to_f64 of the scalar (value.rs:206-207) happens once, here
    const double s = ec_value_to_f64(rhs);
    switch (op) {
        case EC_ADD: return dispatch_binop_scalar<EC_ADD>(lt, l, s, n, out, S(stream));
        case EC_SUB: return dispatch_binop_scalar<EC_SUB>(lt, l, s, n, out, S(stream));
        case EC_MUL: return dispatch_binop_scalar<EC_MUL>(lt, l, s, n, out, S(stream));
        case EC_DIV: return dispatch_binop_scalar<EC_DIV>(lt, l, s, n, out, S(stream));
    }
    return set_error(EC_ERR_ARG, "ec_binop_scalar: bad op %d", int(op));
}

extern "C" ec_status ec_masked_binop(ec_op op, ec_dtype lt, const void* l, const uint8_t* lmask, ec_dtype rt, const void* r,
                                     const uint8_t* rmask, size_t n, double* out, uint8_t* out_mask, ec_stream stream) {
    EC_REQUIRE_INIT();
    if (n == 0) return EC_OK;
    if (!l || !r || !out || !lmask || !rmask || !out_mask) return set_error(EC_ERR_ARG, "ec_masked_binop: null pointer");
    switch (op) {
        case EC_ADD: return dispatch_masked_binop<EC_ADD>(lt, l, lmask, rt, r, rmask, n, out, out_mask, S(stream));
        case EC_SUB: return dispatch_masked_binop<EC_SUB>(lt, l, lmask, rt, r, rmask, n, out, out_mask, S(stream));
        case EC_MUL: return dispatch_masked_binop<EC_MUL>(lt, l, lmask, rt, r, rmask, n, out, out_mask, S(stream));
        case EC_DIV: return dispatch_masked_binop<EC_DIV>(lt, l, lmask, rt, r, rmask, n, out, out_mask, S(stream));
    }
    return set_error(EC_ERR_ARG, "ec_masked_binop: bad op %d", int(op));
}

extern "C" ec_status ec_neg(ec_dtype t, const void* in, size_t n, void* out, ec_stream stream) {
    EC_REQUIRE_INIT();
    if (!ecl::valid(t)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_neg: bad dtype %d", int(t));
    if (n == 0) return EC_OK;
    if (!in || !out) return set_error(EC_ERR_ARG, "ec_neg: null pointer");
    return ecl::with_cell_type(t, [&](auto c) {
        using T = ecl::cell_t<decltype(c)>;
        NegFn<T> fn{static_cast<const T*>(in), static_cast<typename NegOut<T>::type*>(out)};
        return launch_map(fn, n, aligned16(in, out, out), S(stream), "neg");
    }, kTypeChecked);
}

extern "C" ec_status ec_convert(ec_dtype st, const void* src, ec_dtype dt, void* dst, size_t n, ec_stream stream) {
    EC_REQUIRE_INIT();
    if (!ecl::valid(st) || !ecl::valid(dt)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_convert: bad dtype");
    if (!ecl::can_fit_into(st, dt)) return set_narrowing(st, dt);  // buffer.rs:157-159: before touching data
    if (n == 0) return EC_OK;
    if (!src || !dst) return set_error(EC_ERR_ARG, "ec_convert: null pointer");
    if (st == dt) return ec_copy(dst, src, n * ecl::size_of(st), stream);  // buffer.rs:151-153
    return dispatch_convert(st, src, dt, dst, n, S(stream));
}

template <typename W>
static ec_status fill_w(void* dst, size_t n, const ec_value* v, hipStream_t s) {
    FillFn<W> fn{static_cast<W*>(dst), value_as<W>(*v)};
    return launch_map(fn, n, aligned16(dst, dst, dst), s, "fill");
}

extern "C" ec_status ec_fill(ec_dtype t, void* dst, size_t n, const ec_value* value, ec_stream stream) {
    EC_REQUIRE_INIT();
    if (!ecl::valid(t) || !value || value->dtype != t) return set_error(EC_ERR_ARG, "ec_fill: value dtype must equal t");
    if (n == 0) return EC_OK;
    if (!dst) return set_error(EC_ERR_ARG, "ec_fill: null pointer");
    return ecl::with_cell_width(ecl::size_of(t), [&](auto w) { return fill_w<ecl::cell_t<decltype(w)>>(dst, n, value, S(stream)); }, kTypeChecked);
}

// =================================================================== min/max
extern "C" ec_status ec_min_max_keys(ec_dtype t, const void* p, const uint8_t* mask_or_null, size_t n, int64_t* keys2_dev,
                                     ec_stream stream) {
    EC_REQUIRE_INIT();
    if (!keys2_dev || (n > 0 && !p)) return set_error(EC_ERR_ARG, "ec_min_max_keys: null pointer");
    return dispatch_min_max(t, p, mask_or_null, n, keys2_dev, S(stream));
}

extern "C" ec_status ec_min_max_decode(ec_dtype t, const int64_t keys2_host[2], ec_value* mn, ec_value* mx) {
    if (!keys2_host || !mn || !mx) return set_error(EC_ERR_ARG, "ec_min_max_decode: null pointer");
    return ecl::with_cell_type(t, [&](auto c) -> ec_status { decode_keys<ecl::cell_t<decltype(c)>>(keys2_host, mn, mx); return EC_OK; },
                               [&] { return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_min_max_decode: bad dtype %d", int(t)); });
}

extern "C" ec_status ec_min_max(ec_dtype t, const void* p, const uint8_t* mask_or_null, size_t n, ec_value* mn, ec_value* mx,
                                ec_stream stream) {
    EC_REQUIRE_INIT();
    if (!mn || !mx || (n > 0 && !p)) return set_error(EC_ERR_ARG, "ec_min_max: null pointer");
    int64_t keys2[2];
    ec_status st = sync_result(S(stream), kResultWords, keys2, sizeof keys2, [&](const Scratch&, int64_t* words) {
        return dispatch_min_max(t, p, mask_or_null, n, words, S(stream));
    });
    if (st != EC_OK) return st;
    return ec_min_max_decode(t, keys2, mn, mx);
}

// =================================================================== Ord / Eq
template <typename W>
static ec_status first_diff_w(const void* l, const void* r, size_t n, const Scratch& sc, hipStream_t s, unsigned* grid_out) {
    const size_t stream_bytes[2] = {n * sizeof(W), n * sizeof(W)};
    const ReducePlan pl = plan_reduction(l, residue(r, 16), sizeof(W), n, kScanShape, stream_bytes, 2);
    k_first_diff_partials<W, kReduceU><<<pl.grid, kRBlock, 0, s>>>(static_cast<const W*>(l), static_cast<const W*>(r), n,
                                                                  reinterpret_cast<uint64_t*>(sc.at(kScratchPartials)), pl.aligned, pl.head_policy);
    *grid_out = pl.grid;
    return check_launch("first_diff(partials)");
}

extern "C" ec_status ec_first_difference(ec_dtype t, const void* l, const void* r, size_t n, uint64_t* index, ec_stream stream) {
    EC_REQUIRE_INIT();
    if (!ecl::valid(t)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_first_difference: bad dtype %d", int(t));
    if (!index || (n > 0 && (!l || !r))) return set_error(EC_ERR_ARG, "ec_first_difference: null pointer");
    *index = n;
    if (n == 0) return EC_OK;
    uint64_t first = 0;
    ec_status st = sync_result(S(stream), kResultWords, &first, sizeof first, [&](const Scratch& sc, int64_t* words) {
        unsigned grid = 0;
        const ec_status st2 = ecl::with_cell_width(ecl::size_of(t), [&](auto w) { return first_diff_w<ecl::cell_t<decltype(w)>>(l, r, n, sc, S(stream), &grid); }, kTypeChecked);
        if (st2 != EC_OK) return st2;
        k_first_diff_finalize<<<1, kFinalizeBlock, 0, S(stream)>>>(reinterpret_cast<const uint64_t*>(sc.at(kScratchPartials)), static_cast<int>(grid),
                                                           reinterpret_cast<uint64_t*>(words));
        return check_launch("first_diff(finalize)");
    });
    if (st != EC_OK) return st;
    *index = first == ~0ull ? n : first;
    return EC_OK;
}

template <typename T>
static int order_cmp(const void* a, const void* b) {
    T x, y;
    std::memcpy(&x, a, sizeof x);
    std::memcpy(&y, b, sizeof y);
    const int64_t kx = order_key<T>(x), ky = order_key<T>(y);
    return (kx > ky) - (kx < ky);
}

extern "C" ec_status ec_buffer_cmp(ec_dtype lt, const void* l, size_t nl, ec_dtype rt, const void* r, size_t nr,
                                   int32_t* ordering, ec_stream stream) {
    EC_REQUIRE_INIT();
    if (!ordering) return set_error(EC_ERR_ARG, "ec_buffer_cmp: null result pointer");
    if (!ecl::valid(lt) || !ecl::valid(rt)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_buffer_cmp: bad dtype");
    if (lt != rt) { *ordering = lt < rt ? -1 : 1; return EC_OK; }  // cell type first (buffer.rs:391-398)
    const size_t n = nl < nr ? nl : nr;
    uint64_t idx = n;
    ec_status st = ec_first_difference(lt, l, r, n, &idx, stream);
    if (st != EC_OK) return st;
    if (idx >= n) { *ordering = (nl > nr) - (nl < nr); return EC_OK; }  // common prefix equal: length decides (:416)
    unsigned char a[8], b[8];
    const size_t sz = ecl::size_of(lt);
    st = ec_download(a, static_cast<const char*>(l) + idx * sz, sz, stream);
    if (st != EC_OK) return st;
    st = ec_download(b, static_cast<const char*>(r) + idx * sz, sz, stream);
    if (st != EC_OK) return st;
    *ordering = ecl::with_cell_type(lt, [&](auto c) { return order_cmp<ecl::cell_t<decltype(c)>>(a, b); }, 0);  // lt was checked above
    return EC_OK;
}

// =================================================================== masks
template <typename W>
static ec_status mask_from_nd_w(const void* p, size_t n, const ec_value* nd, uint8_t* mask, hipStream_t s) {
    MaskFromNodataFn<W> fn{static_cast<const W*>(p), mask, value_as<W>(*nd)};
    const bool al = aligned16(p, p, p) && aligned_to(mask, 16 / sizeof(W));
    return launch_map(fn, n, al, s, "mask_from_nodata");
}

extern "C" ec_status ec_mask_from_nodata(ec_dtype t, const void* p, size_t n, const ec_value* nd_or_null, uint8_t* mask,
                                         ec_stream stream) {
    EC_REQUIRE_INIT();
    if (!ecl::valid(t)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_mask_from_nodata: bad dtype %d", int(t));
    if (nd_or_null && nd_or_null->dtype != t) return set_error(EC_ERR_ARG, "ec_mask_from_nodata: nodata dtype must equal t");
    if (n == 0) return EC_OK;
    if (!p || !mask) return set_error(EC_ERR_ARG, "ec_mask_from_nodata: null pointer");
    if (!nd_or_null)  // NoData::None: nothing matches (nodata.rs:43-48) -> all true
        return check_hip(hipMemsetAsync(mask, 1, n, S(stream)), "hipMemsetAsync");
    return ecl::with_cell_width(ecl::size_of(t), [&](auto w) { return mask_from_nd_w<ecl::cell_t<decltype(w)>>(p, n, nd_or_null, mask, S(stream)); }, kTypeChecked);
}

template <typename W>
static ec_status mask_select_w(const void* p, const uint8_t* mask, size_t n, const ec_value* nd, void* out, hipStream_t s) {
    MaskSelectFn<W> fn{static_cast<const W*>(p), mask, static_cast<W*>(out), value_as<W>(*nd)};
    const bool al = aligned16(p, out, out) && aligned_to(mask, 16 / sizeof(W));
    return launch_map(fn, n, al, s, "mask_select");
}

extern "C" ec_status ec_mask_select(ec_dtype t, const void* p, const uint8_t* mask, size_t n, const ec_value* nd_or_null,
                                    void* out, ec_stream stream) {
    EC_REQUIRE_INIT();
    if (!ecl::valid(t)) return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_mask_select: bad dtype %d", int(t));
    if (nd_or_null && nd_or_null->dtype != t) return set_error(EC_ERR_ARG, "ec_mask_select: nodata dtype must equal t");
    if (n == 0) return EC_OK;
    if (!p || !out) return set_error(EC_ERR_ARG, "ec_mask_select: null pointer");
    if (!nd_or_null) return ec_copy(out, p, n * ecl::size_of(t), stream);  // masked_buffer.rs:149-151
    if (!mask) return set_error(EC_ERR_ARG, "ec_mask_select: null mask");
    return ecl::with_cell_width(ecl::size_of(t), [&](auto w) { return mask_select_w<ecl::cell_t<decltype(w)>>(p, mask, n, nd_or_null, out, S(stream)); }, kTypeChecked);
}

extern "C" ec_status ec_mask_and(const uint8_t* l, const uint8_t* r, size_t n, uint8_t* out, ec_stream stream) {
    EC_REQUIRE_INIT();
    if (n == 0) return EC_OK;
    if (!l || !r || !out) return set_error(EC_ERR_ARG, "ec_mask_and: null pointer");
    MaskBin<0> fn{l, r, out};
    return launch_map(fn, n, aligned16(l, r, out), S(stream), "mask_and");
}
extern "C" ec_status ec_mask_or(const uint8_t* l, const uint8_t* r, size_t n, uint8_t* out, ec_stream stream) {
    EC_REQUIRE_INIT();
    if (n == 0) return EC_OK;
    if (!l || !r || !out) return set_error(EC_ERR_ARG, "ec_mask_or: null pointer");
    MaskBin<1> fn{l, r, out};
    return launch_map(fn, n, aligned16(l, r, out), S(stream), "mask_or");
}
extern "C" ec_status ec_mask_not(const uint8_t* m, size_t n, uint8_t* out, ec_stream stream) {
    EC_REQUIRE_INIT();
    if (n == 0) return EC_OK;
    if (!m || !out) return set_error(EC_ERR_ARG, "ec_mask_not: null pointer");
    MaskNot fn{m, out};
    return launch_map(fn, n, aligned16(m, out, out), S(stream), "mask_not");
}

extern "C" ec_status ec_mask_counts_device(const uint8_t* m, size_t n, uint64_t* counts2_dev, ec_stream stream) {
    EC_REQUIRE_INIT();
    if (!counts2_dev || (n > 0 && !m)) return set_error(EC_ERR_ARG, "ec_mask_counts_device: null pointer");
    Scratch sc;
    ec_status st = get_scratch(S(stream), &sc);
    if (st != EC_OK) return st;
    const ScratchTurn turn(sc);  // the partials slot is min/max's and first difference's too: one call's launches at a time
    unsigned grid = 0;
    if (n > 0) {
        const size_t stream_bytes[1] = {n};
        const ReducePlan pl = plan_reduction(m, 0u, 1, n, kScanShape, stream_bytes, 1);
        grid = pl.grid;
        uint64_t* direct = pl.single ? counts2_dev : nullptr;  // one workgroup: it writes the result itself
        // more workgroups: the last one to add its count to the stream's accumulator word writes the result (one launch) — for masks below
        // 2^29 cells.  Measured, rotating masks, every byte from HBM (profiles/r04/mask_counts_one_launch.md): 4096² 9.5 -> 7.5 µs, 16384²
        // 49.5 -> 47.7 µs, but 32768² 158.4 -> 166.7 µs: the 1,024 returning atomics on one address queue behind the channel's reads when
        // every workgroup is still streaming a gigabyte.  Big masks keep the finalize launch, which they do not feel (2 %); knob
        // `counts_one_launch`: 0 never, 1 (default) below 2^29 cells, 2 always (below 2^40: ticket and sum share a 64-bit word).
        const int one = tuning().counts_one_launch.load();
        uint64_t* acc = (!direct && ((one == 1 && n < (size_t(1) << 29)) || (one >= 2 && n < (size_t(1) << 40)))) ? reinterpret_cast<uint64_t*>(sc.at(kScratchAcc)) : nullptr;
        k_mask_count_partials<kReduceU><<<grid, kRBlock, 0, S(stream)>>>(m, n, reinterpret_cast<uint64_t*>(sc.at(kScratchPartials)), pl.aligned, pl.head_policy,
                                                                        direct, acc, counts2_dev);
        st = check_launch("mask_counts(partials)");
        if (st != EC_OK || direct || acc) return st;
    }
    k_mask_count_finalize<<<1, kFinalizeBlock, 0, S(stream)>>>(reinterpret_cast<const uint64_t*>(sc.at(kScratchPartials)), static_cast<int>(grid), n, counts2_dev);
    return check_launch("mask_counts(finalize)");
}

extern "C" ec_status ec_mask_counts(const uint8_t* m, size_t n, uint64_t* n_true, uint64_t* n_false, ec_stream stream) {
    EC_REQUIRE_INIT();
    if (!n_true || !n_false) return set_error(EC_ERR_ARG, "ec_mask_counts: null pointer");
    uint64_t counts2[2];
    ec_status st = sync_result(S(stream), kResultWords, counts2, sizeof counts2, [&](const Scratch&, int64_t* words) {
        return ec_mask_counts_device(m, n, reinterpret_cast<uint64_t*>(words), stream);
    });
    if (st != EC_OK) return st;
    *n_true = counts2[0];
    *n_false = counts2[1];
    return EC_OK;
}

// =================================================================== synthetic inputs
template <typename T>
static ec_status synth_t(void* dst, size_t n, uint64_t seed, uint64_t base, double lo, double hi, hipStream_t s) {
    SynthFn<T> fn{static_cast<T*>(dst), seed, base, 1, lo, hi - lo};
    if constexpr (!is_fp<T>::value) fn.span = static_cast<uint64_t>(hi) - static_cast<uint64_t>(lo) + 1;
    return launch_map(fn, n, aligned16(dst, dst, dst), s, "synth_fill");
}

extern "C" ec_status ec_synth_fill(ec_dtype t, void* dst, size_t n, uint64_t seed, uint64_t base, double lo, double hi,
                                   ec_stream stream) {
    EC_REQUIRE_INIT();
    if (n == 0) return EC_OK;
    if (!dst) return set_error(EC_ERR_ARG, "ec_synth_fill: null pointer");
    switch (t) {
        case EC_U8: return synth_t<uint8_t>(dst, n, seed, base, lo, hi, S(stream));
        case EC_U16: return synth_t<uint16_t>(dst, n, seed, base, lo, hi, S(stream));
        case EC_U32: return synth_t<uint32_t>(dst, n, seed, base, lo, hi, S(stream));
        case EC_F32: return synth_t<float>(dst, n, seed, base, lo, hi, S(stream));
        case EC_F64: return synth_t<double>(dst, n, seed, base, lo, hi, S(stream));
    }
    return set_error(EC_ERR_UNSUPPORTED_TYPE, "ec_synth_fill: dtype %d not supported", int(t));
}

extern "C" ec_status ec_synth_mask(uint8_t* dst, size_t n, uint64_t seed, uint64_t base, uint32_t pct_nodata, ec_stream stream) {
    EC_REQUIRE_INIT();
    if (n == 0) return EC_OK;
    if (!dst) return set_error(EC_ERR_ARG, "ec_synth_mask: null pointer");
    SynthMaskFn fn{dst, seed, base, pct_nodata};
    return launch_map(fn, n, aligned16(dst, dst, dst), S(stream), "synth_mask");
}
