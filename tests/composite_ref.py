"""ec_composite restated in numpy (the rule of include/erased_cells.h), the inputs the GPU files use, and models of the mistakes a
composite kernel can make.

`composite(op, ct, layers, masks, min_count) -> (cells, mask, aux)` is the restatement: whole-array numpy, one layer at a time in
ascending k.  numpy's int64 / uint64 -> float64 conversion is the C cast (round to nearest even) and its float64 addition is one
IEEE operation, so SUM and MEAN are the rule exactly; FIRST / LAST / MIN / MAX move cells as unsigned words, so every bit pattern
survives.  tests/test_composite_ref.py holds it to a scalar transcription, hand-worked cells and the oracle.

`stack(ct, k, n, form)` is what the GPU files composite.  It draws every cell from a short per-type palette, so ties of identical
bits, signed zeros, extremes under cleared mask bytes and sums whose order changes their bits are everywhere, and it plants the
cells listed at `planted` at the head and in the ragged tail.  For cell types of 32 bits or fewer the sum of 64 cells is
exact in f64 (64 * 2^32 < 2^53), so no order of additions can change its bits: only f32, f64, i64 and u64 carry order-sensitive
magnitudes.  For 16 bits or fewer it is exact in f32 as well (64 * 65535 < 2^24).

`composite_faulty(kind, ...)` runs the same fold with one mistake in it; tests/test_composite_faults.py shows that the GPU files'
inputs tell each from the right answer.
"""
import numpy as np

U8, U16, U32, U64, I8, I16, I32, I64, F32, F64 = range(10)
NT = 10
NAMES = ["u8", "u16", "u32", "u64", "i8", "i16", "i32", "i64", "f32", "f64"]
NP = [np.dtype(d) for d in (np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64)]
FIRST, LAST, MIN, MAX, SUM, MEAN = range(6)
OPS = (FIRST, LAST, MIN, MAX, SUM, MEAN)
OP_NAMES = ["first", "last", "min", "max", "sum", "mean"]
NONE = 255
MAX_LAYERS = 64
FLOATS = (F32, F64)
BATCH = 4                                                  # kCompositeBatch of ec_composite_kernels.hpp (test_composite_args.py reads it)
KS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 63, 64)              # both sides of every plausible batch size
FORMS = ("none", "all", "some")


def sums(op):
    return op in (SUM, MEAN)


def result_type(op, ct):
    return F64 if sums(op) else ct


def cpl(op, ct):
    """cells per group of the kernel that serves (op, ct): 16 / max(cell bytes, result cell bytes)"""
    return 16 // (8 if sums(op) else NP[ct].itemsize)


def groups_per_lane(op, ct):
    """composite_u of ec_composite_kernels.hpp"""
    return 2 if sums(op) else (1 if NP[ct].itemsize == 1 else 2)


def tile_cells(op, ct):
    return 256 * groups_per_lane(op, ct) * cpl(op, ct)


def words(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def order_key(ct, x):
    """int64 keys whose natural order is the reference's (src/value.rs:248-265): ints natural, floats total_cmp"""
    x = np.ascontiguousarray(x)
    if ct == U64:
        return (x ^ np.uint64(1 << 63)).view(np.int64)
    if ct not in FLOATS:
        return x.astype(np.int64)
    b = x.view(np.int32 if ct == F32 else np.int64).astype(np.int64)
    width = 31 if ct == F32 else 63
    return b ^ ((b >> width) & ((1 << width) - 1))


def to_f64(ct, x, truncate=False):
    """double(cell): the rounding conversion; `truncate` is the fault model's round-toward-zero of a 64-bit integer"""
    r = x.astype(np.float64)
    if truncate and ct in (I64, U64):
        exact = x.astype(np.longdouble)                    # 64 mantissa bits: every 64-bit integer exactly
        assert np.finfo(np.longdouble).nmant >= 63
        r = np.where(np.abs(r.astype(np.longdouble)) > np.abs(exact), np.nextafter(r, 0.0), r)
    return r


def _valid(layers, masks):
    n = layers[0].size
    masks = [None] * len(layers) if masks is None else masks
    return [np.ones(n, bool) if m is None else (np.asarray(m) != 0) for m in masks]


def _fold(op, ct, layers, valid, min_count, fault=None, arg=None):
    """the fold over the layers given, with at most one modelled mistake"""
    dt, k_layers, n = NP[ct], len(layers), layers[0].size
    count = np.zeros(n, np.uint32)
    for v in valid:
        count += v
    ok = count > min_count if fault == "count_gt" else count >= min_count
    if not sums(op):
        pick_op = LAST if (fault == "first_picks_last" and op == FIRST) else op
        val, idx, have = np.zeros(n, words(layers[0]).dtype), np.full(n, NONE, np.uint8), np.zeros(n, bool)
        for k in range(k_layers):
            x, v = layers[k], valid[k]
            if pick_op == FIRST:
                take = v & ~have
            elif pick_op == LAST:
                take = v.copy()
            else:
                cur = val.view(dt)
                if fault == "ieee_less" and ct in FLOATS:
                    with np.errstate(invalid="ignore"):
                        better = x > cur if op == MAX else x < cur
                elif fault == "raw_float_bits" and ct in FLOATS:
                    a, b = words(x).view(np.int32 if ct == F32 else np.int64), val.view(np.int32 if ct == F32 else np.int64)
                    better = a > b if op == MAX else a < b
                elif fault == "u64_signed" and ct == U64:
                    a, b = x.view(np.int64), cur.view(np.int64)
                    better = a > b if op == MAX else a < b
                else:
                    a, b = order_key(ct, x), order_key(ct, cur)
                    if fault == "tie_to_higher":
                        better = a >= b if op == MAX else a <= b
                    else:
                        better = a > b if op == MAX else a < b
                take = v & (~have | better)
            val = np.where(take, words(x), val)
            idx = np.where(take, np.uint8((k % arg) if fault == "aux_index_in_batch" else k), idx)
            have |= v
        zero = ok if fault != "invalid_not_zeroed" else np.ones(n, bool)
        cells = np.where(zero, val, 0).astype(val.dtype).view(dt)
        aux = idx if fault == "invalid_aux_not_255" else np.where(ok, idx, NONE).astype(np.uint8)
        return cells, ok.astype(np.uint8), aux
    order = range(k_layers - 1, -1, -1) if fault == "sum_descending" else range(k_layers)
    acc = np.zeros(n, np.float32 if fault == "sum_in_f32" else np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in order:
            d = to_f64(ct, layers[k], truncate=fault == "int64_truncated")
            a = acc + (d.astype(np.float32) if fault == "sum_in_f32" else d)
            acc = a if fault == "sum_adds_invalid" else np.where(valid[k], a, acc)
    acc = acc.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = acc / (np.float64(k_layers) if fault == "mean_divides_by_k" else count.astype(np.float64)) if op == MEAN else acc
    zero = ok if fault != "invalid_not_zeroed" else np.ones(n, bool)
    return np.where(zero, r, 0.0), ok.astype(np.uint8), count.astype(np.uint8)


def composite(op, ct, layers, masks, min_count):
    """(cells of result_type(op, ct), mask bytes, aux bytes) of ec_composite"""
    assert 1 <= len(layers) <= MAX_LAYERS and 1 <= min_count <= len(layers)
    return _fold(op, ct, layers, _valid(layers, masks), min_count)


# ---- the mistakes: name -> what it takes to apply
FAULTS = ("mask_ignored", "null_mask_takes_neighbour", "first_picks_last", "tie_to_higher", "ieee_less", "raw_float_bits", "u64_signed",
          "sum_descending", "sum_in_f32", "int64_truncated", "sum_adds_invalid", "mean_divides_by_k", "count_gt", "invalid_not_zeroed",
          "invalid_aux_not_255", "aux_index_in_batch", "tail_layers_skipped_2", "tail_layers_skipped_4", "tail_layers_skipped_8",
          "tail_without_masks")


def applies(kind, op, ct, k, form, min_count):
    """can this mistake show at all in a launch of this shape?"""
    masked = form != "none"
    if kind == "mask_ignored":
        return masked
    if kind == "null_mask_takes_neighbour":
        return form == "some" and k >= 2
    if kind == "first_picks_last":
        return op == FIRST and k >= 2
    if kind == "tie_to_higher":
        return op in (MIN, MAX) and k >= 2
    if kind in ("ieee_less", "raw_float_bits"):
        return op in (MIN, MAX) and ct in FLOATS and k >= 2
    if kind == "u64_signed":
        return op in (MIN, MAX) and ct == U64 and k >= 2
    if kind == "sum_descending":
        return sums(op) and ct in (F32, F64, I64, U64) and k >= 3
    if kind == "sum_in_f32":
        return sums(op) and NP[ct].itemsize >= 4 and k >= 2
    if kind == "int64_truncated":
        return sums(op) and ct in (I64, U64)
    if kind == "sum_adds_invalid":
        return sums(op) and masked
    if kind == "mean_divides_by_k":
        return op == MEAN and masked and k >= 2
    if kind == "count_gt":
        return masked or min_count == k
    if kind in ("invalid_not_zeroed", "invalid_aux_not_255"):
        # a cell with 0 < count < min_count: with min_count == 1 an invalid cell has picked nothing and is zero / 255 anyway
        return masked and min_count >= 2 and (kind == "invalid_not_zeroed" or not sums(op))
    if kind == "aux_index_in_batch":
        return not sums(op) and k > BATCH
    if kind.startswith("tail_layers_skipped_"):
        return k % int(kind.rsplit("_", 1)[1]) != 0
    if kind == "tail_without_masks":
        return masked
    raise KeyError(kind)


def composite_faulty(kind, op, ct, layers, masks, min_count, arg=None):
    """what a kernel with the mistake `kind` stores.  `arg`: the layer whose mask is ignored ("mask_ignored")."""
    k_layers, n = len(layers), layers[0].size
    masks = [None] * k_layers if masks is None else list(masks)
    if kind == "mask_ignored":
        masks[arg] = None
    elif kind == "null_mask_takes_neighbour":               # the mask registers of the layer before are still there
        last = None
        for k in range(k_layers):
            if masks[k] is None:
                masks[k] = last
            else:
                last = masks[k]
    valid = _valid(layers, masks)
    if kind.startswith("tail_layers_skipped_"):
        b = int(kind.rsplit("_", 1)[1])
        keep = k_layers - k_layers % b
        # the layers past the last whole batch contribute nothing, not even to the count (aux of SUM)
        for k in range(keep, k_layers):
            valid[k] = np.zeros(n, bool)
        return _fold(op, ct, layers, valid, min_count)
    if kind == "tail_without_masks":
        first_tail = n - n % cpl(op, ct)
        for v in valid:
            v[first_tail:] = True
        return _fold(op, ct, layers, valid, min_count)
    if kind == "aux_index_in_batch":
        return _fold(op, ct, layers, valid, min_count, kind, BATCH)
    return _fold(op, ct, layers, valid, min_count, kind)


def same_cells(got, want, nan_by_class=False):
    """per cell: bit-equal; with nan_by_class two NaNs are equal (which payload an addition keeps is the processor's choice)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    ok = words(got) == words(want)
    if nan_by_class and want.dtype.kind == "f":
        ok |= np.isnan(got) & np.isnan(want)
    return ok


# ---- inputs
def palette(ct):
    """the values a stack draws from: few enough that valid layers tie on identical bits, with the extremes, and — f32, f64, i64, u64 —
    magnitudes whose f64 sum depends on the order of the additions"""
    dt = NP[ct]
    if ct in FLOATS:
        big = 2.0 ** 60 if ct == F32 else 1.0e16
        # no infinities: inf + -inf would be a NaN in a strict comparison (max + max overflows to one infinity and stays there)
        return np.array([0.0, -0.0, 1.0, -1.0, 3.0, 0.1, -2.5, big, -big, big / 3, np.finfo(dt).max, -np.finfo(dt).max, np.finfo(dt).tiny, 128.0], dt)
    lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
    vals = [0, 1, 2, 3, 7, hi, hi - 1, hi // 2, hi // 2 + 1, hi // 3]
    if lo < 0:
        vals += [lo, lo + 1, -1, -2, lo // 3]
    if ct in (I64, U64):
        vals += [(1 << 53) + 1, (1 << 53) + 3, (1 << 62) + 1025, (1 << 60) + 513]   # above 2^53: double() rounds, and the sum's order shows
    return np.array(vals, dt)


def nan_of(ct, payload=0x1234):
    b = (0x7fc00000 | payload) if ct == F32 else (0x7ff8000000000000 | payload)
    return np.array([b], np.uint32 if ct == F32 else np.uint64).view(NP[ct])[0]


def planted(ct, k):
    """(values[k, P], masks[k, P]) of the P planted cells, in this order:
       0  no valid layer                          1  only the last layer valid
       2  an invalid layer holds the maximum      3  an invalid layer holds the minimum
       4  the maximum twice among valid layers    5  the minimum twice among valid layers
       6  floats: +0.0 then -0.0 valid            7  floats: -0.0 then +0.0 valid
       8  a sum whose order changes its bits (f32, f64, i64, u64; three layers at least)
       9  exactly one valid layer, the first      10 a NaN under a cleared mask byte (floats), else as 2"""
    dt, pal = NP[ct], palette(ct)
    if ct in FLOATS:
        vmax, vmin, mid = pal[10], pal[11], pal[2]
    else:
        vmax, vmin, mid = np.iinfo(dt).max, np.iinfo(dt).min, dt.type(np.iinfo(dt).max // 2)
    v = np.full((k, 11), mid, dt)
    m = np.ones((k, 11), np.uint8)
    m[:, 0] = 0
    m[:, 1] = 0
    m[k - 1, 1] = 1
    v[0, 1] = vmax
    if k >= 2:
        v[k // 2, 2], m[k // 2, 2] = vmax, 0
        v[k // 2, 3], m[k // 2, 3] = vmin, 0
        v[0, 4], v[k - 1, 4] = vmax, vmax
        v[0, 5], v[k - 1, 5] = vmin, vmin
        if ct in FLOATS:
            v[:, 6], v[:, 7] = 1.0, -1.0
            v[0, 6], v[1, 6] = 0.0, -0.0
            v[0, 7], v[1, 7] = -0.0, 0.0
            v[k - 1, 10], m[k - 1, 10] = nan_of(ct), 0
        else:
            v[k - 1, 10], m[k - 1, 10] = vmax, 0
    if k >= 3 and ct in (F32, F64, I64, U64):
        if ct in FLOATS:
            v[:, 8] = 0.0
            half = 128.0 if ct == F32 else 1.0                     # half an ulp of big in f64: 2^60 for f32 cells, 1e16 for f64 cells
            v[0, 8], v[1, 8], v[k - 1, 8] = pal[7], half, half     # (big + half) + half == big, (half + half) + big == big + ulp
        else:
            v[:, 8] = 0
            v[0, 8], v[1, 8], v[k - 1, 8] = (1 << 53), 1, 1
    m[1:, 9] = 0
    return v, m


def stack(ct, k, n, form, seed=0):
    """(layers, masks) of a GPU case: k layers of n cells; masks None (form "none"), one per layer ("all"), or with the entries of
    the layers k % 3 == 1 None ("some").  The planted cells sit at the head and — again — in the last cells, which are the ragged
    tail; they keep their planted mask bytes under every form that has the mask."""
    assert form in FORMS
    rng = np.random.default_rng([9700 + seed, ct, k, n])
    pal = palette(ct)
    vals = pal[rng.integers(0, pal.size, size=(k, n))]
    mk = (rng.random((k, n)) < 0.6).astype(np.uint8)
    if ct in FLOATS:                                          # whatever lies under a cleared mask byte must not matter: NaNs there
        hole = (mk == 0) & (rng.random((k, n)) < 0.25)
        vals[hole] = nan_of(ct)
    pv, pm = planted(ct, k)
    p = pv.shape[1]
    if n >= p:
        vals[:, :p], mk[:, :p] = pv, pm
    if n >= 3 * p:
        vals[:, n - p:], mk[:, n - p:] = pv, pm
    layers = [np.ascontiguousarray(vals[i]) for i in range(k)]
    if form == "none":
        if ct in FLOATS:                                      # every cell is valid: no NaNs at all (strict comparison of sums)
            for a in layers:
                a[np.isnan(a)] = pal[5]
        return layers, None
    masks = [np.ascontiguousarray(mk[i]) for i in range(k)]
    if form == "some":
        for i in range(k):
            if i % 3 == 1:
                masks[i] = None
                if ct in FLOATS:
                    layers[i][np.isnan(layers[i])] = pal[5]
    return layers, masks


def main_len(ct):
    """n of the main GPU cases, one per cell type for all ops: two whole tiles of the op with the largest tile, a guarded last tile
    behind them, and — tail_len of tests/compare_ref.py — 15 cells behind the last 16-cell group, a partial last group at every CPL"""
    n = 2 * max(tile_cells(op, ct) for op in OPS) + 1027 + 15
    return n - (n - 15) % 16


def small_lengths(op, ct):
    """1, CPL - 1, one tile and its neighbours"""
    t, c = tile_cells(op, ct), cpl(op, ct)
    return sorted({1, max(c - 1, 1), t - 1, t, t + 1})


def min_counts(k):
    return sorted({1, min(2, k), k})
