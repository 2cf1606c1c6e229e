"""ec_composite_rank restated in numpy (the rule of include/erased_cells.h), the inputs the GPU files use, and models of the mistakes a
selection kernel can make.

`composite_rank(ct, layers, masks, num, den, method, min_count) -> (cells, mask, aux)` is the restatement: the valid layers of every
cell in ascending order of the pair (order_key(cell), k) — two stable sorts, first by key, then by "not valid", so the valid layers
come first in key order with ties by the lesser k — and the one at position r(count) kept, r in Python's integer arithmetic.  It
knows no networks, buckets or sentinels.  `ordered(ct, layers, masks)` is its expensive half, shared by the calls that differ only in
(num, den, method, min_count).  tests/test_composite_rank_ref.py holds it to a scalar transcription, numpy.sort, numpy.median,
composite_ref's MIN and MAX and hand-worked cells.

The inputs are composite_ref's: `stack`, `planted` and `palette`, so ties of identical bits, signed zeros and extremes under cleared
mask bytes are everywhere.  `rank_faulty(kind, ...)` runs the same selection with one mistake in it; tests/test_composite_rank_faults.py
shows that the GPU files' inputs tell each from the right answer.
"""
import numpy as np

import composite_ref as CR
from composite_ref import F32, F64, FLOATS, FORMS, I8, I16, NAMES, NONE, NP, NT, U64, order_key, same_cells, stack, words  # noqa: F401

LOWER, UPPER = 0, 1
METHODS = (LOWER, UPPER)
METHOD_NAMES = ["lower", "upper"]
MAX_DEN = 65535
MAX_LAYERS = CR.MAX_LAYERS
KS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)          # both sides of every bucket edge
QS = ((0, 1), (1, 4), (1, 2), (9, 10), (1, 1))
TRIPLES = ((0, 1, LOWER), (1, 1, UPPER), (1, 2, LOWER), (1, 2, UPPER), (1, 3, LOWER), (1, 3, UPPER), (9, 10, LOWER), (9, 10, UPPER),
           (65535, 65535, LOWER), (65534, 65535, UPPER), (1, 65535, UPPER))


def position(num, den, method, c):
    """r of the header for c >= 1 valid layers"""
    assert 1 <= den <= MAX_DEN and 0 <= num <= den and method in METHODS and c >= 1
    return (num * (c - 1)) // den if method == LOWER else (num * (c - 1) + den - 1) // den


def positions(num, den, method, count):
    """r per cell; 0 where no layer is valid (nothing of the stack is stored there)"""
    table = np.array([0] + [position(num, den, method, c) for c in range(1, MAX_LAYERS + 1)], np.int64)
    return table[count]


def bucket(k):
    """the stack's height rounded up to a power of two (rank_bucket of ec_composite_rank_cell.hpp)"""
    b = 1
    while b < k:
        b *= 2
    return b


def group_cells(ct, k):
    """rank_group of ec_composite_rank_kernels.hpp: cells per lane per group of the kernel that serves (ct, k)"""
    size = NP[ct].itemsize
    regs = 1 if size <= 2 else 2 if size == 4 else 3
    g = 16 // size
    while g > 1 and g * bucket(k) * regs > 64:
        g //= 2
    return 4 if size <= 2 and bucket(k) == 32 else g


def tile_cells(ct, k):
    return 256 * group_cells(ct, k)


def _valid(layers, masks):
    n = layers[0].size
    masks = [None] * len(layers) if masks is None else masks
    return np.stack([np.ones(n, bool) if m is None else (np.asarray(m) != 0) for m in masks])


def _order(key, valid, descending_k=False):
    """(K, n) layer indices: the valid layers first, ascending by (key, k) — or by (key, -k), a fault model's order"""
    if descending_k:
        first = key.shape[0] - 1 - np.argsort(key[::-1], axis=0, kind="stable")
    else:
        first = np.argsort(key, axis=0, kind="stable")
    invalid = ~np.take_along_axis(valid, first, axis=0)
    return np.take_along_axis(first, np.argsort(invalid, axis=0, kind="stable"), axis=0)


def ordered(ct, layers, masks):
    """(order[K, n], count[n], bits[K, n]): the layers of every cell in the rule's order (the count valid ones first)"""
    valid = _valid(layers, masks)
    key = np.stack([order_key(ct, a) for a in layers])
    return _order(key, valid), valid.sum(axis=0), np.stack([words(a) for a in layers])


def pick(ct, od, num, den, method, min_count):
    order, count, bits = od
    assert 1 <= min_count <= order.shape[0]
    r = positions(num, den, method, count)
    k = np.take_along_axis(order, r[None, :], axis=0)[0]
    ok = count >= min_count
    cells = np.where(ok, np.take_along_axis(bits, k[None, :], axis=0)[0], 0).astype(bits.dtype).view(NP[ct])
    return cells, ok.astype(np.uint8), np.where(ok, k, NONE).astype(np.uint8)


def composite_rank(ct, layers, masks, num, den, method, min_count):
    """(cells of type ct, mask bytes, aux bytes) of ec_composite_rank"""
    assert 1 <= len(layers) <= MAX_LAYERS
    return pick(ct, ordered(ct, layers, masks), num, den, method, min_count)


# ---- the mistakes
FAULTS = ("mask_ignored", "invalid_takes_part", "tie_to_higher", "ieee_less", "raw_float_bits", "u64_signed", "sign_bias_forgotten",
          "rank_from_k", "lower_upper_swapped", "upper_is_lower", "position_from_c", "sentinel_counted", "last_layer_dropped",
          "layer_index_truncated", "min_count_ignored", "aux_from_first_tie", "tail_skipped")


def applies(kind, ct, k, form, num, den, method, min_count):
    """can this mistake show at all in a launch of this shape?"""
    masked = form != "none"
    inner = 0 < num < den
    if kind in ("mask_ignored", "invalid_takes_part"):
        return masked
    if kind == "tie_to_higher":
        return k >= 2
    if kind in ("ieee_less", "raw_float_bits"):
        return ct in FLOATS and k >= 2
    if kind == "u64_signed":
        return ct == U64 and k >= 2
    if kind == "sign_bias_forgotten":
        return ct in (I8, I16) and k >= 2
    if kind == "rank_from_k":
        return masked and k >= 2 and num > 0
    if kind in ("lower_upper_swapped", "upper_is_lower"):
        return inner and k >= 2 and (kind == "lower_upper_swapped" or method == UPPER)
    if kind == "position_from_c":
        return inner and k >= 2
    if kind == "sentinel_counted":
        return bucket(k) != k and num > 0
    if kind == "last_layer_dropped":
        return k >= 2 and bucket(k - 1) == k - 1
    if kind == "layer_index_truncated":
        return k > 32
    if kind == "min_count_ignored":
        return min_count >= 2 and masked
    if kind == "aux_from_first_tie":
        return k >= 2 and num > 0
    if kind == "tail_skipped":
        return True
    raise KeyError(kind)


def rank_faulty(kind, ct, layers, masks, num, den, method, min_count, arg=None):
    """what a kernel with the mistake `kind` stores.  `arg`: the layer whose mask is ignored ("mask_ignored")."""
    k_layers, n = len(layers), layers[0].size
    masks = [None] * k_layers if masks is None else list(masks)
    if kind == "mask_ignored":
        masks[arg] = None
    valid = _valid(layers, masks)
    if kind == "last_layer_dropped":
        valid[k_layers - 1] = False
    key = np.stack([order_key(ct, a) for a in layers])
    bits = np.stack([words(a) for a in layers])
    if kind == "ieee_less" and ct in FLOATS:                    # IEEE `<` cannot tell -0.0 from +0.0: they tie, and k decides
        key = np.stack([order_key(ct, np.where(a == 0, np.zeros(1, a.dtype), a)) for a in layers])
    elif kind == "raw_float_bits" and ct in FLOATS:
        key = bits.view(np.int32 if ct == F32 else np.int64).astype(np.int64)
    elif kind == "u64_signed" and ct == U64:
        key = bits.view(np.int64)
    elif kind == "sign_bias_forgotten" and ct in (I8, I16):
        key = bits.astype(np.int64)
    sort_valid = np.ones_like(valid) if kind == "invalid_takes_part" else valid
    if kind == "layer_index_truncated":                         # five bits of k in the packed word: ties and aux by k mod 32
        low = (np.arange(k_layers) % 32)[:, None]
        first = np.lexsort((np.broadcast_to(low, key.shape), key), axis=0)
        invalid = ~np.take_along_axis(valid, first, axis=0)
        order = np.take_along_axis(first, np.argsort(invalid, axis=0, kind="stable"), axis=0)
    else:
        order = _order(key, sort_valid, descending_k=kind == "tie_to_higher")
    count = valid.sum(axis=0)
    c = count
    if kind == "rank_from_k":
        c = np.full(n, k_layers)
    elif kind == "sentinel_counted":
        c = np.minimum(count + (bucket(k_layers) - k_layers), k_layers)
    m = method
    if kind == "lower_upper_swapped":
        m = 1 - method
    elif kind == "upper_is_lower":
        m = LOWER
    if kind == "position_from_c":
        r = np.array([0] + [min(position(num, den, m, x + 1), x - 1) for x in range(1, MAX_LAYERS + 1)], np.int64)[c]
    else:
        r = positions(num, den, m, c)
    k = np.take_along_axis(order, r[None, :], axis=0)[0]
    ok = count >= (1 if kind == "min_count_ignored" else min_count)
    cells = np.where(ok, np.take_along_axis(bits, k[None, :], axis=0)[0], 0).astype(bits.dtype)
    aux_k = k % 32 if kind == "layer_index_truncated" else k
    if kind == "aux_from_first_tie":                            # the bits are right, the aux byte names the first valid layer of that key
        picked = np.take_along_axis(key, k[None, :], axis=0)[0]
        aux_k = np.argmax(valid & (key == picked[None, :]), axis=0)
    mask, aux = ok.astype(np.uint8), np.where(ok, aux_k, NONE).astype(np.uint8)
    if kind == "tail_skipped":                                   # the cells behind the last whole group keep what the buffers held: zeros
        first_tail = n - n % group_cells(ct, k_layers)
        cells[first_tail:], mask[first_tail:], aux[first_tail:] = 0, 0, 0
    return cells.view(NP[ct]), mask, aux


# ---- inputs
def main_len(ct):
    """n of the main GPU cases of one cell type, whatever the stack's height: two whole tiles of the largest group (16 bytes a
    lane), a guarded last tile behind them, and 15 cells behind the last 16-cell group, a partial last group at every cells-per-lane"""
    n = 2 * 256 * (16 // NP[ct].itemsize) + 1027 + 15
    return n - (n - 15) % 16


def small_lengths(ct, k):
    """1, one group less a cell, one tile and its neighbours, three tiles and a partial group"""
    t, g = tile_cells(ct, k), group_cells(ct, k)
    return sorted({1, max(g - 1, 1), t - 1, t, t + 1, 3 * t + max(g - 1, 1)})


def min_counts(k):
    return sorted({1, (k + 1) // 2, k})
