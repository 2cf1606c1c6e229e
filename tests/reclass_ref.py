"""The reclassification rule of include/erased_cells.h (ec_reclass_table_build, ec_reclass) restated in numpy, for the tests.

`classes` does NOT use thresholds: a cell's class is the sum over the breaks of the union-order predicate — both converted to
CellType::union of their types, integers compared naturally, floats by total_cmp (compare_ref.total_key) — so the thresholds
the library derives on the host are tested against something that never heard of them.  `reclass` is built on it.
tests/test_reclass_ref.py holds `classes` to a scalar transcription of the rule, to compare_ref.relation (which the oracle holds)
and to numpy.digitize.

Also here: the record's layout (to read what the builder wrote), the kernels' launch constants restated, the inputs of the GPU
tests (`gpu_inputs`, `gpu_tables`, `gpu_masks`, `tail_len`) and numpy models of the mistakes a reclass kernel or its table can
make (tests/test_reclass_faults.py).  Imports nothing from the library.
"""
import numpy as np

import compare_ref as R
from compare_ref import F32, F64, I8, I16, I32, I64, NAMES, NP, NT, U8, U16, U32, U64, specials, tail_len, total_key, union  # noqa: F401

MAX_BREAKS, TABLE_BYTES = 255, 4384
HAS_NODATA, DROPS = 1, 2
BLOCK, U = 256, 2   # threads of a workgroup, groups per lane of a tile (the default map_u)
TABLE = np.dtype([("t", "<i4"), ("dt", "<i4"), ("n_breaks", "<i4"), ("n_reached", "<i4"), ("flags", "<u4"), ("reserved0", "<u4"),
                  ("nodata_bits", "<u8"), ("reserved1", "<u8"), ("thr", "<i8", (255,)), ("value_bits", "<u8", (256,)), ("valid", "u1", (256,))])
assert TABLE.itemsize == TABLE_BYTES
WORD = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def size_of(ct):
    return NP[ct].itemsize


def cpl(t, dt):
    return 16 // max(size_of(t), size_of(dt))


def tile(t, dt):
    """cells one workgroup takes"""
    return BLOCK * U * cpl(t, dt)


def search_steps(n_reached):
    return int(n_reached).bit_length()


# ---------------------------------------------------------------- the rule
def _in_union(t, x, bt, b):
    u = NP[union(t, bt)]
    with np.errstate(all="ignore"):
        a, b = np.atleast_1d(np.asarray(x, dtype=NP[t])).astype(u), np.atleast_1d(np.asarray(b, dtype=NP[bt])).astype(u)   # `as`: every pair widens
    if u.kind == "f":
        a, b = total_key(a), total_key(b)
    return a, b


def breaks_refusal(t, bt, breaks):
    """why the builder must refuse these breaks, or None"""
    b = np.asarray(breaks, dtype=NP[bt])
    if NP[bt].kind == "f" and np.isnan(b).any():
        return "NaN"
    _, k = _in_union(t, np.zeros(0, NP[t]), bt, b)
    return None if np.all(k[1:] > k[:-1]) else "ascending"


def classes(t, x, bt, breaks, right):
    """c[i] = #{ j : b[j] <= x[i] } (right: <) under the order of the union type, as int32"""
    a, b = _in_union(t, x, bt, breaks)
    c = np.zeros(a.shape, np.int32)
    for bj in b:
        c += (a > bj) if right else (a >= bj)
    return c


def reclass(t, x, mask, bt, breaks, right, dt, values, valid=None, nodata=None):
    """(dst, dst_mask) of ec_reclass: dst of numpy type NP[dt], dst_mask one byte per cell (what the call writes when asked to)"""
    values = np.asarray(values, dtype=NP[dt])
    assert values.size == len(breaks) + 1 and (mask is None) == (nodata is None)
    c = classes(t, x, bt, breaks, right)
    dst = values[c]
    ok = np.ones(c.shape, np.uint8) if valid is None else (np.asarray(valid)[c] != 0).astype(np.uint8)
    if mask is not None:
        m = np.asarray(mask) != 0
        dst = np.where(m, dst, NP[dt].type(nodata)).astype(NP[dt])
        ok = ok & m.astype(np.uint8)
    return dst, ok


# ---------------------------------------------------------------- the record
def order_key(t, x):
    """ec_order_key.hpp order_key<T> as int64"""
    a = np.atleast_1d(np.asarray(x, dtype=NP[t]))
    if NP[t].kind == "f":
        return total_key(a).astype(np.int64)
    if t == U64:
        return (a ^ np.uint64(1 << 63)).view(np.int64)
    return a.astype(np.int64)


def parse(blob: bytes):
    assert len(blob) == TABLE_BYTES
    return np.frombuffer(blob, dtype=TABLE)[0]


def classes_through(tab, t, x):
    """the class the kernels compute from a record: #{ j < n_reached : thr[j] <= key(x) }"""
    thr = tab["thr"][:int(tab["n_reached"])]
    return np.searchsorted(thr, order_key(t, x), side="right").astype(np.int32)


def value_slots(tab, dt):
    return tab["value_bits"].astype(WORD[size_of(dt)]).view(NP[dt])


# ---------------------------------------------------------------- inputs of the GPU tests
def gpu_tables(t, bt, n_breaks, seed=0):
    """n_breaks breaks of type bt, strictly ascending in the union with t: drawn from random cells of t (as bt, so that cells tie
    with breaks) and of bt, NaNs dropped, one per union key, evenly thinned.  Fewer come back when bt has fewer distinct values."""
    from vectors import rand_cells
    with np.errstate(all="ignore"):
        cand = np.concatenate([rand_cells(t, 3000, 9500 + seed, specials=False).astype(NP[bt]), rand_cells(bt, 3000, 9600 + seed, specials=False),
                               specials(bt)])
    if NP[bt].kind == "f":
        cand = cand[~np.isnan(cand)]
    _, k = _in_union(t, np.zeros(0, NP[t]), bt, cand)
    _, first = np.unique(k, return_index=True)
    cand = cand[first]                                 # ascending in the union, one per key
    if cand.size > n_breaks:
        cand = cand[np.linspace(0, cand.size - 1, n_breaks).astype(np.int64)]
    assert breaks_refusal(t, bt, cand) is None
    return cand


def neighbours(t, x):
    """the cells of type t just below and above each cell of x in t's order (saturating at the ends)"""
    k = order_key(t, x)
    lo, hi = order_key(t, key_ends(t)[0])[0], order_key(t, key_ends(t)[1])[0]
    return np.concatenate([from_key(t, np.where(k > lo, k - 1, k)), from_key(t, np.where(k < hi, k + 1, k))])


def key_ends(t):
    """the least and greatest cell of type t in the total order"""
    if NP[t].kind == "f":
        ut = np.uint32 if t == F32 else np.uint64
        return np.array([~ut(0)], ut).view(NP[t])[0], np.array([np.iinfo(ut).max >> 1], ut).view(NP[t])[0]   # -NaN, +NaN with full payloads
    return np.iinfo(NP[t]).min, np.iinfo(NP[t]).max


def from_key(t, k):
    """key_value<T>: the cell of an order key"""
    k = np.asarray(k, dtype=np.int64)
    if NP[t].kind == "f":
        it = np.int32 if t == F32 else np.int64
        k = k.astype(it)
        return (k ^ ((k >> (8 * NP[t].itemsize - 1)) & np.iinfo(it).max)).view(NP[t])
    if t == U64:
        return k.view(np.uint64) ^ np.uint64(1 << 63)
    return k.astype(NP[t])


def special_cells(t):
    """the planted cells of the wide types: the type's table (NaNs of both signs, +-0.0, +-inf, the limits), 2^24 +- 1, 2^53 +- 1"""
    extra = [2**24 - 1, 2**24, 2**24 + 1, 2**53 - 1, 2**53, 2**53 + 1]
    if NP[t].kind == "f":
        more = np.array([float(v) for v in extra] + [-float(v) for v in extra], dtype=NP[t])
    else:
        info = np.iinfo(NP[t])
        more = np.array([v for v in extra + [-v for v in extra] if info.min <= v <= info.max], dtype=object).astype(NP[t])
    return np.concatenate([specials(t), more])


def gpu_inputs(t, bt, breaks, n_random=4099, seed=0):
    """The cells a GPU test classifies: the special cells, every break as a cell of t with its two neighbours in t's order,
    at least 20 cells that tie with a break where t holds one, and random cells."""
    from vectors import rand_cells
    b = np.asarray(breaks, dtype=NP[bt])
    with np.errstate(all="ignore"):
        as_t = b.astype(NP[t])
    ties = as_t[R.cmp3(t, as_t, bt, b) == 0]           # breaks that a cell of t equals
    planted = np.concatenate([as_t, neighbours(t, as_t), np.resize(ties, max(20, ties.size)) if ties.size else as_t[:0]])
    return np.concatenate([special_cells(t), planted, rand_cells(t, n_random, 9400 + seed, specials=False)])


def gpu_masks(n, seed=0):
    """a random mask, valid over the last 15 cells (the ragged tail) and with both values among the first 16"""
    from vectors import rand_mask
    m = rand_mask(n, 9700 + seed)
    m[-15:] = 1
    m[:2] = (0, 1)
    return m


# ---------------------------------------------------------------- modelled mistakes
ORDER_FAULTS = ("f64_whatever_the_union", "signed_compare_of_u64_keys", "raw_float_bits", "ieee_compare", "right_ignored")
TABLE_FAULTS = ("search_drops_the_last_threshold", "search_drops_the_first_threshold", "searches_n_breaks_not_n_reached", "int32_keys_for_an_8_byte_type",
                "values_c_minus_1", "valid_ignored", "input_mask_ignored_in_dst_mask", "nodata_not_written", "value_slot_at_the_wrong_width",
                "lut_indexed_by_the_signed_cell", "tail_group_as_a_full_one")


def applies(kind, t, bt, dt=U8):
    u = union(t, bt)
    return {"f64_whatever_the_union": u in (U64, I64) and size_of(t) == 8, "signed_compare_of_u64_keys": u == U64 or t == U64,
            "raw_float_bits": NP[u].kind == "f" and (NP[t].kind == "f" or t in (I8, I16, I32, I64)), "ieee_compare": NP[t].kind == "f",
            "int32_keys_for_an_8_byte_type": size_of(t) == 8, "lut_indexed_by_the_signed_cell": t == I8,
            "value_slot_at_the_wrong_width": size_of(dt) > 1}.get(kind, True)


def classes_faulty(kind, t, x, bt, breaks, right):
    """`classes` with a mistake in the order"""
    if kind == "right_ignored":
        return classes(t, x, bt, breaks, False)
    u = NP[union(t, bt)]
    with np.errstate(all="ignore"):
        a, b = np.asarray(x, dtype=NP[t]), np.asarray(breaks, dtype=NP[bt])
        if kind == "f64_whatever_the_union":
            a, b = total_key(a.astype(np.float64)), total_key(b.astype(np.float64))
        elif kind == "signed_compare_of_u64_keys":
            a, b = a.astype(u), b.astype(u)
            a, b = (a.view(np.int64), b.view(np.int64)) if u == np.uint64 else (total_key(a), total_key(b)) if u.kind == "f" else (a, b)
        elif kind == "raw_float_bits":
            it = np.int32 if u.itemsize == 4 else np.int64
            a, b = a.astype(u).view(it), b.astype(u).view(it)
        elif kind == "ieee_compare":
            a, b = a.astype(u), b.astype(u)
        else:
            raise KeyError(kind)
        c = np.zeros(a.shape, np.int32)
        for bj in b:
            c += (a > bj) if right else (a >= bj)
    return c


def kernel_model(kind, tab, t, x, mask, dt, want_mask=True):
    """What a kernel with mistake `kind` (None: none) makes of the record `tab` (parse): (dst, dst_mask)."""
    nr, nb = int(tab["n_reached"]), int(tab["n_breaks"])
    thr, key = tab["thr"], order_key(t, x)
    if kind == "int32_keys_for_an_8_byte_type":
        thr, key = thr.astype(np.int32).astype(np.int64), key.astype(np.int32).astype(np.int64)
    if kind == "lut_indexed_by_the_signed_cell":   # the LUT built right over the 256 bytes, read at the SIGNED cell (clamped into it)
        lut = np.searchsorted(thr[:nr], order_key(t, np.arange(256, dtype=np.uint8).view(NP[t])), side="right")
        c = lut[np.clip(np.asarray(x, dtype=NP[t]).astype(np.int64), 0, 255)]
    elif kind == "search_drops_the_last_threshold":
        c = np.searchsorted(thr[:max(nr - 1, 0)], key, side="right")
    elif kind == "search_drops_the_first_threshold":
        c = np.searchsorted(thr[1:nr], key, side="right")
    elif kind == "searches_n_breaks_not_n_reached":
        c = np.zeros(key.shape, np.int64)
        for j in range(nb):                         # the slots past n_reached hold 0: not sorted, so a plain count
            c += thr[j] <= key
    else:
        c = np.searchsorted(thr[:nr], key, side="right")
    c = np.asarray(c, dtype=np.int64)
    w = size_of(dt)
    slots = tab["value_bits"].astype(WORD[w])
    if kind == "value_slot_at_the_wrong_width":     # the table read as packed cells of the output's width
        slots = np.ascontiguousarray(tab["value_bits"]).view(WORD[w])[:256]
    idx = np.clip(c - 1, 0, 255) if kind == "values_c_minus_1" else c
    dst = slots[idx]
    ok = np.ones(c.shape, np.uint8) if kind == "valid_ignored" else tab["valid"][idx].astype(np.uint8)
    if mask is not None:
        m = np.asarray(mask) != 0
        if kind != "nodata_not_written":
            dst = np.where(m, dst, WORD[w](int(tab["nodata_bits"]) & ((1 << (8 * w)) - 1)))
        if kind != "input_mask_ignored_in_dst_mask":
            ok = ok & m.astype(np.uint8)
    if kind == "tail_group_as_a_full_one":          # the cells behind the last whole group never stored: left as they were (zero here)
        full = key.size - key.size % cpl(t, dt)
        dst, ok = dst.copy(), ok.copy()
        dst[full:], ok[full:] = 0, 0
    return dst.astype(WORD[w]).view(NP[dt]), ok
