"""A vectorised numpy restatement of the reference's per-cell order as a predicate — what ec_compare / ec_compare_scalar compute.

impl Ord for CellValue (src/value.rs:248-265, PartialEq :267-271): both cells are converted to CellType::union of their types
(src/value.rs:103-107, the lattice of src/ctype.rs:99-126), integer unions compare naturally, f32 / f64 unions by total_cmp.
tests/test_compare_ref.py holds `cmp3` to the oracle's `eco.value_cmp` cell by cell; the GPU tests and the stand-alone host
program are then held to `relation`.  Also here: the special-values table per type, the inputs the GPU tests use, and numpy
models of the mistakes a compare or select kernel can make (tests/test_compare_faults.py).
"""
import numpy as np

U8, U16, U32, U64, I8, I16, I32, I64, F32, F64 = range(10)
NT = 10
NP = [np.dtype(d) for d in (np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64)]
NAMES = ["UInt8", "UInt16", "UInt32", "UInt64", "Int8", "Int16", "Int32", "Int64", "Float32", "Float64"]
LT, EQ, LE, GT, NE, GE = 1, 2, 3, 4, 5, 6   # ec_cmp: bit 0 Less, bit 1 Equal, bit 2 Greater
RELS = (LT, EQ, LE, GT, NE, GE)


def union(a: int, b: int) -> int:
    """CellType::union (src/ctype.rs:99-126)."""
    sa, sb = NP[a].itemsize, NP[b].itemsize
    ia, ib = NP[a].kind in "ui", NP[b].kind in "ui"
    ga, gb = NP[a].kind != "u", NP[b].kind != "u"
    if ia and not ib:
        mb = max(sb, 2 * sa)
    elif not ia and ib:
        mb = max(sa, 2 * sb)
    elif ga and not gb:
        mb = max(sa, 2 * sb)
    elif not ga and gb:
        mb = max(sb, 2 * sa)
    else:
        mb = max(sa, sb)
    sg, integral = ga or gb, ia and ib
    if integral and mb <= 8:
        return {1: (U8, I8), 2: (U16, I16), 4: (U32, I32), 8: (U64, I64)}[mb][sg]
    return F32 if not integral and mb == 4 else F64


def total_key(a: np.ndarray) -> np.ndarray:
    """f32 / f64::total_cmp as a signed integer key (src/value.rs:260-261): flip the magnitude bits of negatives."""
    it = np.int32 if a.dtype.itemsize == 4 else np.int64
    k = np.ascontiguousarray(a).view(it)
    return k ^ ((k >> (8 * a.dtype.itemsize - 1)) & np.iinfo(it).max)


def cmp3(lt: int, l, rt: int, r) -> np.ndarray:
    """CellValue(l[i]).cmp(CellValue(r[i])) as int8 in {-1, 0, 1}; l, r arrays (or one a scalar) of types lt, rt."""
    u = NP[union(lt, rt)]
    with np.errstate(all="ignore"):
        a, b = np.asarray(l, dtype=NP[lt]).astype(u), np.asarray(r, dtype=NP[rt]).astype(u)   # `as`: every pair is a widening
    if u.kind == "f":
        a, b = total_key(np.atleast_1d(a)), total_key(np.atleast_1d(b))
    return ((a > b).astype(np.int8) - (a < b).astype(np.int8)).reshape(np.broadcast(a, b).shape)


def relation(rel: int, lt: int, l, rt: int, r) -> np.ndarray:
    """out_mask of ec_compare: (rel >> (1 + cmp)) & 1, one byte per cell."""
    return ((rel >> (1 + cmp3(lt, l, rt, r).astype(np.int64))) & 1).astype(np.uint8)


# ---------------------------------------------------------------- the special-values table
_QNAN32 = [0x7FC00000, 0x7FC00001, 0xFFC00000, 0xFFC12345]            # quiet, both signs, two payloads each sign apart
_SNAN32 = [0x7F800001, 0xFFA00000]
_QNAN64 = [0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000000000, 0xFFF8000012345678]
_SNAN64 = [0x7FF0000000000001, 0xFFF4000000000000]


def specials(ct: int, signalling: bool = False) -> np.ndarray:
    """min, max, 0, +-1, 2^24 and 2^24 + 1, 2^53 and 2^53 + 1, 2^63 and 2^64 - 1 where the type holds them; floats also +-0.0,
    +-inf, denormals and quiet NaNs of both signs with two payloads — signalling NaNs only on request (same-type float pairs:
    what a widening conversion does to them is unpinned by the reference)."""
    dt = NP[ct]
    if dt.kind in "ui":
        info = np.iinfo(dt)
        want = [info.min, info.max, 0, 1, -1, 2**24, 2**24 + 1, 2**53, 2**53 + 1, 2**63, 2**64 - 1]
        return np.array(sorted({v for v in want if info.min <= v <= info.max}), dtype=object).astype(dt)
    fi = np.finfo(dt)
    vals = [fi.min, fi.max, 0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, fi.smallest_subnormal, -fi.smallest_subnormal,
            fi.tiny / 2, 2.0**24, 2.0**63]
    vals += [2.0**53] if ct == F32 else [2.0**24 + 1, 2.0**53]          # f32 holds 2^24 but not 2^24 + 1; f64 not 2^53 + 1
    a = np.array(vals, dtype=dt)
    ut = np.uint32 if ct == F32 else np.uint64
    nans = (_QNAN32 if ct == F32 else _QNAN64) + ((_SNAN32 if ct == F32 else _SNAN64) if signalling else [])
    return np.concatenate([a, np.array(nans, dtype=ut).view(dt)])


def cross(lt: int, rt: int):
    """The cross product of the two types' tables as two flat arrays; signalling NaNs in the same-type float pairs only."""
    sig = lt == rt and NP[lt].kind == "f"
    a, b = specials(lt, sig), specials(rt, sig)
    return np.repeat(a, b.size), np.tile(b, a.size)


def gpu_inputs(lt: int, rt: int, n_random: int = 4099, seed: int = 0):
    """What tests/test_gpu_compare.py compares: the special-values cross product, then n_random random cells with ties planted
    (every third random cell of r is l's cell as r's type where that compares Equal, and every third of l is r's cell likewise)."""
    from vectors import rand_cells
    a, b = cross(lt, rt)
    sig = lt == rt and NP[lt].kind == "f"
    ra, rb = rand_cells(lt, n_random, 9100 + seed, specials=sig), rand_cells(rt, n_random, 9200 + seed, specials=sig)
    if not sig:   # rand_cells' specials hold signalling NaNs: mixed pairs take the quiet table instead
        sa, sb = specials(lt), specials(rt)
        ra[::7], rb[3::11] = sa[np.arange(ra[::7].size) % sa.size], sb[np.arange(rb[3::11].size) % sb.size]
    with np.errstate(all="ignore"):
        back = ra.astype(NP[rt])              # a candidate tie: l's cell as r's type; kept only where it really is Equal
    tie = np.zeros(n_random, bool)
    tie[::3] = True
    tie &= cmp3(lt, ra, rt, back) == 0
    rb[tie] = back[tie]
    with np.errstate(all="ignore"):
        forth = rb.astype(NP[lt])             # and the other way round, for the pairs where l's type is the wider one
    tie = np.zeros(n_random, bool)
    tie[1::3] = True
    tie &= cmp3(lt, forth, rt, rb) == 0
    ra[tie] = forth[tie]
    return np.concatenate([a, ra]), np.concatenate([b, rb])


def tail_len(n: int) -> int:
    """The largest length <= n that leaves a ragged tail of 15 cells behind the last 16-cell group (n >= 15): at every CPL of
    the kernels (2, 4, 8, 16) the last group is then partial."""
    return n - (n - 15) % 16


def gpu_masks(n: int):
    """The two masks of the masked forms: random, different, and both valid over the last 15 cells, so that a kernel that ANDs the
    masks but forgets the predicate in the ragged tail is seen there."""
    from vectors import rand_mask
    lm, rm = rand_mask(n, 9300), rand_mask(n, 9301, p_valid=0.6)
    lm[-15:], rm[-15:] = 1, 1
    return lm, rm


def select_inputs(ct: int, n: int = 4099 + 15):
    """(sel, a, amask, b, bmask) of the select tests: two random buffers of one type and three different masks."""
    from vectors import rand_cells, rand_mask
    return (rand_mask(n, 9400, p_valid=0.5), rand_cells(ct, n, 9401), rand_mask(n, 9402), rand_cells(ct, n, 9403), rand_mask(n, 9404, p_valid=0.4))


# ---------------------------------------------------------------- fault models: the mistakes a kernel can make
def _cmp3_faulty(kind: str, lt, l, rt, r):
    u = NP[union(lt, rt)]
    with np.errstate(all="ignore"):
        if kind == "f64_whatever_the_union":
            a, b = total_key(np.asarray(l).astype(np.float64)), total_key(np.asarray(r).astype(np.float64))
        elif kind == "ieee_instead_of_total_order":
            a, b = np.asarray(l).astype(u), np.asarray(r).astype(u)   # NaN: neither <, > nor == -> reads as Equal here
        elif kind == "raw_bits_of_floats":
            a, b = np.asarray(l).astype(u), np.asarray(r).astype(u)
            if u.kind == "f":
                it = np.int32 if u.itemsize == 4 else np.int64
                a, b = a.view(it), b.view(it)
        elif kind == "signed_compare_of_u64":
            a, b = np.asarray(l).astype(u), np.asarray(r).astype(u)
            if u == NP[U64]:
                a, b = a.view(np.int64), b.view(np.int64)
            elif u.kind == "f":
                a, b = total_key(a), total_key(b)
        else:
            raise KeyError(kind)
        return (a > b).astype(np.int8) - (a < b).astype(np.int8)


VALUE_FAULTS = ("f64_whatever_the_union", "ieee_instead_of_total_order", "raw_bits_of_floats", "signed_compare_of_u64")
MASK_FAULTS = ("forgot_lmask", "forgot_rmask", "tail_masks_without_predicate")
SELECT_FAULTS = ("sel_inverted", "out_mask_from_the_wrong_side")


def relation_faulty(kind: str, rel, lt, l, rt, r):
    """`relation` as a kernel with the value fault `kind` would compute it."""
    return ((rel >> (1 + _cmp3_faulty(kind, lt, l, rt, r).astype(np.int64))) & 1).astype(np.uint8)


def masked_relation(rel, lt, l, lm, rt, r, rm):
    """ec_compare with masks: the predicate ANDed with every mask given (None: not given)."""
    out = relation(rel, lt, l, rt, r)
    for m in (lm, rm):
        if m is not None:
            out = out & m[:out.size]
    return out


def masked_relation_faulty(kind: str, rel, lt, l, lm, rt, r, rm, cpl: int):
    """The mask faults: one mask forgotten, or — in the ragged tail behind the last whole group of `cpl` cells — the masks ANDed
    but not the predicate."""
    if kind == "forgot_lmask":
        return masked_relation(rel, lt, l, None, rt, r, rm)
    if kind == "forgot_rmask":
        return masked_relation(rel, lt, l, lm, rt, r, None)
    out = masked_relation(rel, lt, l, lm, rt, r, rm)
    tail = out.size - out.size % cpl
    out[tail:] = (lm[tail:out.size] & rm[tail:out.size])
    return out


def select(sel, a, b):
    return np.where(sel.astype(bool), a, b)


def masked_select(sel, a, am, b, bm):
    return select(sel, a, b), select(sel, am, bm).astype(np.uint8)


def masked_select_faulty(kind: str, sel, a, am, b, bm):
    if kind == "sel_inverted":
        return masked_select(1 - sel, a, am, b, bm)
    return select(sel, a, b), select(sel, bm, am).astype(np.uint8)
