"""Band statistics restated in plain Python, for the tests of ec_stats_device / ec_stats_fold / ec_stats_compute: what one
launch's record must hold and what the host fold must make of one or several records (include/erased_cells.h states both).
Python ints for the exact integer kind, exact rationals (`fractions`, built from `float.as_integer_ratio`) for the pivoted f64
kind, and the fold's formulas step by step in Python floats — each `+ - * /` of two floats is one correctly rounded IEEE
binary64 operation, `float(int)` rounds to nearest even, `math.sqrt` is correctly rounded.
Imports nothing from the library.

dtype codes are the ABI's: U8 0, U16 1, U32 2, U64 3, I8 4, I16 5, I32 6, I64 7, F32 8, F64 9.  Cells come as any sequence of
Python numbers (or something with `.tolist()`); f32 cells as the Python floats that equal them.
"""
import math
import struct
from fractions import Fraction
from operator import mul

U8, U16, U32, U64, I8, I16, I32, I64, F32, F64 = range(10)
KIND = {U8: 0, I8: 0, U16: 0, I16: 0, U32: 0, I32: 0, U64: 1, I64: 1, F32: 1, F64: 1}
_INT_RANGE = {U8: (0, 2**8 - 1), U16: (0, 2**16 - 1), U32: (0, 2**32 - 1), U64: (0, 2**64 - 1),
              I8: (-2**7, 2**7 - 1), I16: (-2**15, 2**15 - 1), I32: (-2**31, 2**31 - 1), I64: (-2**63, 2**63 - 1)}
_F32_MAX = float.fromhex("0x1.fffffep+127")
_F64_MAX = float.fromhex("0x1.fffffffffffffp+1023")


def sentinels(dtype):
    """(T::MAX, T::MIN): what min / max hold when nothing counted (src/buffer.rs:170; finite for floats)."""
    if dtype == F32:
        return _F32_MAX, -_F32_MAX
    if dtype == F64:
        return _F64_MAX, -_F64_MAX
    lo, hi = _INT_RANGE[dtype]
    return hi, lo


def total_key(x):
    """f64::total_cmp as an integer key (src/value.rs:248-265 orders floats by it); widening an f32 to f64 keeps the order."""
    b = struct.unpack("<q", struct.pack("<d", x))[0]
    return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFF)


def _as_list(cells):
    return cells.tolist() if hasattr(cells, "tolist") else list(cells)


def visible(cells, mask=None):
    cells = _as_list(cells)
    if mask is None:
        return cells
    return [x for x, m in zip(cells, _as_list(mask)) if m]


def pivot_of(dtype, cells):
    """to_f64 of the FIRST cell — masked or not — if there is one and it is finite, else 0.0."""
    cells = _as_list(cells)
    if KIND[dtype] == 0 or not cells:
        return 0.0
    c = float(cells[0])
    return c if math.isfinite(c) else 0.0


def exact_sum(floats, power=1):
    """The exact sum of x ** power over finite floats, as a Fraction."""
    pairs = [x.as_integer_ratio() for x in floats]
    if not pairs:
        return Fraction(0)
    den = max(d for _, d in pairs) ** power  # denominators are powers of two: the largest is a common one
    return Fraction(sum(n ** power * (den // d ** power) for n, d in pairs), den)


def deviations(dtype, cells, mask=None):
    """d = to_f64(x) - pivot of every visible cell, each one rounded subtraction, as the kernel forms them."""
    c = pivot_of(dtype, cells)
    return [float(x) - c for x in visible(cells, mask)]


def record(dtype, cells, mask=None):
    """The ec_moments one launch over `cells` must leave, as a dict: count, min, max (cells; the sentinels when empty), kind,
    dtype and `sum`, `sq` (kind 0: exact ints) or `pivot`, `s1`, `s2` (kind 1: the EXACT sums of d and d * d rounded once — what
    any summation order gives when every partial sum is representable; `s1_exact` / `s2_exact` hold the rationals, or None when
    a visible cell is not finite)."""
    vis = visible(cells, mask)
    hi, lo = sentinels(dtype)
    r = {"count": len(vis), "kind": KIND[dtype], "dtype": dtype}
    if KIND[dtype] == 0:
        r["min"] = min(vis, default=hi)
        r["max"] = max(vis, default=lo)
        r["sum"] = sum(vis)
        r["sq"] = sum(map(mul, vis, vis))
        return r
    fl = [float(x) for x in vis] if dtype in (F32, F64) else None
    if fl is not None:  # total order; equal keys are equal bits
        r["min"] = min(fl, key=total_key, default=hi)
        r["max"] = max(fl, key=total_key, default=lo)
    else:
        r["min"] = min(vis, default=hi)
        r["max"] = max(vis, default=lo)
    d = deviations(dtype, cells, mask)
    r["pivot"] = pivot_of(dtype, cells)
    if all(math.isfinite(x) for x in d):
        r["s1_exact"], r["s2_exact"] = exact_sum(d), exact_sum(d, 2)
        r["s1"], r["s2"] = float(r["s1_exact"]), float(r["s2_exact"])
        r["abs_d"], r["sq_d"] = exact_sum([abs(x) for x in d]), r["s2_exact"]
    else:  # IEEE propagation, the same in any order: a NaN, or infinities of both signs, make NaN
        r["s1_exact"] = r["s2_exact"] = None
        nan = any(math.isnan(x) for x in d)
        pos, neg = any(x == math.inf for x in d), any(x == -math.inf for x in d)
        r["s1"] = math.nan if nan or (pos and neg) else (math.inf if pos else -math.inf)
        r["s2"] = math.nan if nan else math.inf
    return r


def _moments_of(r):
    """(n, mean, M2, sum) of one record with count > 0."""
    cnt = float(r["count"])
    if r["kind"] == 0:
        s1, s2 = r["sum"], r["sq"]
        num = r["count"] * s2 - s1 * s1
        assert 0 <= num < 2**128 and -2**63 <= s1 < 2**63 and 0 <= s2 < 2**128
        return r["count"], float(s1) / cnt, float(num) / cnt, float(s1)
    q = r["s1"] / cnt
    mean = r["pivot"] + q
    m2 = r["s2"] - r["s1"] * q
    if m2 < 0.0:
        m2 = 0.0
    return r["count"], mean, m2, r["pivot"] * cnt + r["s1"]


MAX_CELLS = {U8: 2**32, I8: 2**32, U16: 2**32, I16: 2**32, U32: 2**31, I32: 2**31}  # what one exact record may cover


def _runs(records):
    """The non-empty records as they enter the merge: integer records added up exactly, left to right, while the cells they
    cover stay within MAX_CELLS (a run that would pass it is closed and the next begins); f64 records one by one."""
    out, run = [], None
    for r in records:
        if r["count"] == 0:
            continue
        if r["kind"] != 0:
            out.append(r)
        elif run is not None and run["count"] + r["count"] <= MAX_CELLS[r["dtype"]]:
            run = dict(run, count=run["count"] + r["count"], sum=run["sum"] + r["sum"], sq=run["sq"] + r["sq"])
        else:
            if run is not None:
                out.append(run)
            run = r
    return out + ([run] if run is not None else [])


def fold(records):
    """ec_stats_fold: records left to right into count, min, max, sum, mean, stddev."""
    assert len(records) >= 1 and len({r["dtype"] for r in records}) == 1
    dtype = records[0]["dtype"]
    fp = dtype in (F32, F64)
    key = total_key if fp else (lambda x: x)
    mn = min((r["min"] for r in records), key=key)  # empty records hold the sentinels: the identity
    mx = max((r["max"] for r in records), key=key)
    n, mean, m2, total = 0, 0.0, 0.0, 0.0
    for r in _runs(records):
        nb, mean_b, m2_b, sum_b = _moments_of(r)
        if n == 0:
            n, mean, m2, total = nb, mean_b, m2_b, sum_b
            continue
        nn = n + nb
        delta = mean_b - mean
        mean = mean + delta * (float(nb) / float(nn))
        m2 = (m2 + m2_b) + (delta * delta) * (float(n) * float(nb) / float(nn))
        total = total + sum_b
        n = nn
    if n == 0:
        return {"count": 0, "min": mn, "max": mx, "sum": 0.0, "mean": math.nan, "stddev": math.nan}
    var = m2 / float(n)
    return {"count": n, "min": mn, "max": mx, "sum": total, "mean": mean, "stddev": math.sqrt(var)}


def stats(dtype, cells, mask=None):
    """What ec_stats_compute must return for exactly summable cells."""
    return fold([record(dtype, cells, mask)])


def order_key(dtype, x):
    """The int64 order key of a cell, as ec_min_max_keys encodes min / max: the value for integers (u64 biased by 2^63), the
    total_cmp key of the cell's own width for floats."""
    if dtype == U64:
        return x - 2**63
    if dtype == F64:
        return total_key(x)
    if dtype == F32:
        b = struct.unpack("<i", struct.pack("<f", x))[0]
        return b ^ ((b >> 31) & 0x7FFFFFFF)
    return x


def key_value(dtype, k):
    """The cell an order key stands for: the inverse of order_key."""
    if dtype == U64:
        return k + 2**63
    if dtype == F64:
        b = k ^ ((k >> 63) & 0x7FFFFFFFFFFFFFFF)
        return struct.unpack("<d", struct.pack("<q", b))[0]
    if dtype == F32:
        b = k ^ ((k >> 31) & 0x7FFFFFFF)
        return struct.unpack("<f", struct.pack("<i", b))[0]
    return k
