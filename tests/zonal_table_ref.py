"""The zonal table family restated in plain Python, for the tests of ec_zonal_table_device / ec_zonal_table_compute /
ec_sharded_zonal_table / ec_zonal_lookup (include/erased_cells.h states the rule).  Python integers and `Fraction` throughout;
imports nothing from the library.

Membership is zonal_ref's scalar loop.  Record z: count, min, max, and for the exact integer kind sum and sq, are stats_ref's.
For the pivoted f64 kind, with the zone's deviations d_j = float(x_j) - pivot (one rounded subtraction each):
    d_j = m_j * 2^-1074, m_j an integer;  L = bit length of max |m_j|;  k = max(L - 63, 0)
    t_j = sign(m_j) * (|m_j| >> k);  T = sum t_j;  s1 = T * 2^(k - 1074) rounded to nearest even once
    s2: the same over w_j = d_j * d_j (one rounded multiply); +inf if any w_j is +inf
    a NaN among the d_j: s1 = s2 = NaN;  else infinities: s1 = +inf / -inf for one sign, NaN for both, s2 = +inf
An empty zone has zero sums."""
import math
from fractions import Fraction

import stats_ref as R
import zonal_ref as Z

MAX_ZONES = 1 << 24
ZONE_TYPES, ZONE_RANGE, SIZE = Z.ZONE_TYPES, Z.ZONE_RANGE, Z.SIZE
MAX_CELLS_KIND1 = 2**32

# the kernels' launch shape (tests/test_zonal_table_args.py holds it to the headers): 256 threads x 4 loads of 16 bytes of values
BLOCK, U = 256, 4
WORDS = {0: 6, 1: 10}  # 64-bit words of one zone's entry in the workspace
RECORD_BYTES = 64


def cpl(dtype):
    return 16 // SIZE[dtype]


def tile(dtype):
    return BLOCK * U * cpl(dtype)


def workspace_bytes(dtype, n_zones):
    if dtype not in R.KIND or not 1 <= n_zones <= MAX_ZONES:
        return 0
    return n_zones * WORDS[R.KIND[dtype]] * 8


def units(d):
    """m with d == m * 2^-1074, for a finite float"""
    n, den = d.as_integer_ratio()
    assert (1 << 1074) % den == 0
    return n * ((1 << 1074) // den)


def unit_shift(values):
    """k of a zone with the finite floats `values`"""
    longest = max((abs(units(v)).bit_length() for v in values), default=0)
    return max(longest - 63, 0)


def truncated(v, k):
    m = units(v)
    t = abs(m) >> k
    return -t if m < 0 else t


def round_once(T, k):
    """T * 2^(k - 1074) as the nearest-even float; +0.0 for T == 0, an infinity on overflow"""
    if T == 0:
        return 0.0
    try:
        return float(Fraction(T << k, 1 << 1074))  # int / int: correctly rounded
    except OverflowError:
        return math.inf if T > 0 else -math.inf


def truncated_sum(values, trunc=truncated, shift=None):
    """(s, T, k) of finite floats; `trunc` and `shift` are where tests/test_zonal_table_faults.py plants its mistakes"""
    k = unit_shift(values) if shift is None else shift
    T = sum(trunc(v, k) for v in values)
    return round_once(T, k), T, k


def sums(d):
    """(s1, s2) of one zone's deviations, any floats"""
    if any(math.isnan(x) for x in d):
        return math.nan, math.nan
    pos, neg = any(x == math.inf for x in d), any(x == -math.inf for x in d)
    if pos or neg:
        return (math.nan if pos and neg else math.inf if pos else -math.inf), math.inf
    w = [x * x for x in d]
    s1 = truncated_sum(d)[0]
    s2 = math.inf if any(x == math.inf for x in w) else truncated_sum(w)[0]
    return s1, s2


def record_with_pivot(dtype, cells, pivot):
    """The record of one zone's cells under the call's pivot (a dict as stats_ref.record's; kind 1 also carries `d`, the exact sums
    `s1_exact` / `s2_exact` of d and of the ROUNDED squares w, and the units `k1` / `k2`, or None where a deviation is not finite)."""
    if R.KIND[dtype] == 0:
        return R.record(dtype, cells, None)
    hi, lo = R.sentinels(dtype)
    key = R.total_key if dtype in (R.F32, R.F64) else (lambda x: x)  # the total order; equal keys are equal bits
    vis = [float(x) for x in cells] if dtype in (R.F32, R.F64) else list(cells)
    r = {"count": len(vis), "kind": 1, "dtype": dtype, "min": min(vis, key=key, default=hi), "max": max(vis, key=key, default=lo)}
    d = [float(x) - pivot for x in cells]
    r["pivot"], r["d"] = pivot, d
    r["s1"], r["s2"] = sums(d)
    r["s1_exact"] = r["s2_exact"] = r["k1"] = r["k2"] = None
    if all(math.isfinite(x) for x in d):
        w = [x * x for x in d]
        r["s1_exact"], r["k1"] = R.exact_sum(d), unit_shift(d)
        if all(math.isfinite(x) for x in w):
            r["s2_exact"], r["k2"] = R.exact_sum(w), unit_shift(w)
    return r


def records(dtype, cells, zones, n_zones, mask=None):
    """The n_zones records one call must leave."""
    assert 1 <= n_zones <= MAX_ZONES
    cells = Z._as_list(cells)
    assert len(Z._as_list(zones)) == len(cells)
    pivot = R.pivot_of(dtype, cells)
    return [record_with_pivot(dtype, [cells[i] for i in idx], pivot) for idx in Z.members(zones, n_zones, mask, len(cells))]


def sparse_records(dtype, cells, zones, n_zones, mask=None):
    """{z: record} of the zones that have cells, and the empty record every other zone holds: for n_zones of 2^16 and more"""
    cells, zl = Z._as_list(cells), Z._as_list(zones)
    mk = None if mask is None else Z._as_list(mask)
    pivot = R.pivot_of(dtype, cells)
    of = {}
    for i in range(len(cells)):
        z = Z.zone_of(i, zl, n_zones, mk, len(cells))
        if z is not None:
            of.setdefault(z, []).append(cells[i])
    return {z: record_with_pivot(dtype, xs, pivot) for z, xs in of.items()}, record_with_pivot(dtype, [], pivot)


def stats(dtype, cells, zones, n_zones, mask=None):
    """What ec_zonal_table_compute must return: ec_stats_fold of each record alone."""
    return [R.fold([r]) for r in records(dtype, cells, zones, n_zones, mask)]


def lookup(zones, table, n_zones):
    """(cells, mask bytes) of ec_zonal_lookup: zonal_ref.broadcast's rule, word for word"""
    return Z.broadcast(zones, table, n_zones)


def refusal(n_zones, dtype, zt, p, zones, n, out, workspace, caller_workspace=True, overlaps=None):
    """The text ec_zonal_table_device refuses a call with, or None, in the header's order.  Pointers are integers (0: null)."""
    if not 1 <= n_zones <= MAX_ZONES:
        return "EC_ZONAL_TABLE_MAX_ZONES"
    if dtype not in R.KIND:
        return "bad dtype"
    if zt not in ZONE_TYPES:
        return "zone raster's type"
    if not out or (caller_workspace and not workspace) or (n > 0 and (not p or not zones)):
        return "null pointer"
    if n > (R.MAX_CELLS[dtype] if R.KIND[dtype] == 0 else MAX_CELLS_KIND1):
        return "more cells" if R.KIND[dtype] == 0 else "more than 2^32 cells"
    if caller_workspace:
        if out % 16:
            return "records are not 16-byte aligned"
        if workspace % 16:
            return "workspace is not 16-byte aligned"
    return overlaps
