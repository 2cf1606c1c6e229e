"""Zonal statistics restated in plain Python, for the tests of ec_zonal_stats_device / ec_zonal_stats_compute /
ec_sharded_zonal_stats / ec_zonal_broadcast (include/erased_cells.h states the rule).  Membership is a scalar loop over that
rule; record z is stats_ref.record of the cells of zone z with the pivot overridden by the CALL's pivot (the first cell of the
whole raster, whatever its mask byte or zone).  Imports nothing from the library.

Also the launch constants of the kernels, restated (tests/test_zonal_args.py holds them to the kernel headers)."""
import math

import stats_ref as R

ZONE_TYPES = (R.U8, R.U16, R.I32)
ZONE_RANGE = {R.U8: (0, 2**8 - 1), R.U16: (0, 2**16 - 1), R.I32: (-2**31, 2**31 - 1)}
MAX_ZONES = 256

# the zonal kernels' launch shape: 256 threads (4 waves of 64) x 4 loads of 16 bytes of values per lane
BLOCK, WAVE, U = 256, 64, 4
PARTIAL_BYTES, RECORD_BYTES, MAX_BLOCKS = 48, 64, 4096
BROADCAST_U = 2
SIZE = {R.U8: 1, R.U16: 2, R.U32: 4, R.U64: 8, R.I8: 1, R.I16: 2, R.I32: 4, R.I64: 8, R.F32: 4, R.F64: 8}


def cpl(dtype):
    """cells of one 16-byte group of values"""
    return 16 // SIZE[dtype]


def tile(dtype):
    """cells one workgroup takes per round"""
    return BLOCK * U * cpl(dtype)


def broadcast_cpl(dtype, zt):
    return 16 // max(SIZE[dtype], SIZE[zt])


def broadcast_tile(dtype, zt):
    return BLOCK * BROADCAST_U * broadcast_cpl(dtype, zt)


def workspace_bytes(n_zones):
    return n_zones * MAX_BLOCKS * PARTIAL_BYTES if 1 <= n_zones <= MAX_ZONES else 0


def _as_list(a):
    return a.tolist() if hasattr(a, "tolist") else list(a)


def zone_of(i, zones, n_zones, mask, n):
    """The zone cell i belongs to, or None: the header's rule, one cell."""
    if not i < n:
        return None
    z = zones[i]
    if not 0 <= z < n_zones:
        return None
    if mask is not None and mask[i] == 0:
        return None
    return z


def members(zones, n_zones, mask=None, n=None):
    """Per zone, the indices of its cells, in raster order."""
    zones = _as_list(zones)
    mask = None if mask is None else _as_list(mask)
    n = len(zones) if n is None else n
    out = [[] for _ in range(n_zones)]
    for i in range(n):
        z = zone_of(i, zones, n_zones, mask, n)
        if z is not None:
            out[z].append(i)
    return out


def record_with_pivot(dtype, cells, pivot):
    """stats_ref.record(dtype, cells, None) with the deviations taken against `pivot` instead of the cells' own first cell."""
    r = R.record(dtype, cells, None)
    if r["kind"] == 0:
        return r
    d = [float(x) - pivot for x in cells]
    r["pivot"] = pivot
    for k in ("s1_exact", "s2_exact", "s1", "s2", "abs_d", "sq_d"):
        r.pop(k, None)
    if all(math.isfinite(x) for x in d):
        r["s1_exact"], r["s2_exact"] = R.exact_sum(d), R.exact_sum(d, 2)
        r["s1"], r["s2"] = float(r["s1_exact"]), float(r["s2_exact"])
        r["abs_d"], r["sq_d"] = R.exact_sum([abs(x) for x in d]), r["s2_exact"]
    else:
        r["s1_exact"] = r["s2_exact"] = None
        nan = any(math.isnan(x) for x in d)
        pos, neg = any(x == math.inf for x in d), any(x == -math.inf for x in d)
        r["s1"] = math.nan if nan or (pos and neg) else (math.inf if pos else -math.inf)
        r["s2"] = math.nan if nan else math.inf
    return r


def records(dtype, cells, zones, n_zones, mask=None):
    """The n_zones records one call must leave (dicts as stats_ref.record's)."""
    assert 1 <= n_zones <= MAX_ZONES
    cells = _as_list(cells)
    assert len(_as_list(zones)) == len(cells)
    pivot = R.pivot_of(dtype, cells)
    return [record_with_pivot(dtype, [cells[i] for i in idx], pivot) for idx in members(zones, n_zones, mask, len(cells))]


def stats(dtype, cells, zones, n_zones, mask=None):
    """What ec_zonal_stats_compute must return for exactly summable cells: ec_stats_fold of each record alone."""
    return [R.fold([r]) for r in records(dtype, cells, zones, n_zones, mask)]


def broadcast(zones, table, n_zones):
    """(cells, mask bytes) of ec_zonal_broadcast: table[zones[i]] and 1, or 0 and 0 for an id that belongs to no zone."""
    table = _as_list(table)
    assert len(table) >= n_zones
    out, mask = [], []
    for z in _as_list(zones):
        ok = 0 <= z < n_zones
        out.append(table[z] if ok else 0)
        mask.append(1 if ok else 0)
    return out, mask
