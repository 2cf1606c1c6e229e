"""The inputs of tests/test_gpu_zonal_table.py expose the mistakes a kernel of this family can make: for each modelled mistake, the
reference with that mistake built in gives other bytes than the reference itself for at least one of the GPU file's cases
(tests/zonal_table_cases.py builds them without a device).  The model without a mistake IS the reference."""
import math

import numpy as np
import pytest

import stats_ref as R
import zonal_ref as Z
import zonal_table_cases as K
import zonal_table_ref as ZT

RECORD_FAULTS = [
    "rounding where the rule truncates",
    "the unit from the launch-wide maximum",
    "the unit from another zone",
    "s2's unit taken from s1's",
    "a hidden cell's |d| reaches the maximum",
    "a NaN under a cleared byte reaches the flags",
    "a foreign cell's |d| and flag reach the lane's running entry",
    "a lost carry",
    "a lane's run flushed to the previous id",
    "a lane's run dropped at the tail",
    "an id compared as unsigned",
    "an id truncated to 16 bits",
    "record K - 1 unwritten",
]


def rounded(v, k):
    """m / 2^k to the nearest integer, ties to even: what the rule does NOT do"""
    m = ZT.units(v)
    q, rest = abs(m) >> k, abs(m) & ((1 << k) - 1)
    half = (1 << k) >> 1
    if k and (rest > half or (rest == half and q & 1)):
        q += 1
    return -q if m < 0 else q


def wrap64(T):
    return (T + 2**63) % 2**64 - 2**63


def model_sums(d, hidden, fault, k_launch, k_other):
    """(s1, s2) of a zone with the shown deviations d and the hidden ones of its id, with `fault` built in"""
    foreign = fault == "a foreign cell's |d| and flag reach the lane's running entry"   # then `hidden` holds those cells' deviations
    cls = d + (hidden if foreign or fault == "a NaN under a cleared byte reaches the flags" else [])
    if any(math.isnan(x) for x in cls):
        return math.nan, math.nan
    pos, neg = math.inf in cls, -math.inf in cls
    if pos or neg:
        return (math.nan if pos and neg else math.inf if pos else -math.inf), math.inf
    mx = d + ([x for x in hidden if math.isfinite(x)] if foreign or fault == "a hidden cell's |d| reaches the maximum" else [])
    wmx = [x * x for x in mx]
    k1, k2 = ZT.unit_shift(mx), (ZT.unit_shift(wmx) if all(math.isfinite(x) for x in wmx) else None)
    if fault == "the unit from the launch-wide maximum":
        k1, k2 = k_launch
    if fault == "the unit from another zone":
        k1, k2 = k_other
    if fault == "s2's unit taken from s1's" and k2 is not None:
        k2 = k1
    trunc = rounded if fault == "rounding where the rule truncates" else ZT.truncated
    fix = wrap64 if fault == "a lost carry" else (lambda T: T)
    s1 = ZT.round_once(fix(sum(trunc(x, k1) for x in d)), k1)
    s2 = math.inf if k2 is None or any(math.isinf(x * x) for x in d) else ZT.round_once(fix(sum(trunc(x * x, k2) for x in d)), k2)
    return s1, s2


def units_of(values):
    fin = [x for x in values if math.isfinite(x)]
    w = [x * x for x in fin]
    return ZT.unit_shift(fin), (ZT.unit_shift(w) if all(math.isfinite(x) for x in w) else None)


def model(ct, cells, zones, nz, mask, fault=None):
    """the n_zones records as {z: 64 bytes} of the zones that differ from the empty record, and the empty record's bytes"""
    cells, zid = Z._as_list(cells), Z._as_list(zones)
    n = len(cells)
    shown = [mask is None or mask[i] != 0 for i in range(n)]
    if fault == "an id truncated to 16 bits":
        zid = [z & 0xFFFF for z in zid]
    if fault == "an id compared as unsigned":   # only `id < n_zones` is asked, and -1 indexes the word before the next zone's
        zid = [z + nz if -nz <= z < 0 else z for z in zid]
    member = [zid[i] if 0 <= zid[i] < nz and shown[i] else None for i in range(n)]
    if fault in ("a lane's run flushed to the previous id", "a lane's run dropped at the tail"):   # one lane over the raster
        runs = []
        for i, z in enumerate(member):
            if z is None:
                continue
            if runs and runs[-1][0] == z:
                runs[-1][1].append(i)
            else:
                runs.append((z, [i]))
        if fault == "a lane's run dropped at the tail":
            runs = runs[:-1]
        else:
            runs = [(runs[j - 1][0] if j else z, idx) for j, (z, idx) in enumerate(runs)]
        member = [None] * n
        for z, idx in runs:
            for i in idx:
                member[i] = z
    pivot = R.pivot_of(ct, cells)
    of, hidden = {}, {}
    stray = fault == "a foreign cell's |d| and flag reach the lane's running entry"   # abs_bits(d) and the flag taken before the validity select
    held = None                                                                       # the zone the lane holds: the previous member in raster order
    for i in range(n):
        if member[i] is not None:
            of.setdefault(member[i], []).append(cells[i])
            held = member[i]
        elif stray:
            if shown[i] and held is not None:   # a shown cell of no zone
                hidden.setdefault(held, []).append(float(cells[i]) - pivot)
        elif 0 <= zid[i] < nz and not shown[i]:
            hidden.setdefault(zid[i], []).append(float(cells[i]) - pivot)
    out = {}
    kind1 = R.KIND[ct] == 1
    if kind1:
        dev = {z: [float(x) - pivot for x in xs] for z, xs in of.items()}
        k_launch = units_of([x for d in dev.values() for x in d])
    for z, xs in of.items():
        r = ZT.record_with_pivot(ct, xs, pivot)
        if kind1:
            k_other = units_of(dev.get((z + 1) % nz, []))
            r["s1"], r["s2"] = model_sums(dev[z], hidden.get(z, []), fault, k_launch, k_other)
        elif fault == "a lost carry":
            r["sq"] &= 2**64 - 1
        out[z] = K.record_bytes(r)
    empty = K.record_bytes(ZT.record_with_pivot(ct, [], pivot))
    if kind1 and fault == "a NaN under a cleared byte reaches the flags":   # a zone of hidden cells only
        for z, h in hidden.items():
            if z not in of and any(not math.isfinite(x) for x in h):
                r = ZT.record_with_pivot(ct, [], pivot)
                r["s1"], r["s2"] = model_sums([], h, fault, None, None)
                out[z] = K.record_bytes(r)
    if fault == "record K - 1 unwritten":
        out[nz - 1] = b"\xa5" * 64   # what tests/test_gpu_zonal_table.py fills the block with
    return {z: b for z, b in out.items() if b != empty}, empty


def cases():
    """(what, ct, cells, zones, nz, mask or None) of the GPU file's record tests (one zone type of the planted raster; the sizes,
    patterns and the second-round case repeat these arrays' kinds at other lengths)"""
    for zt in (R.I32, R.U16):
        cells, zones, mask, nz = K.planted_raster(zt)
        yield ("planted", zt), R.F64, cells.tolist(), zones.tolist(), nz, mask.tolist()
    for case in list(K.kind0_cases()) + list(K.kind1_exact_cases()):
        ct, zt, masked, nz, pattern, n, off, seed = case
        cells, mask, zones = K.arrays(ct, zt, nz, pattern, n, off, seed)
        yield case, ct, cells[off:].tolist(), zones[off:].tolist(), nz, mask[off:].tolist() if masked else None
    for nz in K.BIG_K:
        for ct, zt, masked in ((R.F64, R.I32, True), (R.U32, R.U16, False), (R.I16, R.I32, True)):
            cells, mask, zones = K.big_k_case(nz, zt, ct, 0xB16 + nz % 97)
            yield ("many zones", nz, ct), ct, cells.tolist(), zones.tolist(), nz, mask.tolist() if masked else None
    n = 2 * ZT.tile(R.F64) + 5
    cells, zones, mask = K.general_raster(n, 300, R.U16, seed=0x0DE4)
    cells[5] = 2.0**90
    yield "general", R.F64, cells.tolist(), zones.tolist(), 300, mask.tolist()


@pytest.fixture(scope="module")
def right():
    """the model without a mistake, per case — computed once"""
    return [(c, model(*c[1:])) for c in cases()]


def test_the_model_without_a_mistake_is_the_reference(right):
    for (what, ct, cells, zones, nz, mask), (found, empty) in right:
        want, want_empty = ZT.sparse_records(ct, cells, zones, nz, mask)
        assert empty == K.record_bytes(want_empty), what
        assert found == {z: K.record_bytes(r) for z, r in want.items() if K.record_bytes(r) != empty}, what


@pytest.mark.parametrize("fault", RECORD_FAULTS)
def test_every_fault_changes_a_record(right, fault):
    shows = [c[0] for c, good in right if model(*c[1:], fault=fault) != good]
    print(fault, "shows in", len(shows), "of", len(right), "cases")
    assert shows, fault


def test_the_lookup_indexing_with_a_foreign_id_would_show():
    shows = 0
    for nz in K.LOOKUP_ZONES:
        for ct, zt in K.LOOKUP_PAIRS:
            zones, table = K.lookup_arrays(ct, zt, nz, 200)
            right_cells, right_mask = ZT.lookup(zones.tolist(), table.tolist(), nz)
            wrong = [table[z % nz] for z in zones.tolist()]   # the id used as it comes
            if nz > Z.ZONE_RANGE[zt][1]:   # every id the type holds is a zone: nothing is foreign
                continue
            assert any(m == 0 for m in right_mask), (nz, ct, zt, "no foreign id in the case")
            assert np.array(wrong, dtype=K.NP[ct]).tobytes() != np.array(right_cells, dtype=K.NP[ct]).tobytes(), (nz, ct, zt)
            shows += 1
    assert shows == sum(nz <= Z.ZONE_RANGE[zt][1] for nz in K.LOOKUP_ZONES for _, zt in K.LOOKUP_PAIRS) == 19


def test_a_foreign_cells_maximum_or_flag_would_show_on_the_planted_raster():
    """the planted raster's shown decoys of no zone (NaN, -inf, 1e300, 2^1000 under the ids n_zones and -1 or the type's maximum):
    merged into the entry of the zone the lane holds, the non-finite ones turn that zone's sums into NaN or infinities and the
    finite ones move its unit"""
    fault = "a foreign cell's |d| and flag reach the lane's running entry"
    for zt in (R.I32, R.U16, R.U8):
        cells, zones, mask, nz = K.planted_raster(zt)
        good, _ = model(R.F64, cells, zones, nz, mask.tolist())
        bad, _ = model(R.F64, cells, zones, nz, mask.tolist(), fault=fault)
        changed = {z for z in range(nz) if good.get(z) != bad.get(z)}
        assert len(changed) >= 2 and nz - 1 in changed, (zt, changed)   # the general zone holds most lanes' entries


def test_the_planted_zones_are_where_each_unit_mistake_shows():
    """the hand zones single the unit mistakes out: with the launch-wide unit (the hidden 1e300 apart, 2^900 of the +inf zone's is
    not a sum) the zone of 2^70 and 1.5s keeps its big cell but every small zone loses its sum"""
    cells, zones, mask, nz = K.planted_raster()
    good, _ = model(R.F64, cells, zones, nz, mask.tolist())
    bad, _ = model(R.F64, cells, zones, nz, mask.tolist(), fault="the unit from the launch-wide maximum")
    changed = {z for z in range(nz) if good.get(z) != bad.get(z)}
    assert 3 in changed and nz - 1 in changed   # the subnormal zone and the general zone
    bad, _ = model(R.F64, cells, zones, nz, mask.tolist(), fault="rounding where the rule truncates")
    assert {z for z in range(nz) if good.get(z) != bad.get(z)} >= {1, 12}   # 384 = 1.5 units: a tie, to 2; -384.5 to -2
