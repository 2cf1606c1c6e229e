"""The inputs of tests/test_gpu_zonal.py can tell a right zonal kernel from a wrong one — checked here without a GPU.

For each mistake a kernel of this family can make, `faulty_members` below is a model of the kernel that makes it: which cells
it folds into which zone's record, given where each cell sits in the launch (`place`: the peeled head, the ragged tail, or tile,
workgroup, wave, lane and slot of the vector kernel — the launch shape restated in tests/zonal_ref.py).  The GPU file's own
inputs (its generators `type_cases`, `pattern_cases`, `poison_inputs`) must contain a launch where the wrong kernel's records
differ from the right ones: count, sum or sum of squares of some zone.  An input set that passed a faulty model would show
nothing on the GPU either."""
import numpy as np
import pytest

import stats_ref as R
import zonal_ref as Z
from test_gpu_stats import NAMES
from test_gpu_zonal import PATTERNS, case_arrays, pattern_cases, poison_inputs, type_cases, zone_ids

CUS, PER_CU = 256, 4   # the grid's cap on an MI355X: a launch of fewer tiles has a workgroup per tile

FAULTS = ["le_at_n_zones", "negative_wraps", "unsigned_read_as_signed", "masked_counted", "first_id_only", "last_id_dropped",
          "last_wave_not_folded", "last_workgroup_skipped", "first_workgroup_twice", "head_to_zone_0", "tail_to_zone_0", "zones_at_value_stride"]


def place(i, n, head, ct):
    """Where cell i of a launch of n cells sits: ("head",), ("tail",) or ("tile", tile, workgroup, load, wave, lane, slot)."""
    cpl = Z.cpl(ct)
    if i < head:
        return ("head",)
    j = i - head
    groups = (n - head) // cpl
    if j >= groups * cpl:
        return ("tail",)
    g, slot = divmod(j, cpl)
    per_tile = Z.BLOCK * Z.U
    tiles = -(-groups // per_tile)
    grid = min(tiles, CUS * PER_CU)
    tile, within = divmod(g, per_tile)
    load, thread = divmod(within, Z.BLOCK)
    return ("tile", tile, tile % grid, load, thread // Z.WAVE, thread % Z.WAVE, slot, grid)


def head_cells(offset_cells, ct, n):
    h = ((16 - offset_cells * Z.SIZE[ct]) % 16) // Z.SIZE[ct]
    return h if h <= n else 0


def faulty_members(kind, ct, zt, zones, nz, mask, head, zone_bytes=None):
    """Per zone, the cells (indices, repeated if folded twice) the faulty kernel folds: Z.members with one mistake."""
    n = len(zones)
    out = [[] for _ in range(nz)]
    bits = 8 * Z.SIZE[zt]
    slots = {}   # (tile, load, wave, slot) -> [(lane, i, z)] of the valid cells, for the mistakes inside one wave slot
    for i in range(n):
        z = zones[i]
        if kind == "zones_at_value_stride":          # the id of cell i read at i * sizeof(T) bytes into the zone raster
            at = i * Z.SIZE[ct]
            raw = zone_bytes[at:at + Z.SIZE[zt]]
            z = int(np.frombuffer(raw, dtype=zones_dtype(zt))[0]) if len(raw) == Z.SIZE[zt] else -1
        if kind == "unsigned_read_as_signed" and zt != R.I32 and z >= 2**(bits - 1):
            z -= 2**bits
        if kind == "negative_wraps" and z < 0:
            z %= nz                                   # an unsigned compare against a table index taken modulo: some zone gets it
        ok = 0 <= z < nz or (kind == "le_at_n_zones" and z == nz)
        if not ok or (mask is not None and mask[i] == 0 and kind != "masked_counted"):
            continue
        z = min(z, nz - 1)                            # le_at_n_zones: the neighbouring entry
        where = place(i, n, head, ct)
        if where[0] == "head":
            out[0 if kind == "head_to_zone_0" else z].append(i)
        elif where[0] == "tail":
            out[0 if kind == "tail_to_zone_0" else z].append(i)
        else:
            _, tile, wg, load, wave, lane, slot, grid = where
            if kind == "last_wave_not_folded" and wave == Z.BLOCK // Z.WAVE - 1:
                continue
            if kind == "last_workgroup_skipped" and grid > 1 and wg == grid - 1:
                continue
            if kind in ("first_id_only", "last_id_dropped"):
                slots.setdefault((tile, load, wave, slot), []).append((lane, i, z))
                continue
            out[z].append(i)
            if kind == "first_workgroup_twice" and grid > 1 and wg == 0:
                out[z].append(i)
    for cells in slots.values():
        cells.sort()
        order = []
        for _, _, z in cells:
            if z not in order:
                order.append(z)
        keep = order[:1] if kind == "first_id_only" else (order[:-1] if len(order) > 1 else order)
        for _, i, z in cells:
            if z in keep:
                out[z].append(i)
    return out


def zones_dtype(zt):
    return {R.U8: np.uint8, R.U16: np.uint16, R.I32: np.int32}[zt]


def figures(cells, members):
    """(count, sum, sum of squares) per zone, exact (the cells here are integers or integer-valued floats)"""
    return [(len(idx), sum(int(cells[i]) for i in idx), sum(int(cells[i]) ** 2 for i in idx)) for idx in members]


def launches():
    """(ct, zt, nz, cells, zones, mask or None, head): the main GPU cases, small ones first"""
    for pattern in PATTERNS:
        for ct, zt, masked, nz, n, seed in pattern_cases(pattern):
            cells, mask = case_arrays(ct, n, seed)
            yield ct, zt, nz, cells, zone_ids(pattern, n, nz, zt), mask if masked else None, 0
    for ct in (R.F64, R.I32, R.U16, R.U8):
        for zt, masked, nz, pattern, pool, off, n, seed in type_cases(ct):
            cells, mask = case_arrays(ct, pool, seed)
            zones = zone_ids(pattern, pool, nz, zt)
            yield ct, zt, nz, cells[off:off + n], zones[off:off + n], mask[off:off + n] if masked else None, head_cells(off, ct, n)


@pytest.mark.parametrize("kind", FAULTS)
def test_every_fault_changes_a_record(kind):
    for ct, zt, nz, cells, zones, mask, head in launches():
        hz, hm = zones.tolist(), None if mask is None else mask.tolist()
        if kind == "zones_at_value_stride" and Z.SIZE[ct] == Z.SIZE[zt]:
            continue
        good = Z.members(hz, nz, hm)
        bad = faulty_members(kind, ct, zt, hz, nz, hm, head, zones.tobytes())
        if figures(cells, good) != figures(cells, bad):
            return
    raise AssertionError(f"no launch of the GPU file tells a kernel with the mistake {kind!r} from a right one")


def test_the_model_without_a_mistake_is_the_reference():
    for k, (ct, zt, nz, cells, zones, mask, head) in enumerate(launches()):
        if k % 9 == 0:
            hz, hm = zones.tolist(), None if mask is None else mask.tolist()
            assert [sorted(m) for m in faulty_members("none", ct, zt, hz, nz, hm, head)] == Z.members(hz, nz, hm)


def test_an_empty_zones_record_left_unwritten_would_show():
    """Some launch has a zone with no cell — and the GPU file fills the records' memory with 0xA5 bytes before every call, which is
    no empty record: count 0xA5A5A5A5A5A5A5A5."""
    empty = 0
    for ct, zt, nz, cells, zones, mask, head in launches():
        empty += any(len(m) == 0 for m in Z.members(zones.tolist(), nz, None if mask is None else mask.tolist()))
    assert empty >= 10
    import inspect

    import test_gpu_zonal
    assert 'b"\\xa5" * (nz * 64)' in inspect.getsource(test_gpu_zonal.device_records)


def test_a_foreign_or_hidden_nan_added_as_nan_times_zero_would_show():
    """The poison launch holds a non-finite cell under a cleared mask byte with an id in range, and one under a foreign id with its
    mask byte set, in the tiles as well as in the ragged tail; every zone has finite cells to poison."""
    for ct in (R.F32, R.F64):
        cells, zones, mask, nz, zt = poison_inputs(ct)
        inr = (zones >= 0) & (zones < nz)
        bad = ~np.isfinite(cells)
        hidden, foreign = bad & inr & (mask == 0), bad & ~inr & (mask == 1)
        assert hidden.sum() > 100 and foreign.sum() > 100 and np.isnan(cells[hidden]).any() and np.isnan(cells[foreign]).any(), NAMES[ct]
        assert not (bad & inr & (mask == 1)).any()
        refs = Z.records(ct, cells.tolist(), zones.tolist(), nz, mask.tolist())
        assert all(r["count"] > 100 and r["s1_exact"] is not None for r in refs)
        # NaN * 0 is NaN: a kernel that multiplies instead of selecting poisons every zone that shares a wave slot with such a cell
        n = cells.size
        for z in range(nz):
            shares = False
            for i in np.flatnonzero(hidden | foreign)[:200]:
                w = place(int(i), n, 0, ct)
                if w[0] == "tile":
                    lo = int(i) - w[5] * Z.cpl(ct)
                    lanes = zones[lo:lo + Z.WAVE * Z.cpl(ct):Z.cpl(ct)]
                    shares = shares or bool((lanes == z).any())
            assert shares, (NAMES[ct], z)
