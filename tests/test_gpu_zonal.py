"""Zonal statistics on the device (ec_zonal_stats_device / ec_zonal_stats_compute / ec_zonal_broadcast and the Python
mirror's `zonal_stats()` / `broadcast()`) against tests/zonal_ref.py — never against the library itself.  Records are compared
field by field (assert_record of tests/test_gpu_stats.py); for the exact integer kind that is the whole answer, for the
pivoted f64 kind the cells are BASE + r with 0 < |r| <= 512 as there, so every partial sum of d and d * d is representable
and the record must equal the exact sums in whatever order the launch adds them.

Sizes come from the kernels' tile, restated in zonal_ref (256 threads x 4 loads of 16 bytes of values): T = 1024 * (16 / size)
cells; test_zonal_args.py holds those constants to the kernel headers."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import stats_ref as R
import zonal_ref as Z
from test_gpu_stats import BASE, NAMES, NP, assert_record, assert_stats, bits, random_cells, random_mask, size_of

pytestmark = pytest.mark.gpu

ZNP = {R.U8: np.uint8, R.U16: np.uint16, R.I32: np.int32}
N_ZONES = [1, 2, 63, 64, 65, 255, 256]
PATTERNS = ["constant", "modulo", "runs37", "alternating", "edges"]


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


@pytest.fixture(scope="module")
def space(ec):
    """workspace and record memory per n_zones, allocated once"""
    made = {}

    def get(nz):
        if nz not in made:
            made[nz] = (ec.DeviceMem(ec.lib().ec_zonal_workspace_bytes(nz)), ec.DeviceMem(nz * 64))
        return made[nz]
    return get


def zone_ids(pattern, n, nz, zt, seed=0):
    """n zone ids of type zt"""
    lo, hi = Z.ZONE_RANGE[zt]
    i = np.arange(n, dtype=np.int64)
    if pattern == "constant":
        z = np.full(n, nz // 2, dtype=np.int64)
    elif pattern == "modulo":          # every lane of a slot has a different id
        z = i % nz
    elif pattern == "runs37":          # runs of prime length that straddle slots, waves and tiles
        z = (i // 37) % nz
    elif pattern == "alternating":
        z = np.where(i % 2 == 0, 0, nz - 1)
    elif pattern == "edges":           # the last zone, the first foreign id, the type's extremes
        vals = [nz - 1, nz, hi, 0] + ([-1, lo] if zt == R.I32 else [])
        vals = [v for v in vals if lo <= v <= hi]
        z = np.array(vals, dtype=np.int64)[(i // 3) % len(vals)]
    elif pattern == "random":
        z = np.random.default_rng(seed).integers(-1 if zt == R.I32 else 0, nz, size=n, endpoint=True)  # nz itself: foreign
        z = np.clip(z, lo, hi)
    else:
        raise AssertionError(pattern)
    return z.astype(ZNP[zt])


def device_records(ec, space, ct, p, pm, zt, zp, n, nz, stream=None):
    L, E = ec.lib(), ec._ffi
    ws, out = space(nz)
    E.check(L.ec_upload(out.ptr, b"\xa5" * (nz * 64), nz * 64, stream))  # a record left unwritten would show
    E.check(L.ec_zonal_stats_device(ct, p, pm, zt, zp, n, nz, out.ptr, ws.ptr, stream))
    recs = (E.EcMoments * nz)()
    E.check(L.ec_download(recs, out.ptr, nz * 64, stream))
    return recs


def compute(ec, ct, p, pm, zt, zp, n, nz):
    out = (ec._ffi.EcStats * nz)()
    ec._ffi.check(ec.lib().ec_zonal_stats_compute(ct, p, pm, zt, zp, n, nz, out, None))
    return out


def case_arrays(ct, n, seed):
    """the cells and the mask bytes of a Case (tests/test_zonal_faults.py rebuilds them without a GPU)"""
    return random_cells(ct, n, seed), random_mask(n, seed + 1)


class Case:
    """A value raster, a mask and a zone raster on the device, with windows into them at cell offsets."""

    def __init__(self, ec, ct, zt, zones, seed):
        self.ct, self.zt, self.n = ct, zt, zones.size
        self.cells, self.mask = case_arrays(ct, self.n, seed)
        self.zones = zones
        self.dev, self.dmask, self.dzones = ec.CellBuffer.from_vec(self.cells), ec.Mask.new(self.mask.astype(bool)), ec.CellBuffer.from_vec(zones)
        assert self.dev.mem.ptr % 16 == 0 and self.dmask.mem.ptr % 16 == 0 and self.dzones.mem.ptr % 16 == 0
        self.host, self.hmask, self.hzones = self.cells.tolist(), self.mask.tolist(), zones.tolist()

    def check(self, ec, space, nz, off, n, masked, what, with_compute=False):
        ct, zt = self.ct, self.zt
        cells, zones = self.host[off:off + n], self.hzones[off:off + n]
        mk = self.hmask[off:off + n] if masked else None
        refs = Z.records(ct, cells, zones, nz, mk)
        p, zp = self.dev.mem.ptr + off * size_of(ct), self.dzones.mem.ptr + off * Z.SIZE[zt]
        pm = (self.dmask.mem.ptr + off) if masked else None
        recs = device_records(ec, space, ct, p, pm, zt, zp, n, nz)
        for z in range(nz):
            assert_record(recs[z], refs[z], (what, "zone", z))
        if with_compute:
            st = compute(ec, ct, p, pm, zt, zp, n, nz)
            for z in range(nz):
                assert_stats(st[z], R.fold([refs[z]]), ct, (what, "compute, zone", z))
        return refs


def combos():
    """(zt, masked, n_zones): the three zone types, masked and not, the seven zone counts spread over them"""
    out = []
    for k, (zt, masked) in enumerate([(zt, m) for zt in Z.ZONE_TYPES for m in (False, True)]):
        out.append((zt, masked, [N_ZONES[k % 7], N_ZONES[(k + 3) % 7]]))
    return out


# ---------------------------------------------------------------- 1. every value type x zone type x mask, every n_zones
def type_cases(ct):
    """(zt, masked, nz, pattern, pool, offset, n, seed) of test 1: windows at cell offset 1 of both rasters, two tiles and a ragged rest"""
    n = 2 * Z.tile(ct) + Z.cpl(ct) + 3
    for zt, masked, counts in combos():
        for nz in counts:
            yield zt, masked, nz, "runs37" if nz > 2 else "edges", n + 3, 1, n, 0x20A1 + 16 * ct + nz


@pytest.mark.parametrize("ct", range(10), ids=lambda t: NAMES[t])
def test_records_every_type_zone_type_mask_and_zone_count(ec, space, ct):
    for zt, masked, nz, pattern, pool, off, n, seed in type_cases(ct):
        case = Case(ec, ct, zt, zone_ids(pattern, pool, nz, zt), seed)
        case.check(ec, space, nz, off, n, masked, (NAMES[ct], NAMES[zt], "masked", masked, "zones", nz, pattern), with_compute=True)


# ---------------------------------------------------------------- 2. every place a cell can be lost
@pytest.mark.parametrize("ct", range(10), ids=lambda t: NAMES[t])
def test_sizes(ec, space, ct):
    T, cpl = Z.tile(ct), Z.cpl(ct)
    sizes = [0, 1, cpl - 1, cpl, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
    zt = Z.ZONE_TYPES[ct % 3]
    nz = 65
    case = Case(ec, ct, zt, zone_ids("runs37", max(sizes) + 3, nz, zt), 0x512E + ct)
    for n in sizes:
        for masked in (False, True):
            case.check(ec, space, nz, 0, n, masked, (NAMES[ct], NAMES[zt], "n", n, "masked", masked), with_compute=n in (0, 1, T + 1))


@pytest.mark.parametrize("ct", [R.U8, R.I16, R.F32, R.F64], ids=lambda t: NAMES[t])
def test_offsets_of_both_rasters_under_both_alignment_plans(ec, space, ct):
    """Pointer offsets of 1 .. 15 bytes' worth of cells, the values' and the zones' independently: the two rasters are two
    allocations here, each with its own window."""
    T = Z.tile(ct)
    n, nz = T // 4 + 67, 64
    for zt in Z.ZONE_TYPES:
        voffs, zoffs = range(0, 15 // size_of(ct) + 1), range(0, 15 // Z.SIZE[zt] + 1)
        pool = n + 16
        cells, mask = random_cells(ct, pool, 0x0FF5 + ct), random_mask(pool, 0x0FF6 + ct)
        zones = zone_ids("runs37", pool, nz, zt)
        dev, dmask, dz = ec.CellBuffer.from_vec(cells), ec.Mask.new(mask.astype(bool)), ec.CellBuffer.from_vec(zones)
        host, hmask, hz = cells.tolist(), mask.tolist(), zones.tolist()
        pairs = [(v, 0) for v in voffs] + [(0, z) for z in zoffs if z] + [(max(voffs), max(zoffs))]
        for vo, zo in pairs:
            for masked in (False, True):
                refs = Z.records(ct, host[vo:vo + n], hz[zo:zo + n], nz, hmask[vo:vo + n] if masked else None)
                for knob in (1, 0):
                    with ec.tuned(unaligned_vector=knob):
                        recs = device_records(ec, space, ct, dev.mem.ptr + vo * size_of(ct), (dmask.mem.ptr + vo) if masked else None, zt,
                                              dz.mem.ptr + zo * Z.SIZE[zt], n, nz)
                    for z in range(nz):
                        assert_record(recs[z], refs[z], (NAMES[ct], NAMES[zt], "offsets", vo, zo, "masked", masked, "unaligned_vector", knob, "zone", z))


@pytest.mark.parametrize("ct", [R.U8, R.U32, R.F64], ids=lambda t: NAMES[t])
def test_cellwise_plan_several_workgroups(ec, space, ct):
    """unaligned_vector = 0 at an odd offset: the cell-wise kernel with several workgroups, and under reduce_bpc = 1 further rounds."""
    n, nz, zt = 70001, 63, Z.ZONE_TYPES[ct % 3]
    case = Case(ec, ct, zt, zone_ids("runs37", n + 1, nz, zt), 0xCE77 + ct)
    for knobs in ({"unaligned_vector": 0}, {"unaligned_vector": 0, "reduce_bpc": 1}):
        with ec.tuned(**knobs):
            case.check(ec, space, nz, 1, n, True, (NAMES[ct], knobs))


# ---------------------------------------------------------------- 3. zone patterns
PATTERN_TYPES = ((R.U16, R.U8, True), (R.F32, R.U16, False), (R.I64, R.I32, True))


def pattern_cases(pattern):
    """(ct, zt, masked, nz, n, seed) of test 3: two tiles and one cell, at every zone count"""
    for ct, zt, masked in PATTERN_TYPES:
        for nz in N_ZONES:
            yield ct, zt, masked, nz, 2 * Z.tile(ct) + 1, 0x9A77 + nz


@pytest.mark.parametrize("pattern", PATTERNS)
def test_zone_patterns_at_every_zone_count(ec, space, pattern):
    for ct, zt, masked, nz, n, seed in pattern_cases(pattern):
        case = Case(ec, ct, zt, zone_ids(pattern, n, nz, zt), seed)
        case.check(ec, space, nz, 0, n, masked, (pattern, NAMES[ct], NAMES[zt], "zones", nz))


@pytest.mark.parametrize("ct,zt", [(R.U8, R.U8), (R.F64, R.I32)], ids=["u8-u8", "f64-i32"])
def test_a_zone_of_one_cell_wherever_it_is_planted(ec, space, ct, zt):
    """Zone nz - 1 holds exactly one cell: at the peeled head, in the first and last lane of the first and last wave of the first
    tile, at the tile's edge, in the last workgroup's tile and in the ragged tail."""
    T, cpl, nz = Z.tile(ct), Z.cpl(ct), 5
    off = 1                                         # an odd offset: the kernel peels head cells
    head = ((16 - off * size_of(ct)) % 16) // size_of(ct)
    n = head + 3 * T + cpl + 2
    lanes = [0, Z.WAVE - 1, Z.BLOCK - Z.WAVE, Z.BLOCK - 1]
    spots = [0, head - 1] + [head + lane * cpl + k for lane in lanes for k in (0, cpl - 1)] + [head + T - 1, head + T, head + 2 * T + 17, n - 1, n - 2]
    cells = random_cells(ct, n + off, 0x51C + ct)
    mask = np.ones(n + off, dtype=np.uint8)
    dev, dmask = ec.CellBuffer.from_vec(cells), ec.Mask.new(mask.astype(bool))
    for spot in sorted(set(s for s in spots if 0 <= s < n)):
        zones = np.zeros(n + off, dtype=ZNP[zt])
        zones[off + spot] = nz - 1
        dz = ec.CellBuffer.from_vec(zones)
        refs = Z.records(ct, cells[off:].tolist(), zones[off:].tolist(), nz)
        assert refs[nz - 1]["count"] == 1 and refs[0]["count"] == n - 1
        recs = device_records(ec, space, ct, dev.mem.ptr + off * size_of(ct), dmask.mem.ptr + off, zt, dz.mem.ptr + off * Z.SIZE[zt], n, nz)
        for z in range(nz):
            assert_record(recs[z], refs[z], (NAMES[ct], "one cell at", spot, "zone", z))


@pytest.mark.parametrize("ct", [R.U32, R.F64], ids=lambda t: NAMES[t])
def test_grid_stride_second_round(ec, space, ct):
    """reduce_bpc = 1: one workgroup per CU (at most 256 of them), so 257 tiles and a ragged rest take the grid-stride loop into
    a second round."""
    T, nz, zt = Z.tile(ct), 64, R.U8
    n = 257 * T + 2 * Z.cpl(ct) + 1
    case = Case(ec, ct, zt, zone_ids("runs37", n, nz, zt), 0x2D0 + ct)
    with ec.tuned(reduce_bpc=1):
        case.check(ec, space, nz, 0, n, True, (NAMES[ct], "second round"))


# ---------------------------------------------------------------- 4. what a foreign or hidden cell holds does not matter
def poison_inputs(ct):
    """(cells, zones, mask, nz, zt): every cell that belongs to no zone — hidden, or under a foreign id — is NaN, +Inf or -Inf, the first
    cell among them, so the pivot is 0.0 and the sums must stay exact"""
    T, nz, zt = Z.tile(ct), 7, R.I32
    n = 2 * T + 3
    rng = np.random.default_rng(0xBAD2 + ct)
    base = 0 if ct == R.F32 else 2**16
    vis = (rng.integers(1, 512, size=n, endpoint=True) * rng.choice(np.array([-1, 1]), size=n) + base).astype(NP[ct])
    poison = np.array([np.nan, np.inf, -np.inf], dtype=NP[ct])[rng.integers(0, 3, size=n)]
    zones = zone_ids("random", n, nz, zt, seed=5)
    mask = random_mask(n, 0xBAD3)
    mask[0] = 1 if not 0 <= zones[0] < nz else 0
    counted = mask.astype(bool) & (zones >= 0) & (zones < nz)
    cells = np.where(counted, vis, poison).astype(NP[ct])
    assert not np.isfinite(cells[0])
    return cells, zones, mask, nz, zt


@pytest.mark.parametrize("ct", [R.F32, R.F64], ids=lambda t: NAMES[t])
def test_nan_and_infinities_under_cleared_mask_bytes_and_foreign_ids(ec, space, ct):
    cells, zones, mask, nz, zt = poison_inputs(ct)
    n = cells.size
    dev, dmask, dz = ec.CellBuffer.from_vec(cells), ec.Mask.new(mask.astype(bool)), ec.CellBuffer.from_vec(zones)
    refs = Z.records(ct, cells.tolist(), zones.tolist(), nz, mask.tolist())
    assert all(r["s1_exact"] is not None and r["count"] > 0 and r["pivot"] == 0.0 for r in refs)
    recs = device_records(ec, space, ct, dev.mem.ptr, dmask.mem.ptr, zt, dz.mem.ptr, n, nz)
    for z in range(nz):
        assert_record(recs[z], refs[z], (NAMES[ct], "poison", "zone", z))


# ---------------------------------------------------------------- 5. determinism and general data
def general_case(ec):
    n, nz = 2 * Z.tile(R.F64) + 5, 37
    cells = np.random.default_rng(0x6E4).standard_normal(n) * 1e3 + 1e6
    zones = zone_ids("random", n, nz, R.U8, seed=0x6E6)
    mask = random_mask(n, 0x6E5)
    return n, nz, cells, zones, mask, ec.CellBuffer.from_vec(cells), ec.CellBuffer.from_vec(zones), ec.Mask.new(mask.astype(bool))


def test_same_call_twice_gives_the_same_bytes(ec, space):
    n, nz, _, _, _, dev, dz, dmask = general_case(ec)
    for pm in (None, dmask.mem.ptr):
        a = bytes(device_records(ec, space, R.F64, dev.mem.ptr, pm, R.U8, dz.mem.ptr, n, nz))
        b = bytes(device_records(ec, space, R.F64, dev.mem.ptr, pm, R.U8, dz.mem.ptr, n, nz))
        assert a == b and len(a) == nz * 64


def test_general_f64_every_zone_within_the_summation_bound(ec, space):
    """The bound of test_gpu_stats.py's whole-raster test, per zone: |s1 - exact| <= gamma * sum|d|, |s2 - exact| <= gamma * sum d^2,
    gamma = (m + 1) u / (1 - (m + 1) u) for the m cells of the zone, u = 2^-53 (any summation order of m terms, one more rounding
    for the fma).  Every zone is checked."""
    n, nz, cells, zones, mask, dev, dz, dmask = general_case(ec)
    u = Fraction(1, 2**53)
    for pm, mk in ((None, None), (dmask.mem.ptr, mask.tolist())):
        refs = Z.records(R.F64, cells.tolist(), zones.tolist(), nz, mk)
        recs = device_records(ec, space, R.F64, dev.mem.ptr, pm, R.U8, dz.mem.ptr, n, nz)
        for z in range(nz):
            ref, rec = refs[z], recs[z]
            m = ref["count"]
            gamma = (m + 1) * u / (1 - (m + 1) * u)
            e1, e2 = abs(Fraction(rec.u.f.s1) - ref["s1_exact"]), abs(Fraction(rec.u.f.s2) - ref["s2_exact"])
            print("zone", z, "masked" if mk else "unmasked", "cells", m, "err s1", float(e1), "bound", float(gamma * ref["abs_d"]), "err s2", float(e2),
                  "bound", float(gamma * ref["sq_d"]))
            assert m > 0 and rec.count == m and bits(rec.u.f.pivot) == bits(ref["pivot"])
            assert e1 <= gamma * ref["abs_d"] and e2 <= gamma * ref["sq_d"]
            assert float(ref["abs_d"]) / m > 100 * float(gamma * ref["abs_d"])  # a lost cell could not hide inside the bound


# ---------------------------------------------------------------- 6. the Python mirror
def test_python_mirror_bit_for_bit(ec):
    n, nz = Z.tile(R.I16) + 77, 9
    for ct, zt in ((R.I16, R.U8), (R.F64, R.U16), (R.U64, R.I32)):
        cells, mask, zones = random_cells(ct, n, 0x717 + ct), random_mask(n, 0x718), zone_ids("edges", n, nz, zt)
        buf, zb = ec.CellBuffer.from_vec(cells), ec.CellBuffer.from_vec(zones)
        for mk in (None, mask):
            got = (buf if mk is None else ec.MaskedCellBuffer(buf, ec.Mask.new(mk.astype(bool)))).zonal_stats(zb, nz)
            want = Z.stats(ct, cells.tolist(), zones.tolist(), nz, None if mk is None else mk.tolist())
            assert len(got) == nz
            for z in range(nz):
                assert got[z].count == want[z]["count"]
                for name in ("sum", "mean", "stddev"):
                    g, w = getattr(got[z], name), want[z][name]
                    assert bits(g) == bits(w) or (np.isnan(g) and np.isnan(w)), (NAMES[ct], z, name, g, w)
                assert (R.order_key(ct, got[z].min.value.item()), R.order_key(ct, got[z].max.value.item())) == \
                    (R.order_key(ct, want[z]["min"]), R.order_key(ct, want[z]["max"]))
    # the way back: anomaly = value - mean of its zone
    means = np.array([s["mean"] if s["count"] else 0.0 for s in want])
    back = zb.broadcast(means, ec.Float64)
    exp, emask = Z.broadcast(zones.tolist(), means.tolist(), nz)
    assert back.buffer().to_numpy().tolist() == exp and back.mask().to_numpy().astype(np.uint8).tolist() == emask


# ---------------------------------------------------------------- 7. broadcast
@pytest.mark.parametrize("zt", Z.ZONE_TYPES, ids=lambda t: NAMES[t])
def test_broadcast_every_cell_type_size_and_offset(ec, zt):
    L, E = ec.lib(), ec._ffi
    nz = 200
    for ct in range(10):
        T, cpl, sz = Z.broadcast_tile(ct, zt), Z.broadcast_cpl(ct, zt), size_of(ct)
        sizes = [0, 1, cpl - 1, cpl, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
        pool = max(sizes) + 16
        zones = zone_ids("random", pool, nz, zt, seed=0xB0 + ct)
        zones[::11] = Z.ZONE_RANGE[zt][1]  # the type's maximum: foreign
        table = random_cells(ct, nz, 0xB1 + ct)
        dz, dt = ec.CellBuffer.from_vec(zones), ec.CellBuffer.from_vec(table)
        out, om = ec.DeviceMem((pool + 16) * sz), ec.DeviceMem(pool + 16)
        hz, ht = zones.tolist(), table.tolist()
        for n, zo, oo, knob, with_mask in [(n, 0, 0, 1, True) for n in sizes] + [(T + 65, zo, 0, k, True) for zo in (1, 3, 15 // Z.SIZE[zt]) for k in (1, 0)] + \
                                          [(T + 65, 0, oo, k, m) for oo in (1, 15 // sz) for k in (1, 0) for m in (True, False)]:
            exp, emask = Z.broadcast(hz[zo:zo + n], ht, nz)
            E.check(L.ec_upload(out.ptr, b"\x5a" * ((pool + 16) * sz), (pool + 16) * sz, None))
            E.check(L.ec_upload(om.ptr, b"\x5a" * (pool + 16), pool + 16, None))
            with ec.tuned(unaligned_vector=knob):
                E.check(L.ec_zonal_broadcast(zt, dz.mem.ptr + zo * Z.SIZE[zt], n, nz, ct, dt.mem.ptr, out.ptr + oo * sz, (om.ptr + oo) if with_mask else None, None))
            got = np.empty(n, dtype=NP[ct])
            gm = np.empty(n, dtype=np.uint8)
            if n:
                E.check(L.ec_download(got.ctypes.data, out.ptr + oo * sz, n * sz, None))
                E.check(L.ec_download(gm.ctypes.data, om.ptr + oo, n, None))
            what = (NAMES[zt], NAMES[ct], "n", n, "offsets", zo, oo, "unaligned_vector", knob, "mask", with_mask)
            assert got.tobytes() == np.array(exp, dtype=NP[ct]).tobytes(), what
            assert gm.tolist() == (emask if with_mask else [0x5a] * n), what


# ---------------------------------------------------------------- the C++ mirror
def test_cpp_mirror_zonal_program():
    """erased-cells_amd/host/test_zonal_mirror.cpp: zonal_stats() / broadcast() of the C++ host mirror, whole, masked and sharded, on
    hand-checkable cells and against the C ABI called directly."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = os.path.join(root, "erased-cells_amd", "host")
    binary = os.path.join(host, "test_zonal_mirror")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", host, "-s", "test_zonal_mirror"])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
