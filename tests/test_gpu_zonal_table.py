"""The zonal table family on the device (ec_zonal_table_device / ec_zonal_table_compute / ec_zonal_lookup and the Python mirror's
`zonal_table()` / `lookup()`) against tests/zonal_table_ref.py — never against the library itself.  Every record is compared as its
64 bytes: for the exact integer kind that is count, keys and the exact sums; for the pivoted f64 kind the truncated fixed-point
sums of the header's rule, bit for bit, on planted, hand-worked and general data alike — the rule has one answer whatever the
launch shape or the order of the cells, and tests 4 and 5 hold the kernels to that.

Sizes come from the kernels' tile, restated in zonal_table_ref (256 threads x 4 loads of 16 bytes of values); the inputs from
tests/zonal_table_cases.py, where tests/test_zonal_table_faults.py shows what each of them is there to expose."""
import ctypes as C
import threading

import numpy as np
import pytest

import stats_ref as R
import zonal_ref as Z
import zonal_table_cases as K
import zonal_table_ref as ZT
from test_gpu_stats import NAMES, NP, random_cells, random_mask, size_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


@pytest.fixture(scope="module")
def space(ec):
    """workspace and record memory per (kind, n_zones), allocated once"""
    made = {}

    def get(ct, nz):
        key = (R.KIND[ct], nz)
        if key not in made:
            made[key] = (ec.DeviceMem(ec.lib().ec_zonal_table_workspace_bytes(ct, nz)), ec.DeviceMem(nz * 64))
        return made[key]
    return get


def device_bytes(ec, space, ct, p, pm, zt, zp, n, nz, stream=None):
    """the n_zones records of one call, as bytes; the block is pre-filled so that a record left unwritten would show"""
    L, E = ec.lib(), ec._ffi
    ws, out = space(ct, nz)
    fill = np.full(nz * 64, 0xA5, dtype=np.uint8)
    E.check(L.ec_upload(out.ptr, fill.ctypes.data, nz * 64, stream))
    E.check(L.ec_zonal_table_device(ct, p, pm, zt, zp, n, nz, out.ptr, ws.ptr, stream))
    got = np.empty(nz * 64, dtype=np.uint8)
    E.check(L.ec_download(got.ctypes.data, out.ptr, nz * 64, stream))
    return got.tobytes()


def first_difference(got, want):
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    assert a.size == b.size
    bad = np.flatnonzero(a != b)
    if bad.size == 0:
        return None
    z = int(bad[0]) // 64
    return z, got[64 * z:64 * z + 64].hex(), want[64 * z:64 * z + 64].hex()


class Raster:
    """cells, mask bytes and ids on the device; a call sees the window [off : off + n]"""

    def __init__(self, ec, ct, zt, cells, mask, zones):
        self.ct, self.zt = ct, zt
        self.cells, self.mask, self.zones = cells, mask, zones
        self.dev, self.dmask, self.dz = ec.CellBuffer.from_vec(cells), ec.Mask.new(mask.astype(bool)), ec.CellBuffer.from_vec(zones)
        self.host, self.hmask, self.hz = cells.tolist(), mask.tolist(), zones.tolist()

    def ptrs(self, off, masked):
        return self.dev.mem.ptr + off * size_of(self.ct), (self.dmask.mem.ptr + off) if masked else None, self.dz.mem.ptr + off * Z.SIZE[self.zt]

    def want(self, off, n, nz, masked):
        return ZT.records(self.ct, self.host[off:off + n], self.hz[off:off + n], nz, self.hmask[off:off + n] if masked else None)

    def check(self, ec, space, nz, off, n, masked, what):
        p, pm, zp = self.ptrs(off, masked)
        got = device_bytes(ec, space, self.ct, p, pm, self.zt, zp, n, nz)
        assert first_difference(got, K.table_bytes(self.want(off, n, nz, masked))) is None, what
        return got


# ---------------------------------------------------------------- 1. kind 0 over every value type class; kind 1 where the sums are exact
@pytest.mark.parametrize("case", list(K.kind0_cases()) + list(K.kind1_exact_cases()), ids=lambda c: f"{NAMES[c[0]]}-{NAMES[c[1]]}-{c[3]}-{c[4]}")
def test_records_every_type_zone_type_mask_and_pattern(ec, space, case):
    ct, zt, masked, nz, pattern, n, off, seed = case
    cells, mask, zones = K.arrays(ct, zt, nz, pattern, n, off, seed)
    r = Raster(ec, ct, zt, cells, mask, zones)
    got = r.check(ec, space, nz, off, n, masked, case)
    if R.KIND[ct] == 0 and nz <= Z.MAX_ZONES:   # byte-identical to the LDS family's records
        L, E = ec.lib(), ec._ffi
        ws, out = ec.DeviceMem(L.ec_zonal_workspace_bytes(nz)), ec.DeviceMem(nz * 64)
        p, pm, zp = r.ptrs(off, masked)
        E.check(L.ec_zonal_stats_device(ct, p, pm, zt, zp, n, nz, out.ptr, ws.ptr, None))
        old = np.empty(nz * 64, dtype=np.uint8)
        E.check(L.ec_download(old.ctypes.data, out.ptr, nz * 64, None))
        assert old.tobytes() == got


# ---------------------------------------------------------------- 2. the planted and hand-worked zones, bit for bit
@pytest.mark.parametrize("zt", [R.I32, R.U16, R.U8], ids=lambda t: NAMES[t])
def test_planted_and_hand_worked_zones(ec, space, zt):
    cells, zones, mask, nz = K.planted_raster(zt)
    r = Raster(ec, R.F64, zt, cells, mask, zones)
    for knobs in ({}, {"reduce_bpc": 1}, {"unaligned_vector": 0}):
        with ec.tuned(**knobs):
            r.check(ec, space, nz, 0, cells.size, True, ("planted", NAMES[zt], knobs))


# ---------------------------------------------------------------- 3. every place a cell can be lost
@pytest.mark.parametrize("ct", [R.U16, R.F64, R.F32, R.U8], ids=lambda t: NAMES[t])
def test_sizes_and_offsets(ec, space, ct):
    T = ZT.tile(ct)
    sizes, offsets = [0, 1, T - 1, T, T + 1, 2 * T + 5], (0, 1, 3)
    if ct == R.U8:   # the longest peel: 16 cells a group, a head of up to 15 cells, which whole waves walk with the ragged tail
        sizes, offsets = [0, 1, 15, 16, 17, T + 1], (0, 1, 15)
    zt, nz = Z.ZONE_TYPES[ct % 3], 257
    cells, mask, zones = K.arrays(ct, zt, nz, "runs37", max(sizes), max(offsets), 0x512E + ct)
    r = Raster(ec, ct, zt, cells, mask, zones)
    for n in sizes:
        for off in offsets:
            for masked in (False, True):
                r.check(ec, space, nz, off, n, masked, (NAMES[ct], "n", n, "offset", off, "masked", masked))


def test_grid_stride_second_round(ec, space):
    """reduce_bpc = 1: one workgroup per CU (at most 256 of them), so 257 tiles and a ragged rest take the grid-stride loop into a
    second round; general data, so kind 1 truncates."""
    ct, zt, nz = R.F64, R.U8, 64
    n = 257 * ZT.tile(ct) + 2 * ZT.cpl(ct) + 1
    cells, zones, mask = K.general_raster(n, nz, zt, seed=0x2D0)
    r = Raster(ec, ct, zt, cells, mask, zones)
    with ec.tuned(reduce_bpc=1):
        r.check(ec, space, nz, 0, n, True, "second round")


@pytest.mark.parametrize("pattern", K.PATTERNS)
def test_zone_patterns(ec, space, pattern):
    for ct, zt, masked in ((R.U16, R.U16, True), (R.F64, R.I32, False)):
        n = 2 * ZT.tile(ct) + 5
        nz = n if pattern == "own" else 4097
        cells, mask = random_cells(ct, n, 0x9A77 + ct), random_mask(n, 0x9A78)
        if ct == R.F64:
            cells = K.general_raster(n, 2, R.U8, seed=0x9A79)[0]
        r = Raster(ec, ct, zt, cells, mask, K.ids(pattern, n, nz, zt))
        r.check(ec, space, nz, 0, n, masked, (pattern, NAMES[ct], NAMES[zt]))


# ---------------------------------------------------------------- 4. 2^16 zones and more: ids 0, K - 1 and K; the empty records in bulk
@pytest.mark.parametrize("nz", K.BIG_K)
def test_many_zones(ec, space, nz):
    for ct, zt, masked in ((R.F64, R.I32, True), (R.U32, R.U16, False), (R.I16, R.I32, True)):
        cells, mask, zones = K.big_k_case(nz, zt, ct, 0xB16 + nz % 97)
        found, empty = ZT.sparse_records(ct, cells.tolist(), zones.tolist(), nz, mask.tolist() if masked else None)
        r = Raster(ec, ct, zt, cells, mask, zones)
        p, pm, zp = r.ptrs(0, masked)
        got = device_bytes(ec, space, ct, p, pm, zt, zp, cells.size, nz)
        assert first_difference(got, K.sparse_table_bytes(found, empty, nz)) is None, (nz, NAMES[ct], NAMES[zt])


# ---------------------------------------------------------------- 5. one answer: twice, under another launch shape, in another order
def test_same_bytes_twice_under_another_grid_and_in_another_order(ec, space):
    ct, zt, nz = R.F64, R.U16, 300
    n = 6 * ZT.tile(ct) + 7
    cells, zones, mask = K.general_raster(n, nz, zt, seed=0x0DE4)
    cells[5] = 2.0**90       # a zone that truncates
    r = Raster(ec, ct, zt, cells, mask, zones)
    want = K.table_bytes(r.want(0, n, nz, True))
    a = r.check(ec, space, nz, 0, n, True, "first")
    assert r.check(ec, space, nz, 0, n, True, "second") == a == want
    with ec.tuned(reduce_bpc=1):
        assert r.check(ec, space, nz, 0, n, True, "one workgroup per CU") == a
    with ec.tuned(unaligned_vector=0):
        assert r.check(ec, space, nz, 0, n, True, "cell-wise") == a
    order = np.concatenate([[0], 1 + np.random.default_rng(0x5AFE).permutation(n - 1)])   # cell 0 keeps the pivot
    shuffled = Raster(ec, ct, zt, cells[order], mask[order], zones[order])
    p, pm, zp = shuffled.ptrs(0, True)
    assert device_bytes(ec, space, ct, p, pm, zt, zp, n, nz) == a


# ---------------------------------------------------------------- 6. compute and the Python mirror
def assert_rows(rows, want, ct, what):
    assert rows.dtype.names == ("count", "min", "max", "sum", "mean", "stddev") and rows.size == len(want), what
    assert rows["count"].tolist() == [w["count"] for w in want], what
    for name in ("sum", "mean", "stddev"):
        g, w = rows[name], np.array([x[name] for x in want], dtype=np.float64)
        assert np.array_equal(g.view(np.uint64)[~np.isnan(w)], w.view(np.uint64)[~np.isnan(w)]) and np.array_equal(np.isnan(g), np.isnan(w)), (what, name)
    for name in ("min", "max"):
        assert rows[name].tobytes() == np.array([x[name] for x in want], dtype=NP[ct]).tobytes(), (what, name)


def test_compute_and_python_mirror_bit_for_bit(ec):
    n, nz = ZT.tile(R.I16) + 77, 300
    for ct, zt in ((R.I16, R.U16), (R.F64, R.U16), (R.U64, R.I32)):
        cells, mask, zones = random_cells(ct, n, 0x717 + ct), random_mask(n, 0x718), K.ids("edges", n, nz, zt)
        if ct == R.F64:
            cells = K.general_raster(n, 2, R.U8, seed=0x719)[0]
        buf, zb = ec.CellBuffer.from_vec(cells), ec.CellBuffer.from_vec(zones)
        for mk in (None, mask):
            want = ZT.stats(ct, cells.tolist(), zones.tolist(), nz, None if mk is None else mk.tolist())
            rows = (buf if mk is None else ec.MaskedCellBuffer(buf, ec.Mask.new(mk.astype(bool)))).zonal_table(zb, nz)
            assert_rows(rows, want, ct, (NAMES[ct], "python", mk is not None))
            raw = np.empty(nz, dtype=ec.buffer._EC_STATS_DTYPE)
            ec._ffi.check(ec.lib().ec_zonal_table_compute(ct, buf.mem.ptr, None if mk is None else ec.Mask.new(mk.astype(bool)).mem.ptr, zt, zb.mem.ptr, n, nz,
                                                          raw.ctypes.data, None))
            assert_rows(ec.buffer.stats_table(raw, ct), want, ct, (NAMES[ct], "compute", mk is not None))


def test_regions_then_zonal_table_then_lookup(ec):
    """the chain the family closes: labels of a speckled class raster (K > 256), statistics per label, the means back in the raster"""
    cols, rows = 96, 80
    rng = np.random.default_rng(0x9E610)
    classes = rng.integers(0, 3, size=cols * rows).astype(np.uint8)
    values = rng.standard_normal(cols * rows) * 1e3 + 1e6
    labels, k = ec.CellBuffer.from_vec(classes).regions(cols)
    assert k > 256
    lab = labels.buffer() if hasattr(labels, "buffer") else labels
    host_labels = lab.to_numpy()
    assert host_labels.dtype == np.int32 and host_labels.max() == k
    per = ec.CellBuffer.from_vec(values).zonal_table(lab, k + 1)
    want = ZT.stats(R.F64, values.tolist(), host_labels.tolist(), k + 1)
    assert_rows(per, want, R.F64, "regions")
    assert int(per["count"].sum()) == cols * rows
    back = lab.lookup(per["mean"])
    exp, emask = ZT.lookup(host_labels.tolist(), per["mean"].tolist(), k + 1)
    assert back.buffer().to_numpy().tobytes() == np.array(exp, dtype=np.float64).tobytes()
    assert back.mask().to_numpy().astype(np.uint8).tolist() == emask


# ---------------------------------------------------------------- 7. the lookup
@pytest.mark.parametrize("nz", K.LOOKUP_ZONES)
def test_lookup_every_cell_width_size_and_offset(ec, nz):
    L, E = ec.lib(), ec._ffi
    for ct, zt in K.LOOKUP_PAIRS:
        T, cpl, sz = Z.broadcast_tile(ct, zt), Z.broadcast_cpl(ct, zt), size_of(ct)
        sizes = [0, 1, cpl - 1, cpl, T - 1, T, T + 1, 2 * T + 5]
        pool = max(sizes) + 16
        zones, table = K.lookup_arrays(ct, zt, nz, pool)
        dz, dt = ec.CellBuffer.from_vec(zones), ec.CellBuffer.from_vec(table)
        out, om = ec.DeviceMem((pool + 16) * sz), ec.DeviceMem(pool + 16)
        hz, ht = zones.tolist(), table.tolist()
        fill, mfill = np.full((pool + 16) * sz, 0x5A, dtype=np.uint8), np.full(pool + 16, 0x5A, dtype=np.uint8)
        for n, zo, oo, knob, with_mask in [(n, 0, 0, 1, True) for n in sizes] + [(T + 65, zo, oo, k, m) for zo, oo in ((1, 0), (3, 1), (0, 3)) for k in (1, 0) for m in (True, False)]:
            exp, emask = ZT.lookup(hz[zo:zo + n], ht, nz)
            E.check(L.ec_upload(out.ptr, fill.ctypes.data, fill.size, None))
            E.check(L.ec_upload(om.ptr, mfill.ctypes.data, mfill.size, None))
            with ec.tuned(unaligned_vector=knob):
                E.check(L.ec_zonal_lookup(zt, dz.mem.ptr + zo * Z.SIZE[zt], n, nz, ct, dt.mem.ptr, out.ptr + oo * sz, (om.ptr + oo) if with_mask else None, None))
            got, gm = np.empty(n, dtype=NP[ct]), np.empty(n, dtype=np.uint8)
            if n:
                E.check(L.ec_download(got.ctypes.data, out.ptr + oo * sz, n * sz, None))
                E.check(L.ec_download(gm.ctypes.data, om.ptr + oo, n, None))
            what = (NAMES[zt], NAMES[ct], "zones", nz, "n", n, "offsets", zo, oo, "unaligned_vector", knob, "mask", with_mask)
            assert got.tobytes() == np.array(exp, dtype=NP[ct]).tobytes(), what
            assert gm.tolist() == (emask if with_mask else [0x5A] * n), what


# ---------------------------------------------------------------- 8. four host threads, a stream each
def test_four_threads_on_streams_of_their_own(ec):
    L, E = ec.lib(), ec._ffi
    ct, zt, nz = R.F64, R.I32, 1000
    n = 3 * ZT.tile(ct) + 11
    jobs, errors = [], []
    for k in range(4):
        cells, zones, mask = K.general_raster(n, nz, zt, seed=0x7EAD + k)
        cells[3 + k] = 2.0**(80 + k)
        jobs.append((Raster(ec, ct, zt, cells, mask, zones), ec.DeviceMem(L.ec_zonal_table_workspace_bytes(ct, nz)), ec.DeviceMem(nz * 64)))
    wants = [K.table_bytes(r.want(0, n, nz, True)) for r, _, _ in jobs]
    gots, streams = [None] * 4, [C.c_void_p() for _ in range(4)]
    for s in streams:
        E.check(L.ec_stream_create(C.byref(s)))

    def work(k):
        try:
            r, ws, out = jobs[k]
            s = streams[k]
            p, pm, zp = r.ptrs(0, True)
            E.check(L.ec_zonal_table_device(ct, p, pm, zt, zp, n, nz, out.ptr, ws.ptr, s))
            got = np.empty(nz * 64, dtype=np.uint8)
            E.check(L.ec_download(got.ctypes.data, out.ptr, nz * 64, s))
            E.check(L.ec_stream_sync(s))
            gots[k] = got.tobytes()
        except Exception as e:  # noqa: BLE001 — reported by the main thread
            errors.append((k, repr(e)))
    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for s in streams:
        E.check(L.ec_stream_sync(s))
        E.check(L.ec_release_stream(s))
        E.check(L.ec_stream_destroy(s))
    assert not errors, errors
    for k in range(4):
        assert first_difference(gots[k], wants[k]) is None, k


# ---------------------------------------------------------------- the C++ mirror
def test_cpp_mirror_zonal_table_program():
    """erased-cells_amd/host/test_zonal_table_mirror.cpp: zonal_table() / lookup() of the C++ host mirror, whole, masked and sharded, with
    more than 256 zones, on hand-checkable cells and against the C ABI called directly."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = os.path.join(root, "erased-cells_amd", "host")
    binary = os.path.join(host, "test_zonal_table_mirror")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", host, "-s", "test_zonal_table_mirror"])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
