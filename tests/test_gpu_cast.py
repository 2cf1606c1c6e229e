"""ec_cast / ec_cast_scaled on the GPU against tests/cast_ref.py — bit for bit.  The one exception is the one the header states:
where the destination is a float type and the restatement itself is a NaN, a NaN of the same sign is accepted.

Per source type (one test each, not one per pair): all 10 destinations x both modes at n = 2 T + 16 / widest + 1 cells
(T = 256 x 2 x 16 / widest: an unguarded tile, the guarded last tile, the cell tail), the special values tiled through; both
settings of `unaligned_vector` at a one-cell offset on every pointer (the knob decides between the vector and the cell-wise
kernel); both modes again under each forced load policy (cache_force 0..3: the unforced calls are small enough for the
cache plan to admit them, so only the forced ones reach the nt arm).  ec_cast_scaled for one source per byte width (and both float types) into every
destination, four (scale, offset) pairs, with and without a mask, NaNs under cleared and under set mask bytes.  No call
allocates.  Then the Python mirror and the C++ mirror.  tests/test_cast_faults.py shows (without a GPU) that these inputs
notice a wrong kernel.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cast_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT, NP, NAMES = R.NT, R.NP, R.NAMES


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def _stat(ec, key):
    v = C.c_int64(0)
    ec._ffi.check(ec.lib().ec_stat_get(key, C.byref(v)))
    return v.value


class Dev:
    """An array on the device one cell behind an allocation's start as well as at it: `at(0)` is 256-byte aligned, `at(1)` is not
    16-byte aligned for any cell width."""

    def __init__(self, ec, a):
        self.a = np.ascontiguousarray(a)
        self.sz = self.a.dtype.itemsize
        self.mem = ec.DeviceMem((self.a.size + 1) * self.sz)
        self.ec = ec
        self._at = None

    def at(self, off):
        if self._at != off:
            self.ec._ffi.check(self.ec.lib().ec_upload(self.mem.ptr + off * self.sz, self.a.ctypes.data_as(C.c_void_p), self.a.nbytes, self.ec.stream()))
            self._at = off
        return self.mem.ptr + off * self.sz


class Out:
    """n cells of type dt (and one more in front), read back as that type."""

    def __init__(self, ec, n, dt):
        self.ec, self.n, self.dt = ec, n, NP[dt]
        self.mem = ec.DeviceMem((n + 1) * self.dt.itemsize + 16)

    def at(self, off):
        return self.mem.ptr + off * self.dt.itemsize

    def read(self, off):
        out = np.empty(self.n, self.dt)
        self.ec._ffi.check(self.ec.lib().ec_download(out.ctypes.data_as(C.c_void_p), self.at(off), out.nbytes, self.ec.stream()))
        return out


def _same(got, want, x, what):
    bad = np.flatnonzero(~R.same_cells(got, want))
    assert bad.size == 0, f"{what}: {bad.size} cells differ, first at {int(bad[0])} of {got.size}: {x[bad[0]]!r} -> got {got[bad[0]]!r}, want {want[bad[0]]!r}"


@pytest.mark.parametrize("st", range(NT), ids=NAMES)
def test_cast_into_all_destinations(ec, st):
    L, chk, E = ec.lib(), ec._ffi.check, ec._ffi
    for dt in range(NT):
        x = R.gpu_inputs(st, dt)
        n = x.size
        dx, out = Dev(ec, x), Out(ec, n, dt)
        want = {mode: R.cast(mode, st, x, dt) for mode in R.MODES}
        p0 = dx.at(0)
        before = _stat(ec, b"pool_allocs")
        for mode in R.MODES:
            chk(L.ec_cast(mode, st, p0, dt, out.at(0), n, ec.stream()))
            _same(out.read(0), want[mode], x, f"ec_cast mode {mode} {NAMES[st]} -> {NAMES[dt]}")
        for bits in (0, 1, 2, 3):   # the load policy forced: every kernel (a mode is a kernel of its own) under its nt arm and its default arm
            with ec.tuned(cache_force=bits):
                for mode in R.MODES:
                    chk(L.ec_cast(mode, st, p0, dt, out.at(0), n, ec.stream()))
                    _same(out.read(0), want[mode], x, f"cache_force {bits} mode {mode} {NAMES[st]} -> {NAMES[dt]}")
        p1 = dx.at(1)               # a one-cell offset on both pointers: the vector kernel (unaligned_vector = 1) and the cell-wise one (0)
        for uv in (1, 0):
            with ec.tuned(unaligned_vector=uv):
                for mode in R.MODES:
                    chk(L.ec_cast(mode, st, p1, dt, out.at(1), n, ec.stream()))
                    _same(out.read(1), want[mode], x, f"unaligned_vector {uv} mode {mode} {NAMES[st]} -> {NAMES[dt]}")
        assert _stat(ec, b"pool_allocs") == before, "an ec_cast call allocated"
        if R.can_fit_into(st, dt) and st != dt:   # a pair that fits: exactly ec_convert's cells
            chk(L.ec_cast(R.ROUND, st, p1, dt, out.at(0), n, ec.stream()))
            cast_cells = out.read(0).tobytes()
            chk(L.ec_convert(st, p1, dt, out.at(0), n, ec.stream()))
            assert out.read(0).tobytes() == cast_cells, f"ec_cast against ec_convert {NAMES[st]} -> {NAMES[dt]}"


@pytest.mark.parametrize("st", R.SCALED_SOURCES, ids=lambda c: NAMES[c])
def test_cast_scaled_into_all_destinations(ec, st):
    L, chk = ec.lib(), ec._ffi.check
    for dt in range(NT):
        x, m = R.scaled_inputs(st, dt)
        n = x.size
        nd = R.nodata_of(dt)
        v = ec.CellValue(dt, nd).to_ec()
        dx, dm, out = Dev(ec, x), Dev(ec, m), Out(ec, n, dt)
        px, pm = dx.at(0), dm.at(0)
        before = _stat(ec, b"pool_allocs")
        for scale, offset in R.SCALED_PARAMS:
            what = f"ec_cast_scaled {NAMES[st]} * {scale} + {offset} -> {NAMES[dt]}"
            chk(L.ec_cast_scaled(st, px, None, n, scale, offset, dt, None, out.at(0), ec.stream()))
            _same(out.read(0), R.scaled(st, x, None, scale, offset, dt), x, what)
            chk(L.ec_cast_scaled(st, px, pm, n, scale, offset, dt, C.byref(v), out.at(0), ec.stream()))
            _same(out.read(0), R.scaled(st, x, m, scale, offset, dt, nd), x, what + ", masked")
        scale, offset = R.SCALED_PARAMS[dt % len(R.SCALED_PARAMS)]
        want, want_m = R.scaled(st, x, None, scale, offset, dt), R.scaled(st, x, m, scale, offset, dt, nd)
        for bits in (0, 1, 2, 3):   # the load policy forced: the cells' bit and the mask's; the unmasked kernel has its own arms
            with ec.tuned(cache_force=bits):
                chk(L.ec_cast_scaled(st, px, None, n, scale, offset, dt, None, out.at(0), ec.stream()))
                _same(out.read(0), want, x, f"cache_force {bits} {NAMES[st]} -> {NAMES[dt]}")
                chk(L.ec_cast_scaled(st, px, pm, n, scale, offset, dt, C.byref(v), out.at(0), ec.stream()))
                _same(out.read(0), want_m, x, f"cache_force {bits} masked {NAMES[st]} -> {NAMES[dt]}")
        px1, pm1 = dx.at(1), dm.at(1)
        for uv in (1, 0):
            with ec.tuned(unaligned_vector=uv):
                chk(L.ec_cast_scaled(st, px1, None, n, scale, offset, dt, None, out.at(1), ec.stream()))
                _same(out.read(1), want, x, f"unaligned_vector {uv} {NAMES[st]} -> {NAMES[dt]}")
                chk(L.ec_cast_scaled(st, px1, pm1, n, scale, offset, dt, C.byref(v), out.at(1), ec.stream()))
                _same(out.read(1), want_m, x, f"unaligned_vector {uv} masked {NAMES[st]} -> {NAMES[dt]}")
        assert _stat(ec, b"pool_allocs") == before, "an ec_cast_scaled call allocated"


def test_the_stated_cells(ec):
    """The cells the header and the issue name, through the Python mirror."""
    i64 = ec.CellBuffer.from_vec(np.array([2**53 + 1, -1, 2**63 - 1], np.int64))
    assert i64.cast(ec.UInt64).to_numpy().tolist() == [2**53 + 1, 0, 2**63 - 1]                  # exact in integers, no detour through f64
    assert i64.cast(ec.UInt64, "as").to_numpy().tolist() == [2**53 + 1, 2**64 - 1, 2**63 - 1]
    f = ec.CellBuffer.from_vec(np.array([0.5, 1.5, 2.5, -0.5, -2.5, 0.49999999999999994, np.nan, 2.0**63, -np.inf, 300.0], np.float64))
    assert f.cast(ec.Int8).to_numpy().tolist() == [1, 2, 3, -1, -3, 1, 0, 127, -128, 127]
    assert f.cast(ec.Int8, "as").to_numpy().tolist() == [0, 1, 2, 0, -2, 0, 0, 127, -128, 127]
    assert f.cast(ec.Int64).to_numpy().tolist()[7:9] == [2**63 - 1, -2**63] and f.cast(ec.UInt64).to_numpy().tolist()[7:9] == [2**63, 0]
    tenth = ec.CellBuffer.from_vec(np.array([0.1], np.float64))
    assert tenth.to_scaled(ec.Float64, 10.0, -1.0).to_numpy().tolist() == [0.0]                 # two roundings; a fused evaluation gives 2^-54


def test_python_mirror(ec):
    """CellBuffer.cast / to_scaled, MaskedCellBuffer.cast / to_scaled, one example each."""
    ndvi = ec.CellBuffer.from_vec(np.array([0.12344, -0.5, 0.99996, np.nan, 7.0]))
    assert ndvi.cast(ec.Float32).cell_type() == ec.Float32 and ndvi.cast(ec.Float32).to_numpy()[0] == np.float32(0.12344)
    assert ndvi.to_scaled(ec.Int16, 10000.0, 0.0).to_numpy().tolist() == [1234, -5000, 10000, 0, 32767]
    classes = ec.CellBuffer.from_vec(np.array([0.4, 1.5, 254.5, 255.5, -3.0]))
    assert classes.cast(ec.UInt8).to_numpy().tolist() == [0, 2, 255, 255, 0] and classes.cast(ec.UInt8, mode="as").to_numpy().tolist() == [0, 1, 254, 255, 0]
    assert classes.cast(ec.Float64).to_numpy().tolist() == classes.to_numpy().tolist()          # a pair that fits
    with pytest.raises(ec.EcError):
        classes.cast(ec.UInt8, mode="floor")
    m = ec.MaskedCellBuffer(ndvi, ec.Mask.new([1, 1, 0, 0, 1]))
    c = m.cast(ec.Int8)
    assert c.cell_type() == ec.Int8 and c.buffer().to_numpy().tolist() == [0, -1, 1, 0, 7] and c.mask().to_numpy().tolist() == [1, 1, 0, 0, 1]
    s = m.to_scaled(ec.Int16, 10000.0, 0.0, ec.NoData.new(-9999))
    assert s.cell_type() == ec.Int16 and s.to_numpy().tolist() == [1234, -5000, -9999, -9999, 32767]
    assert m.to_scaled(ec.Int16, 10000.0, 0.0, ec.NoData.none()).to_numpy().tolist() == [1234, -5000, 10000, 0, 32767]
    assert ec.CellBuffer.from_vec(np.array([], np.float64)).cast(ec.UInt8).len() == 0


def test_cpp_mirror_cast_program():
    """erased-cells_amd/host/test_cast_mirror.cpp: cast / to_scaled / sharded cast of the C++ host mirror on hand-checkable cells."""
    host = os.path.join(ROOT, "erased-cells_amd", "host")
    binary = os.path.join(host, "test_cast_mirror")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", host, "-s", "test_cast_mirror"])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
