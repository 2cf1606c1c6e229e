"""ec_compare / ec_compare_scalar / ec_select / ec_masked_select on the GPU against tests/compare_ref.py — bit for bit, no
exception: the order is total, every cell has one right answer.

Per lhs type (one test each, not one per pair): all 10 rhs types x 6 relations on the special-values cross product plus 4,099
random cells with ties planted; all 10 scalar types; the masked forms with one mask, the other, both (at a length that leaves a
ragged tail at every CPL); both settings of `unaligned_vector` (at an odd cell offset, where the knob decides between the vector
and the cell-wise kernel); the load policy forced to all-`nt`, to each split, and split by a budget (`mall_mb`).  Then the
identities that tie the family to what is already trusted, the Python mirror, the shard group, the C++ mirror and one known answer
from the fixtures.  tests/test_compare_faults.py shows (without a GPU) that these inputs notice a wrong kernel.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import compare_ref as R
from oracle import eco
from tiff_util import read_tiff
from vectors import rand_cells

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT = R.NT


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


@pytest.fixture(scope="module")
def inputs():
    """(l, r) per type pair, computed once and left unchanged."""
    memo = {}

    def get(lt, rt):
        if (lt, rt) not in memo:
            memo[lt, rt] = R.gpu_inputs(lt, rt)
        return memo[lt, rt]
    return get


def _stat(ec, key):
    v = C.c_int64(0)
    ec._ffi.check(ec.lib().ec_stat_get(key, C.byref(v)))
    return v.value


class Dev:
    """An array on the device one cell behind an allocation's start as well as at it: `at(0)` is 256-byte aligned, `at(1)` is not
    16-byte aligned for any cell width."""

    def __init__(self, ec, a):
        self.a = np.ascontiguousarray(a)
        sz = self.a.dtype.itemsize
        self.mem = ec.DeviceMem((self.a.size + 1) * sz)
        self.sz = sz
        self.ec = ec
        self._at = None

    def at(self, off):
        if self._at != off:
            self.ec._ffi.check(self.ec.lib().ec_upload(self.mem.ptr + off * self.sz, self.a.ctypes.data_as(C.c_void_p), self.a.nbytes, self.ec.stream()))
            self._at = off
        return self.mem.ptr + off * self.sz


def _out(ec, n):
    return ec.DeviceMem(n + 16)


def _read(ec, mem, off, n):
    out = np.empty(n, np.uint8)
    ec._ffi.check(ec.lib().ec_download(out.ctypes.data_as(C.c_void_p), mem.ptr + off, n, ec.stream()))
    return out


def _same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} cells differ, first at {int(bad[0])} of {got.size}: got {int(got[bad[0]])}"


@pytest.mark.parametrize("lt", range(NT), ids=R.NAMES)
def test_compare_all_rhs_types(ec, inputs, lt):
    L, chk, E = ec.lib(), ec._ffi.check, ec._ffi
    before = None
    for rt in range(NT):
        l, r = inputs(lt, rt)
        n = l.size
        dl, dr, out = Dev(ec, l), Dev(ec, r), _out(ec, n)
        nt = R.tail_len(n)
        lm, rm = R.gpu_masks(nt)
        dlm, drm = Dev(ec, lm), Dev(ec, rm)
        pl, pr, plm, prm = dl.at(0), dr.at(0), dlm.at(0), drm.at(0)
        before = _stat(ec, b"pool_allocs")
        got = {}
        for rel in R.RELS:
            chk(L.ec_compare(rel, lt, pl, None, rt, pr, None, n, out.ptr, ec.stream()))
            got[rel] = _read(ec, out, 0, n)
            _same(got[rel], R.relation(rel, lt, l, rt, r), f"ec_compare {R.NAMES[lt]} rel {rel} {R.NAMES[rt]}")
        assert np.array_equal(got[R.LT], 1 - got[R.GE]) and np.array_equal(got[R.GT], 1 - got[R.LE]) and np.array_equal(got[R.EQ], 1 - got[R.NE])
        # the masked forms: one mask, the other, both — LT and GE, at a length with a ragged tail at every CPL
        for rel in (R.LT, R.GE):
            for a, b, ha, hb in ((plm, None, lm, None), (None, prm, None, rm), (plm, prm, lm, rm)):
                chk(L.ec_compare(rel, lt, pl, a, rt, pr, b, nt, out.ptr, ec.stream()))
                _same(_read(ec, out, 0, nt), R.masked_relation(rel, lt, l[:nt], ha, rt, r[:nt], hb),
                      f"masked ec_compare {R.NAMES[lt]} rel {rel} {R.NAMES[rt]} masks {a is not None}/{b is not None}")
        # load policy forced: all nt, each split, both default
        for bits in (0, 1, 2, 3):
            with ec.tuned(cache_force=bits):
                chk(L.ec_compare(R.LE, lt, pl, plm, rt, pr, prm, nt, out.ptr, ec.stream()))
                _same(_read(ec, out, 0, nt), R.masked_relation(R.LE, lt, l[:nt], lm, rt, r[:nt], rm), f"cache_force {bits} {R.NAMES[lt]} {R.NAMES[rt]}")
        # an odd cell offset on every pointer: the vector kernel (unaligned_vector = 1) and the cell-wise kernel (0)
        pl1, pr1, plm1, prm1 = dl.at(1), dr.at(1), dlm.at(1), drm.at(1)
        for uv in (1, 0):
            with ec.tuned(unaligned_vector=uv):
                chk(L.ec_compare(R.GT, lt, pl1, None, rt, pr1, None, n, out.ptr + 1, ec.stream()))
                _same(_read(ec, out, 1, n), got[R.GT], f"unaligned_vector {uv} {R.NAMES[lt]} {R.NAMES[rt]}")
                chk(L.ec_compare(R.NE, lt, pl1, plm1, rt, pr1, prm1, nt, out.ptr + 3, ec.stream()))
                _same(_read(ec, out, 3, nt), R.masked_relation(R.NE, lt, l[:nt], lm, rt, r[:nt], rm), f"masked, unaligned_vector {uv}")
        assert _stat(ec, b"pool_allocs") == before, "a compare call allocated"
    # split by a budget: 125,000 cells against f64 under a 1 MiB budget admit the smaller operand and stream the other
    n = 125000
    l, r = rand_cells(lt, n, 9500, specials=False), rand_cells(eco.F64, n, 9501, specials=False)
    sp = R.specials(lt)                       # quiet NaNs only: what a widening does to a signalling one is unpinned
    l[::7] = sp[np.arange(l[::7].size) % sp.size]
    with np.errstate(all="ignore"):
        r[::5] = l[::5].astype(np.float64)    # ties
    dl, dr, out = Dev(ec, l), Dev(ec, r), _out(ec, n)
    with ec.tuned(mall_mb=1):
        chk(L.ec_compare(R.LE, lt, dl.at(0), None, eco.F64, dr.at(0), None, n, out.ptr, ec.stream()))
    _same(_read(ec, out, 0, n), R.relation(R.LE, lt, l, eco.F64, r), f"mall_mb 1 {R.NAMES[lt]} <= Float64")


@pytest.mark.parametrize("lt", range(NT), ids=R.NAMES)
def test_compare_scalar_all_scalar_types(ec, inputs, lt):
    L, chk = ec.lib(), ec._ffi.check
    # cells with signalling NaNs meet scalars of their own type only: what a widening does to them is unpinned
    sets = {}
    for same in (True, False):
        l = inputs(lt, lt if same else (R.U16 if lt == R.U8 else R.U8))[0]
        n = R.tail_len(l.size)
        sets[same] = (l[:n], n, R.gpu_masks(n)[0], Dev(ec, l[:n]), Dev(ec, R.gpu_masks(n)[0]), _out(ec, n))
    before = _stat(ec, b"pool_allocs")
    for st in range(NT):
        l, n, lm, dl, dlm, out = sets[st == lt]
        table = R.specials(st, signalling=(st == lt and R.NP[st].kind == "f"))
        with np.errstate(all="ignore"):
            tie = l[(7 * st) % n:][:1].astype(R.NP[st])   # a cell of the buffer as the scalar's type: a tie where it converts exactly
        for k, s in enumerate(list(table) + list(tie)):
            rel = R.RELS[(k + st) % 6]
            v = ec.CellValue(st, s).to_ec()
            for off, uv in ((0, 1), (1, 1), (1, 0)):
                with ec.tuned(unaligned_vector=uv):
                    masked = (k + off) % 2 == 1
                    chk(L.ec_compare_scalar(rel, lt, dl.at(off), dlm.at(off) if masked else None, n, C.byref(v), out.ptr + off, ec.stream()))
                    want = R.relation(rel, lt, l, st, s)
                    _same(_read(ec, out, off, n), want & lm if masked else want,
                          f"ec_compare_scalar {R.NAMES[lt]} rel {rel} {R.NAMES[st]}({s!r}) offset {off} unaligned_vector {uv} masked {masked}")
    assert _stat(ec, b"pool_allocs") == before, "a compare_scalar call allocated"


@pytest.mark.parametrize("ct", range(NT), ids=R.NAMES)
def test_identities(ec, inputs, ct):
    """compare_scalar(NE, x, nd) == ec_mask_from_nodata(x, nd); EQ(x, x) is all ones, NaNs included; ec_select with sel all true /
    all false copies a / b; ec_select equals ec_mask_select when b is a filled buffer; ec_masked_select against numpy."""
    L, chk = ec.lib(), ec._ffi.check
    x, _ = inputs(ct, ct)
    n = x.size
    dx, out, out2 = Dev(ec, x), _out(ec, n), _out(ec, n)
    for nd in (x[3], x[n // 2], x[n - 1]):
        v = ec.CellValue(ct, nd).to_ec()
        chk(L.ec_compare_scalar(R.NE, ct, dx.at(0), None, n, C.byref(v), out.ptr, ec.stream()))
        chk(L.ec_mask_from_nodata(ct, dx.at(0), n, C.byref(v), out2.ptr, ec.stream()))
        _same(_read(ec, out, 0, n), _read(ec, out2, 0, n), f"NE against ec_mask_from_nodata {R.NAMES[ct]} {nd!r}")
    chk(L.ec_compare(R.EQ, ct, dx.at(0), None, ct, dx.at(0), None, n, out.ptr, ec.stream()))
    assert _read(ec, out, 0, n).all(), "EQ(x, x)"
    # select
    sel, a, am, b, bm = R.select_inputs(ct)
    m = sel.size
    sz = a.dtype.itemsize
    da, db, dsel, dam, dbm = Dev(ec, a), Dev(ec, b), Dev(ec, sel), Dev(ec, am), Dev(ec, bm)
    ones, zeros = Dev(ec, np.ones(m, np.uint8)), Dev(ec, np.zeros(m, np.uint8))
    o, om = ec.DeviceMem(m * sz + 16), _out(ec, m)
    before = _stat(ec, b"pool_allocs")

    def cells(mem, off_cells=0):
        return _read(ec, mem, off_cells * sz, m * sz)

    for off, uv in ((0, 1), (1, 1), (1, 0)):
        with ec.tuned(unaligned_vector=uv):
            pa, pb, ps = da.at(off), db.at(off), dsel.at(off)
            chk(L.ec_select(ct, pa, pb, ps, m, o.ptr + off * sz, ec.stream()))
            _same(cells(o, off), R.select(sel, a, b).view(np.uint8), f"ec_select {R.NAMES[ct]} offset {off} unaligned_vector {uv}")
            chk(L.ec_select(ct, pa, pb, ones.at(off), m, o.ptr + off * sz, ec.stream()))
            _same(cells(o, off), a.view(np.uint8), "ec_select, sel all true: a copy of a")
            chk(L.ec_select(ct, pa, pb, zeros.at(off), m, o.ptr + off * sz, ec.stream()))
            _same(cells(o, off), b.view(np.uint8), "ec_select, sel all false: a copy of b")
            chk(L.ec_masked_select(ct, pa, dam.at(off), pb, dbm.at(off), ps, m, o.ptr + off * sz, om.ptr + off, ec.stream()))
            want, want_m = R.masked_select(sel, a, am, b, bm)
            _same(cells(o, off), want.view(np.uint8), f"ec_masked_select values {R.NAMES[ct]} offset {off} unaligned_vector {uv}")
            _same(_read(ec, om, off, m), want_m, f"ec_masked_select mask {R.NAMES[ct]} offset {off} unaligned_vector {uv}")
    assert _stat(ec, b"pool_allocs") == before, "a select call allocated"
    # against ec_mask_select: b a buffer filled with the nodata value
    nd = ec.CellValue(ct, b[5])
    filled = ec.CellBuffer.fill(m, nd)
    v = nd.to_ec()
    o2 = ec.DeviceMem(m * sz)
    chk(L.ec_select(ct, da.at(0), filled.mem.ptr, dsel.at(0), m, o.ptr, ec.stream()))
    chk(L.ec_mask_select(ct, da.at(0), dsel.at(0), m, C.byref(v), o2.ptr, ec.stream()))
    _same(cells(o), cells(o2), f"ec_select against ec_mask_select {R.NAMES[ct]}")


def test_python_mirror(ec):
    """CellBuffer.compare and its shorthands, MaskedCellBuffer.compare, select with operands of different types, or_else."""
    a = np.array([0.1, 0.3, 0.31, -0.0, np.nan])
    ndvi = ec.CellBuffer.from_vec(a)
    assert ndvi.compare(">", 0.3).to_numpy().tolist() == [0, 0, 1, 0, 1]           # a positive NaN is above +inf
    assert ndvi.lt(0.0).to_numpy().tolist() == [0, 0, 0, 1, 0]                     # -0.0 < +0.0
    qa = ec.CellBuffer.from_vec(np.array([4, 5, 4, 0], np.uint8))
    assert qa.eq(4).to_numpy().tolist() == [1, 0, 1, 0] and qa.compare(ec._ffi.EC_CMP_NE, 4).to_numpy().tolist() == [0, 1, 0, 1]
    nir, red = ec.CellBuffer.from_vec(np.array([10, 20, 30], np.uint16)), ec.CellBuffer.from_vec(np.array([11, 20, -1, 7], np.int16))
    assert nir.lt(red).to_numpy().tolist() == [1, 0, 0] and nir.ge(red).to_numpy().tolist() == [0, 1, 1]
    assert nir.le(red).to_numpy().tolist() == [1, 1, 0] and nir.gt(red).to_numpy().tolist() == [0, 0, 1] and nir.ne(red).to_numpy().tolist() == [1, 0, 1]
    assert not (nir == red) and (nir == nir)                                        # the operators stay the whole-buffer Ord
    with pytest.raises(ec.EcError):
        nir.compare("=>", red)
    ma = ec.MaskedCellBuffer(ec.CellBuffer.from_vec(np.array([1, 2, 3, 4], np.float32)), ec.Mask.new([1, 0, 1, 1]))
    mb = ec.MaskedCellBuffer(ec.CellBuffer.from_vec(np.array([0, 0, 9, 0], np.uint8)), ec.Mask.new([1, 1, 1, 0]))
    assert ma.gt(mb).to_numpy().tolist() == [1, 0, 0, 0] and ma.ne(np.float32(1.0)).to_numpy().tolist() == [0, 0, 1, 1]
    assert ma.compare(">", mb.buffer()).to_numpy().tolist() == [1, 0, 0, 1]
    f = ma.or_else(mb)
    assert f.cell_type() == ec.Float32 and f.buffer().to_numpy().tolist() == [1.0, 0.0, 3.0, 4.0] and f.mask().to_numpy().tolist() == [1, 1, 1, 1]
    g = mb.or_else(ma)
    assert g.cell_type() == ec.Float32 and g.buffer().to_numpy().tolist() == [0.0, 0.0, 9.0, 4.0] and g.mask().to_numpy().tolist() == [1, 1, 1, 1]
    s = ec.select(ec.Mask.new([1, 0, 0, 1]), ma.buffer(), mb.buffer())
    assert s.cell_type() == ec.Float32 and s.to_numpy().tolist() == [1.0, 0.0, 9.0, 4.0]
    assert ec.CellBuffer.from_vec(np.array([], np.uint8)).gt(3).len() == 0


@pytest.mark.parametrize("shards", [1, 3])
def test_shard_group_compare(ec, inputs, shards):
    """A group of 1 and of 3 shards of one device against the whole-raster call."""
    from erased_cells_hip.sharded import ShardGroup
    rows, cols = 21, 11
    n = rows * cols
    l, r = (x[-n:] for x in inputs(eco.U16, eco.F32))
    lm, rm = R.gpu_masks(n)
    whole = ec.MaskedCellBuffer(ec.CellBuffer.from_vec(l), ec.Mask.new(lm)).compare("<=", ec.MaskedCellBuffer(ec.CellBuffer.from_vec(r), ec.Mask.new(rm)))
    whole_s = ec.CellBuffer.from_vec(l).gt(np.float32(30000.5)).to_numpy()
    assert np.array_equal(whole.to_numpy(), R.masked_relation(R.LE, eco.U16, l, lm, eco.F32, r, rm))
    with ShardGroup([0] * shards, host_combine=True) as g:
        sl, sr = g.scatter(l, rows, cols), g.scatter(r, rows, cols)
        slm, srm = g.scatter(lm, rows, cols), g.scatter(rm, rows, cols)
        out = g.compare("<=", sl, sr, lmask=slm, rmask=srm)
        out_s = g.compare(">", sl, np.float32(30000.5))
        assert np.array_equal(g.gather(out), whole.to_numpy())
        assert np.array_equal(g.gather(out_s), whole_s)
        with pytest.raises(ec.EcError):
            g.compare(7, sl, sr)
        for b in (sl, sr, slm, srm, out, out_s):
            b.free()


def test_cpp_mirror_compare_program():
    """erased-cells_amd/host/test_compare_mirror.cpp: compare / select / or_else / sharded compare of the C++ host mirror on
    hand-checkable cells."""
    host = os.path.join(ROOT, "erased-cells_amd", "host")
    binary = os.path.join(host, "test_compare_mirror")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", host, "-s", "test_compare_mirror"])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout


def test_elkton_ndvi_above_zero(ec, golden_dir):
    """One known answer from the fixtures: the count of cells with NDVI > 0 on the Landsat bands, against numpy on the oracle's NDVI."""
    b5, _ = read_tiff(os.path.join(golden_dir, "L8-Elkton-VA-B5.tiff"))
    b4, _ = read_tiff(os.path.join(golden_dir, "L8-Elkton-VA-B4.tiff"))
    nir, red = b5.ravel(), b4.ravel()
    ndvi = eco.f_binop(eco.DIV, eco.f_binop(eco.SUB, nir, red), eco.f_binop(eco.ADD, nir, red))
    want = R.relation(R.GT, eco.F64, ndvi, eco.F64, 0.0)
    dn, dr = ec.CellBuffer.from_vec(nir), ec.CellBuffer.from_vec(red)
    mask = ((dn - dr) / (dn + dr)).gt(0.0)
    assert np.array_equal(mask.to_numpy(), want)
    assert mask.counts() == (int(want.sum()), int(want.size - want.sum())) and 0 < int(want.sum()) < want.size
