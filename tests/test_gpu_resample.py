"""ec_window_resample on the GPU: average and bilinear reads of resident rasters against tests/resample_ref.py, the rule of
include/erased_cells.h in Python integers and np.float64 scalars.  The rule gives every cell one right answer, so every comparison
is on the raw bits (bits(), as in test_gpu_window.py).  Integer sources are hashed bytes, as there.  Float sources are hashed bytes
with the exponent folded into 2^-32 .. 2^31, so every sum is finite and the comparison stays strict; ONE test,
test_hashed_float_bits_nan_by_class, runs the raw hashed floats (NaNs, infinities, sums that overflow) over every geometry, and there
two NaNs are equal by class (which payload an addition of two NaNs keeps is the processor's choice, not the rule's).  Nothing expected
comes from the library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import resample_ref as R
from oracle import eco

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
ALGS = {"Bilinear": R.BILINEAR, "Average": R.AVERAGE}
# (w, h -> ow, oh): whole and fractional factors, up and down, one axis copied while the other resamples, single-cell windows and
# outputs, the cap itself
SHAPES = [(40, 8, 20, 4), (33, 7, 11, 7), (35, 7, 14, 3), (31, 5, 47, 8), (17, 3, 1, 1), (8, 8, 8, 3), (2, 2, 5, 5), (1, 1, 3, 2), (64, 2, 1, 2)]
SOURCES = [(61, 9), (97, 6)]
ARMS = [dict(), dict(mall_mb=0)]
ARM_IDS = ["default", "every-load-nt"]


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def raster_cells(ec, ct, cols, rows, seed, raw=False):
    """rows x cols cells of type ct whose BYTES are a hash of their position; a -0.0 among the floats.  Floats keep their hashed sign
    and mantissa and get an exponent of -32 .. 31 from their hashed one (finite, and so are all sums of them) unless `raw`."""
    dt = ec.NP_DTYPES[ct]
    a = eco.fill_u8(cols * rows * dt.itemsize, seed).view(dt).copy()
    if dt.kind == "f":
        if not raw:
            u = a.view(UINT[dt.itemsize])
            mant, ebits = (23, 8) if dt.itemsize == 4 else (52, 11)
            e = (u >> mant) & ((1 << ebits) - 1)
            folded = (e % 64) + ((1 << (ebits - 1)) - 1 - 32)
            keep = ((1 << (8 * dt.itemsize)) - 1) ^ (((1 << ebits) - 1) << mant)
            u[...] = (u & u.dtype.type(keep)) | (folded << mant)
            assert np.isfinite(a).all()
        else:  # f64 bytes hash to a NaN once in 2048 cells: make sure some are there, and infinities of both signs
            a[5::37], a[6::41], a[9::43] = np.nan, np.inf, -np.inf
        if a.size > 3:
            a[3] = dt.type(-0.0)
    return a.reshape(rows, cols)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def same_cells(got, exp, nan_by_class=False):
    """bit for bit; with nan_by_class (the one test over raw hashed floats) two NaNs are equal"""
    got, exp = np.asarray(got).ravel(), np.asarray(exp).ravel()
    assert got.dtype == exp.dtype and got.shape == exp.shape
    same = bits(got) == bits(exp)
    if nan_by_class:
        same |= np.isnan(got) & np.isnan(exp)
    return bool(same.all())


def placements(cols, rows, w, h):
    """the window at (3, 1) and flush against each edge of the raster, where it fits"""
    at = [(3, 1), (0, 1), (cols - w, 1), (3, 0), (3, rows - h), (cols - w, rows - h)]
    return sorted({(min(x, cols - w), min(y, rows - h)) for x, y in at})


def geometries():
    out = []
    for w, h, ow, oh in SHAPES:
        fits = [(c, r) for c, r in SOURCES if w <= c and h <= r]
        assert fits, (w, h)
        for cols, rows in fits:
            for x0, y0 in placements(cols, rows, w, h):
                out.append((cols, rows, x0, y0, w, h, ow, oh))
    return out


GEOMS = geometries()
_expected = {}


def expected(ec, ct, alg, geom, masked, raw=False):
    """the yardstick's answer, computed once per case and shared by the tuning arms"""
    key = (ct, alg, geom, masked, raw)
    if key not in _expected:
        cols, rows, x0, y0, w, h, ow, oh = geom
        a = raster_cells(ec, ct, cols, rows, 0x2E5A + ct, raw)
        m = eco.fill_u8(cols * rows, 0x3A5C + ct, lo=0, hi=99).reshape(rows, cols) < 60 if masked else None
        m = None if m is None else m.astype(np.uint8)
        _expected[key] = (a, m) + R.resample(alg, a, m, x0, y0, w, h, ow, oh)
    return _expected[key]


@pytest.mark.parametrize("arm", ARMS, ids=ARM_IDS)
@pytest.mark.parametrize("name", sorted(ALGS))
@pytest.mark.parametrize("ct", range(10))
def test_every_type_and_geometry(ec, ct, name, arm):
    assert {g[:2] for g in GEOMS} == set(SOURCES) and {g[4:] for g in GEOMS} == set(SHAPES)
    with ec.tuned(**arm):
        bufs = {}
        for geom in GEOMS:
            cols, rows, x0, y0, w, h, ow, oh = geom
            a, _, exp, _ = expected(ec, ct, ALGS[name], geom, False)
            if (cols, rows) not in bufs:
                bufs[(cols, rows)] = ec.CellBuffer.from_vec(a.ravel())
            got = bufs[(cols, rows)].window(cols, (x0, y0), (w, h), (ow, oh), resample=name)
            assert got.cell_type() == ct and got.len() == ow * oh
            assert same_cells(got.to_numpy(), exp), (name, geom)


@pytest.mark.parametrize("arm", ARMS, ids=ARM_IDS)
@pytest.mark.parametrize("name", sorted(ALGS))
@pytest.mark.parametrize("ct", range(10))
def test_masked_every_type_and_geometry(ec, ct, name, arm):
    """60 % of the cells valid: only they carry weight; the mask of the result says where a footprint had none"""
    with ec.tuned(**arm):
        bufs = {}
        for geom in GEOMS:
            cols, rows, x0, y0, w, h, ow, oh = geom
            a, m, exp, em = expected(ec, ct, ALGS[name], geom, True)
            if (cols, rows) not in bufs:
                bufs[(cols, rows)] = ec.MaskedCellBuffer(ec.CellBuffer.from_vec(a.ravel()), ec.Mask.new(m.ravel()))
            got = bufs[(cols, rows)].window(cols, (x0, y0), (w, h), (ow, oh), resample=name)
            assert np.array_equal(got.mask().to_numpy(), em.ravel()), (name, geom)
            assert same_cells(got.buffer().to_numpy(), exp), (name, geom)
            assert got.counts() == (int(em.sum()), int(em.size - em.sum()))


@pytest.mark.parametrize("name", sorted(ALGS))
@pytest.mark.parametrize("ct", (8, 9))
def test_hashed_float_bits_nan_by_class(ec, ct, name):
    """the one test with NaNs: f32 / f64 cells of raw hashed bytes — NaNs of every payload, infinities, denormals, sums that overflow —
    over every geometry, plain and masked; bit for bit except that a NaN matches a NaN"""
    bufs, nans = {}, 0
    for geom in GEOMS:
        cols, rows, x0, y0, w, h, ow, oh = geom
        a, _, exp, _ = expected(ec, ct, ALGS[name], geom, False, raw=True)
        _, m, mexp, em = expected(ec, ct, ALGS[name], geom, True, raw=True)
        if (cols, rows) not in bufs:
            bufs[(cols, rows)] = (ec.CellBuffer.from_vec(a.ravel()), ec.MaskedCellBuffer(ec.CellBuffer.from_vec(a.ravel()), ec.Mask.new(m.ravel())))
        buf, mb = bufs[(cols, rows)]
        assert same_cells(buf.window(cols, (x0, y0), (w, h), (ow, oh), resample=name).to_numpy(), exp, nan_by_class=True), (name, geom)
        got = mb.window(cols, (x0, y0), (w, h), (ow, oh), resample=name)
        assert np.array_equal(got.mask().to_numpy(), em.ravel()), (name, geom)
        assert same_cells(got.buffer().to_numpy(), mexp, nan_by_class=True), (name, geom)
        nans += int(np.isnan(exp).sum())
    assert nans > 0  # the sources do hold NaNs, and they reach the results


def _hashed(n, seed, k):
    return np.unique((eco.fill_u8(8 * k, seed).view(np.uint64) % np.uint64(n)).astype(np.int64))


# one output per cell width with several workgroups, both fronts and a last tile that is not full (a tile: 1024 slots of 16 bytes)
LARGE = [(0, "Average", 600, 64, 300, 56), (5, "Bilinear", 300, 40, 421, 47), (8, "Average", 250, 60, 111, 47), (7, "Bilinear", 90, 70, 131, 53)]


@pytest.mark.parametrize("ct,name,w,h,ow,oh", LARGE)
def test_more_than_one_tile(ec, ct, name, w, h, ow, oh):
    """checked on a sample: the first and last slot of every tile, the last cells, 2000 hashed cells — both values and mask"""
    cols, rows, x0, y0 = w + 5, h + 3, 2, 1
    a = raster_cells(ec, ct, cols, rows, 0xB16 + ct)
    m = (eco.fill_u8(cols * rows, 0xB17 + ct, lo=0, hi=99).reshape(rows, cols) < 60).astype(np.uint8)
    cpl = 16 // a.dtype.itemsize
    n, tile = ow * oh, 1024 * cpl
    assert n > tile and n % tile != 0
    idx = set(_hashed(n, 0x5A3 + ct, 2000).tolist()) | set(range(n - cpl - 3, n))
    for t0 in range(0, n, tile):
        idx |= set(range(t0, min(n, t0 + cpl))) | set(range(min(n, t0 + tile) - cpl, min(n, t0 + tile)))
    idx = np.array(sorted(idx))
    plain = ec.CellBuffer.from_vec(a.ravel()).window(cols, (x0, y0), (w, h), (ow, oh), resample=name).to_numpy()
    masked = ec.MaskedCellBuffer(ec.CellBuffer.from_vec(a.ravel()), ec.Mask.new(m.ravel())).window(cols, (x0, y0), (w, h), (ow, oh), resample=name)
    mv, mm = masked.buffer().to_numpy(), masked.mask().to_numpy()
    exp = [R.cell(ALGS[name], a, None, x0, y0, w, h, ow, oh, k // ow, k % ow)[0] for k in idx]
    mexp = [R.cell(ALGS[name], a, m, x0, y0, w, h, ow, oh, k // ow, k % ow) for k in idx]
    assert same_cells(plain[idx], np.array(exp, dtype=a.dtype))
    assert same_cells(mv[idx], np.array([v for v, _ in mexp], dtype=a.dtype))
    assert np.array_equal(mm[idx], np.array([ok for _, ok in mexp], dtype=np.uint8))


@pytest.mark.parametrize("name", sorted(ALGS))
def test_cells_outside_the_window_do_not_matter(ec, name):
    """every raster cell OUTSIDE the window overwritten with a sentinel: bilinear taps clamp to the window, not to the raster"""
    for ct in (ec.UInt8, ec.Int32, ec.Float64):
        cols, rows, x0, y0, w, h = 61, 9, 3, 1, 31, 5
        a = raster_cells(ec, ct, cols, rows, 0xED6E + ct)
        b = np.full_like(a, 77)
        b[y0:y0 + h, x0:x0 + w] = a[y0:y0 + h, x0:x0 + w]
        for ow, oh in ((47, 8), (14, 3), (62, 10), (31, 9)):
            one = ec.CellBuffer.from_vec(a.ravel()).window(cols, (x0, y0), (w, h), (ow, oh), resample=name).to_numpy()
            two = ec.CellBuffer.from_vec(b.ravel()).window(cols, (x0, y0), (w, h), (ow, oh), resample=name).to_numpy()
            assert same_cells(one, two), (ct, ow, oh)
            assert same_cells(one, R.resample(ALGS[name], b, None, x0, y0, w, h, ow, oh)[0])


def test_integer_rounding_and_saturation(ec):
    # i8 cells that average to exactly -0.5 and +0.5: half away from zero
    a = np.array([[-1, 0, 1, 0], [0, -1, 0, 1]], dtype=np.int8)
    got = ec.CellBuffer.from_vec(a.ravel()).window(4, (0, 0), (4, 2), (2, 1), resample="Average").to_numpy()
    assert got.tolist() == [-1, 1]
    got = ec.CellBuffer.from_vec(np.array([-1, 0, 0, 1], dtype=np.int8)).window(4, (0, 0), (4, 1), (2, 1), resample="Average").to_numpy()
    assert got.tolist() == [-1, 1]
    # 64-bit cells at the ends of their range: double(cell) rounds to 2^64 and to -2^63, and the result saturates
    for dt, v in ((np.uint64, 2 ** 64 - 1), (np.int64, -2 ** 63), (np.int64, 2 ** 63 - 1), (np.uint64, 0)):
        a = np.full((6, 10), v, dtype=dt)
        for name, size in (("Average", (5, 2)), ("Average", (3, 4)), ("Bilinear", (15, 4)), ("Bilinear", (4, 7))):
            got = ec.CellBuffer.from_vec(a.ravel()).window(10, (0, 0), (10, 6), size, resample=name).to_numpy()
            assert got.dtype == dt and (got == dt(v)).all(), (dt, v, name, size)
            assert same_cells(got, R.resample(ALGS[name], a, None, 0, 0, 10, 6, *size)[0])


def test_masked_footprints(ec):
    cols, rows = 12, 8
    a = np.arange(cols * rows, dtype=np.float64).reshape(rows, cols) * 1.25 - 7.0
    m = np.ones((rows, cols), dtype=np.uint8)
    m[0:4, 0:4] = 0          # a footprint with no valid cell
    m[4:8, 4:8] = 0
    m[6, 5] = 1              # ... and one with a single valid cell
    a[0, 1] = a[5, 5] = np.nan  # invalid NaNs: under a masked-out tap they leave no trace
    mb = ec.MaskedCellBuffer(ec.CellBuffer.from_vec(a.ravel()), ec.Mask.new(m.ravel()))
    got = mb.window(cols, (0, 0), (12, 8), (3, 2), resample="Average")
    v, ok = got.buffer().to_numpy().reshape(2, 3), got.mask().to_numpy().reshape(2, 3)
    assert ok.tolist() == [[0, 1, 1], [1, 1, 1]]
    assert bits(v[0, 0:1])[0] == 0 and bits(v[1, 1:2])[0] == bits(a[6, 5:6])[0]
    exp, em = R.resample(R.AVERAGE, a, m, 0, 0, 12, 8, 3, 2)
    assert same_cells(v, exp) and np.array_equal(ok, em) and not np.isnan(v).any()
    # bilinear 3 -> 1 along a row: t = 3 + 1 = 4 = 2 * 2 + 0, so the second tap (cell 2) has weight 0 and is never read
    b = np.array([[1.0, 5.0, np.nan]], dtype=np.float64)
    assert R.bilinear_taps(0, 3, 1) == [(1, 2)]
    got = ec.CellBuffer.from_vec(b.ravel()).window(3, (0, 0), (3, 1), (1, 1), resample="Bilinear").to_numpy()
    assert bits(got)[0] == bits(np.array([5.0]))[0]   # unmasked: the NaN sits under the zero-weight tap
    bm = np.array([[1, 1, 0]], dtype=np.uint8)
    got = ec.MaskedCellBuffer(ec.CellBuffer.from_vec(b.ravel()), ec.Mask.new(bm.ravel())).window(3, (0, 0), (3, 1), (2, 1), resample="Bilinear")
    exp, em = R.resample(R.BILINEAR, b, bm, 0, 0, 3, 1, 2, 1)
    assert not np.isnan(exp).any() and same_cells(got.buffer().to_numpy(), exp) and np.array_equal(got.mask().to_numpy(), em.ravel())


def test_nearest_and_none_are_window_itself(ec):
    for ct in (ec.UInt8, ec.Float32, ec.Int64):
        a = raster_cells(ec, ct, 97, 10, 0x11E + ct)
        m = eco.fill_u8(97 * 10, 0x22E, lo=0, hi=1)
        buf = ec.CellBuffer.from_vec(a.ravel())
        mb = ec.MaskedCellBuffer(ec.CellBuffer.from_vec(a.ravel()), ec.Mask.new(m))
        for w, h, ow, oh in SHAPES[:6] + [(40, 5, 40, 5)]:
            base = buf.window(97, (3, 1), (w, h), (ow, oh))
            mbase = mb.window(97, (3, 1), (w, h), (ow, oh))
            for name in (None, "NearestNeighbour"):
                assert np.array_equal(bits(buf.window(97, (3, 1), (w, h), (ow, oh), resample=name).to_numpy()), bits(base.to_numpy()))
                got = mb.window(97, (3, 1), (w, h), (ow, oh), resample=name)
                assert np.array_equal(bits(got.buffer().to_numpy()), bits(mbase.buffer().to_numpy()))
                assert np.array_equal(got.mask().to_numpy(), mbase.mask().to_numpy())
            # the C entry point with EC_RESAMPLE_NEAREST, and any algorithm at equal size: the copy
            out = ec.CellBuffer.empty(ow * oh, ct)
            ec._ffi.check(ec.lib().ec_window_resample(R.NEAREST, ct, buf.mem.ptr, None, 97, 10, 3, 1, w, h, ow, oh, out.mem.ptr, None, ec.stream()))
            assert np.array_equal(bits(out.to_numpy()), bits(base.to_numpy()))
        for name in ALGS:
            assert np.array_equal(bits(buf.window(97, (3, 1), (40, 5), (40, 5), resample=name).to_numpy()), bits(a[1:6, 3:43]).ravel())


def test_python_forms_agree_with_the_c_abi(ec):
    L = ec.lib()
    cols, rows, x0, y0, w, h, ow, oh = 97, 6, 5, 1, 64, 5, 23, 3
    a = raster_cells(ec, ec.UInt16, cols, rows, 0xABE)
    m = eco.fill_u8(cols * rows, 0xABF, lo=0, hi=1)
    buf, mask = ec.CellBuffer.from_vec(a.ravel()), ec.Mask.new(m)
    for name, alg in ALGS.items():
        out, om = ec.CellBuffer.empty(ow * oh, ec.UInt16), ec.Mask.empty(ow * oh)
        ec._ffi.check(L.ec_window_resample(alg, ec.UInt16, buf.mem.ptr, None, cols, rows, x0, y0, w, h, ow, oh, out.mem.ptr, None, ec.stream()))
        assert np.array_equal(out.to_numpy(), buf.window(cols, (x0, y0), (w, h), (ow, oh), resample=name).to_numpy())
        ec._ffi.check(L.ec_window_resample(alg, ec.UInt16, buf.mem.ptr, mask.mem.ptr, cols, rows, x0, y0, w, h, ow, oh, out.mem.ptr, om.mem.ptr, ec.stream()))
        got = ec.MaskedCellBuffer(buf, mask).window(cols, (x0, y0), (w, h), (ow, oh), resample=name)
        assert np.array_equal(out.to_numpy(), got.buffer().to_numpy()) and np.array_equal(om.to_numpy(), got.mask().to_numpy())
        assert np.array_equal(out.to_numpy(), R.resample(alg, a, m.reshape(rows, cols), x0, y0, w, h, ow, oh)[0].ravel())
    with pytest.raises(ec.EcError, match="EC_WINDOW_MAX_REDUCTION"):
        buf.window(cols, (0, 0), (65, 1), (1, 1), resample="Average")
    with pytest.raises(ec.EcError, match="Lanczos"):
        buf.window(cols, (0, 0), (4, 4), (2, 2), resample="Lanczos")


def test_cpp_mirror_resample_program():
    """erased-cells_amd/host/test_resample_mirror.cpp: CellBuffer::window / MaskedCellBuffer::window with a ResampleAlg against the C ABI
    and against hand-computed cells"""
    host = os.path.join(ROOT, "erased-cells_amd", "host")
    binary = os.path.join(host, "test_resample_mirror")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", host, "-s", "test_resample_mirror"])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout and "host-only" not in r.stdout


def test_captured_in_a_graph_and_replayed_without_allocation(ec):
    import torch
    L = ec.lib()
    side = torch.cuda.Stream()
    ec._ffi.check(L.ec_prepare_stream(side.cuda_stream))
    cols, rows, x0, y0, w, h = 301, 90, 17, 5, 250, 80
    sizes = {"Average": (100, 33), "Bilinear": (333, 97)}
    a = raster_cells(ec, ec.UInt16, cols, rows, 0x6A9)
    m = (eco.fill_u8(cols * rows, 0x6AA, lo=0, hi=99) < 60).astype(np.uint8).reshape(rows, cols)
    t_src = torch.from_numpy(a.view(np.int16).copy()).cuda()
    t_mask = torch.from_numpy(m.copy()).cuda()
    t_out = {k: torch.zeros(s[0] * s[1], dtype=torch.int16, device="cuda") for k, s in sizes.items()}
    t_mout = {k: torch.zeros(s[0] * s[1], dtype=torch.int16, device="cuda") for k, s in sizes.items()}
    t_om = {k: torch.zeros(s[0] * s[1], dtype=torch.uint8, device="cuda") for k, s in sizes.items()}
    torch.cuda.synchronize()
    before, after = C.c_int64(), C.c_int64()
    ec._ffi.check(L.ec_stat_get(b"pool_allocs", C.byref(before)))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        for k, (ow, oh) in sizes.items():
            ec._ffi.check(L.ec_window_resample(ALGS[k], ec.UInt16, t_src.data_ptr(), None, cols, rows, x0, y0, w, h, ow, oh, t_out[k].data_ptr(), None, s))
            ec._ffi.check(L.ec_window_resample(ALGS[k], ec.UInt16, t_src.data_ptr(), t_mask.data_ptr(), cols, rows, x0, y0, w, h, ow, oh,
                                               t_mout[k].data_ptr(), t_om[k].data_ptr(), s))
    for trial in range(3):
        if trial:
            a = raster_cells(ec, ec.UInt16, cols, rows, 0x6A9 + trial)
            t_src.copy_(torch.from_numpy(a.view(np.int16).copy()))
        g.replay()
        torch.cuda.synchronize()
        for k, (ow, oh) in sizes.items():
            idx = _hashed(ow * oh, 0x77 + trial, 150)
            got, gm, gom = (t.cpu().numpy() for t in (t_out[k], t_mout[k], t_om[k]))
            exp = [R.cell(ALGS[k], a, None, x0, y0, w, h, ow, oh, i // ow, i % ow)[0] for i in idx]
            mexp = [R.cell(ALGS[k], a, m, x0, y0, w, h, ow, oh, i // ow, i % ow) for i in idx]
            assert np.array_equal(got.view(np.uint16)[idx], np.array(exp, dtype=np.uint16)), (k, trial)
            assert np.array_equal(gm.view(np.uint16)[idx], np.array([v for v, _ in mexp], dtype=np.uint16)), (k, trial)
            assert np.array_equal(gom[idx], np.array([ok for _, ok in mexp], dtype=np.uint8)), (k, trial)
    ec._ffi.check(L.ec_stat_get(b"pool_allocs", C.byref(after)))
    assert after.value == before.value
