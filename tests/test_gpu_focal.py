"""ec_focal and ec_focal_convolve on the GPU against tests/focal_ref.py, the rule of include/erased_cells.h in numpy.  The rule gives
every cell one right answer, so every comparison is on the raw bits; ONE test, test_raw_hashed_floats_nan_by_class, runs raw hashed
floats with NaNs and infinities, and there two NaNs are equal by class for sum, mean and convolution only (which payload an addition
of two NaNs keeps is the processor's choice, not the rule's) — min and max copy bits and stay strict.  Inputs and shapes come from
tests/focal_cases.py; tests/test_focal_faults.py shows that they expose the mistakes a tiled kernel can make.  Nothing expected comes
from the library."""
import ctypes as C

import numpy as np
import pytest

import focal_cases as K
import focal_ref as R

pytestmark = pytest.mark.gpu

ARMS = [dict(), dict(mall_mb=0)]
ARM_IDS = ["default", "every-load-nt"]
WHOLE, NORMALIZE = 1, 2
# (what, flags): the four operations, two of them again over whole footprints only, and the convolution with and without each flag
FOCAL_CALLS = [(R.SUM, 0), (R.MEAN, 0), (R.MIN, 0), (R.MAX, 0), (R.SUM, WHOLE), (R.MAX, WHOLE)]
CONV_FLAGS = [0, NORMALIZE, WHOLE, WHOLE | NORMALIZE]


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(K.UINT[a.dtype.itemsize])


def same_cells(got, exp, nan_by_class=False):
    got, exp = np.asarray(got).ravel(), np.asarray(exp).ravel()
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    same = bits(got) == bits(exp)
    if nan_by_class:
        same |= np.isnan(got) & np.isnan(exp)
    return bool(same.all())


_sources, _expected = {}, {}


def source(ct, cols, rows, masked, raw=False):
    key = (ct, cols, rows, masked, raw)
    if key not in _sources:
        a = K.raster_cells(ct, cols, rows, 0xF0CA + 131 * ct + cols + 1000 * rows, raw)
        m = K.mask_bytes("hashed", cols, rows, 0x5EED + cols + 7 * rows) if masked else None
        _sources[key] = (a, m)
    return _sources[key]


def expected(ct, cols, rows, masked, what, flags, radius, raw=False):
    """the yardstick's answer, computed once per case and shared by the tuning arms; `what` an operation number or "convolve" """
    key = (ct, cols, rows, masked, what, flags, radius, raw)
    if key not in _expected:
        a, m = source(ct, cols, rows, masked, raw)
        if what == "convolve":
            _expected[key] = R.convolve(a, m, K.weights(*radius), bool(flags & NORMALIZE), bool(flags & WHOLE))
        else:
            _expected[key] = R.focal(what, a, m, radius[0], radius[1], bool(flags & WHOLE))
    return _expected[key]


def run(ec, ct, src, smask, cols, rows, what, flags, radius, want_mask):
    """one call through the C ABI -> (cells, mask bytes or None)"""
    L = ec.lib()
    n = cols * rows
    out_ct = ec.Float64 if what == "convolve" else L.ec_focal_result_type(what, ct)
    out = ec.CellBuffer.empty(n, out_ct)
    om = ec.Mask.empty(n) if want_mask else None
    sm, dm = (smask.mem.ptr if smask is not None else None), (om.mem.ptr if om is not None else None)
    if what == "convolve":
        w = np.ascontiguousarray(K.weights(*radius))
        ec._ffi.check(L.ec_focal_convolve(ct, src.mem.ptr, sm, cols, rows, w.ctypes.data_as(C.POINTER(C.c_double)), radius[0], radius[1], flags,
                                          out.mem.ptr, dm, ec.stream()))
        w[...] = np.nan   # the weights were read before the call returned
    else:
        ec._ffi.check(L.ec_focal(what, ct, src.mem.ptr, sm, cols, rows, radius[0], radius[1], flags, out.mem.ptr, dm, ec.stream()))
    return out.to_numpy(), (om.to_numpy() if om is not None else None)


def sweep(ec, ct, masked, raw=False):
    nans = 0
    for radius in K.RADII:
        for cols, rows in K.shapes(*radius):
            a, m = source(ct, cols, rows, masked, raw)
            src = ec.CellBuffer.from_vec(a.ravel())
            smask = ec.Mask.new(m.ravel()) if masked else None
            for what, flags in FOCAL_CALLS + [("convolve", f) for f in CONV_FLAGS]:
                exp, ev = expected(ct, cols, rows, masked, what, flags, radius, raw)
                want_mask = masked or bool(flags & WHOLE) or (cols + rows) % 2 == 0   # optional: given for half of the shapes
                got, gm = run(ec, ct, src, smask, cols, rows, what, flags, radius, want_mask)
                case = (ct, masked, what, flags, radius, cols, rows)
                by_class = raw and what not in (R.MIN, R.MAX)
                assert same_cells(got, exp, by_class), case
                if gm is not None:
                    assert np.array_equal(gm, ev.ravel()), case
                nans += int(np.isnan(exp).sum()) if exp.dtype.kind == "f" else 0
    return nans


@pytest.mark.parametrize("arm", ARMS, ids=ARM_IDS)
@pytest.mark.parametrize("masked", (False, True), ids=("plain", "masked"))
@pytest.mark.parametrize("ct", range(10))
def test_every_type_operation_radius_and_shape(ec, ct, masked, arm):
    for radius in K.RADII:
        assert 9 <= len(K.shapes(*radius)) <= 16
    with ec.tuned(**arm):
        sweep(ec, ct, masked)


@pytest.mark.parametrize("ct", (8, 9))
def test_raw_hashed_floats_nan_by_class(ec, ct):
    """the one test with NaNs: raw hashed bits with NaN and +-inf planted, plain and masked.  min / max stay bit for bit."""
    nans = sweep(ec, ct, False, raw=True) + sweep(ec, ct, True, raw=True)
    assert nans > 0   # the sources do hold NaNs, and they reach the results


@pytest.mark.parametrize("kind", [k for k in K.MASK_KINDS if k != "hashed"])
def test_special_masks(ec, kind):
    """all-zero, all-one, a single zero, a single one: every cell invalid, every cell valid, one hole filled from its neighbours, one
    cell spread over its footprint"""
    for ct in (ec.UInt8, ec.Int16, ec.Float32, ec.Float64):
        for radius in ((1, 1), (2, 1), (7, 7), (0, 0)):
            for cols, rows in ((K.TW + 1, K.TH + 1), (5, 3), (2 * K.TW + 1, 2)):
                a = K.raster_cells(ct, cols, rows, 0xAA + ct)
                m = K.mask_bytes(kind, cols, rows, ct + radius[0])
                src, smask = ec.CellBuffer.from_vec(a.ravel()), ec.Mask.new(m.ravel())
                for what, flags in FOCAL_CALLS:
                    exp, ev = R.focal(what, a, m, radius[0], radius[1], bool(flags & WHOLE))
                    got, gm = run(ec, ct, src, smask, cols, rows, what, flags, radius, True)
                    assert same_cells(got, exp) and np.array_equal(gm, ev.ravel()), (kind, ct, radius, cols, rows, what, flags)
                for flags in CONV_FLAGS:
                    exp, ev = R.convolve(a, m, K.weights(*radius), bool(flags & NORMALIZE), bool(flags & WHOLE))
                    got, gm = run(ec, ct, src, smask, cols, rows, "convolve", flags, radius, True)
                    assert same_cells(got, exp) and np.array_equal(gm, ev.ravel()), (kind, ct, radius, cols, rows, flags)


def test_impulses_at_tile_and_raster_corners(ec):
    """one non-zero cell at each position of the 2 x 2 block around every tile corner and at each raster corner, radius (2, 1): the
    output is exactly the clipped footprint — the sum holds the cell's value there and 0 elsewhere, the maximum likewise"""
    rx, ry = 2, 1
    for cols, rows in ((2 * K.TW + 1, 2 * K.TH + 1), (K.TW, K.TH), (K.TW + 1, K.TH - 1)):
        positions = K.impulse_positions(cols, rows)
        assert len(positions) >= (20 if cols > K.TW and rows > K.TH else 4)
        for ct, value in ((ec.UInt8, 200), (ec.Float32, 2.5), (ec.Int64, -3)):
            dt = K.NP_DTYPES[ct]
            for y, x in positions:
                a = np.zeros((rows, cols), dtype=dt)
                a[y, x] = value
                foot = np.zeros((rows, cols), dtype=bool)
                foot[max(0, y - ry):y + ry + 1, max(0, x - rx):x + rx + 1] = True
                src = ec.CellBuffer.from_vec(a.ravel())
                got, _ = run(ec, ct, src, None, cols, rows, R.SUM, 0, (rx, ry), False)
                assert np.array_equal(got.reshape(rows, cols), np.where(foot, np.float64(value), 0.0)), (ct, y, x, cols, rows)
                op = R.MAX if value > 0 else R.MIN
                got, _ = run(ec, ct, src, None, cols, rows, op, 0, (rx, ry), False)
                assert np.array_equal(got.reshape(rows, cols), np.where(foot, dt.type(value), dt.type(0))), (ct, y, x, cols, rows)


def test_min_max_follow_the_total_order(ec):
    """-0.0 before +0.0, -NaN first and +NaN last, negative floats by value: neither the raw bit patterns nor `<` give this order"""
    for ct in (ec.Float32, ec.Float64):
        a = K.order_edge_raster(K.NP_DTYPES[ct])
        src = ec.CellBuffer.from_vec(a.ravel())
        for op in (R.MIN, R.MAX):
            for radius in ((1, 0), (2, 0), (0, 0)):
                got, _ = run(ec, ct, src, None, a.shape[1], 1, op, 0, radius, False)
                assert same_cells(got, R.focal(op, a, None, radius[0], radius[1])[0]), (ct, op, radius)


def test_zero_sum_weights_normalized(ec):
    """Sobel weights sum to 0.0: with NORMALIZE a cell whose counted weights sum to 0.0 is invalid — every interior cell"""
    cols, rows = K.TW + 3, K.TH + 2
    a = K.raster_cells(ec.Int16, cols, rows, 0x50BE1)
    src = ec.CellBuffer.from_vec(a.ravel())
    L, w = ec.lib(), np.ascontiguousarray(K.SOBEL_X)
    for flags in (NORMALIZE, 0):
        exp, ev = R.convolve(a, None, w, bool(flags), False)
        out, om = ec.CellBuffer.empty(cols * rows, ec.Float64), ec.Mask.empty(cols * rows)
        ec._ffi.check(L.ec_focal_convolve(ec.Int16, src.mem.ptr, None, cols, rows, w.ctypes.data_as(C.POINTER(C.c_double)), 1, 1, flags, out.mem.ptr,
                                          om.mem.ptr, ec.stream()))
        assert same_cells(out.to_numpy(), exp) and np.array_equal(om.to_numpy(), ev.ravel())
        assert (ev[1:-1, 1:-1] == (0 if flags else 1)).all()


def test_more_than_a_grid_row_of_tiles_both_fronts(ec):
    """5 x 4 tiles with a ragged last row and column, every kind, masked: the two fronts and the tile numbering"""
    cols, rows, radius = 4 * K.TW + 9, 3 * K.TH + 5, (3, 2)
    for ct in (ec.UInt16, ec.Float64):
        a = K.raster_cells(ct, cols, rows, 0xB16 + ct)
        m = K.mask_bytes("hashed", cols, rows, 0xB17)
        src, smask = ec.CellBuffer.from_vec(a.ravel()), ec.Mask.new(m.ravel())
        for what, flags in ((R.MEAN, 0), (R.MIN, WHOLE), ("convolve", NORMALIZE)):
            exp, ev = R.convolve(a, m, K.weights(*radius), True, False) if what == "convolve" else R.focal(what, a, m, 3, 2, bool(flags & WHOLE))
            got, gm = run(ec, ct, src, smask, cols, rows, what, flags, radius, True)
            assert same_cells(got, exp) and np.array_equal(gm, ev.ravel()), (ct, what)


def test_captured_in_a_graph_and_replayed_without_allocation(ec):
    import torch
    L = ec.lib()
    side = torch.cuda.Stream()
    ec._ffi.check(L.ec_prepare_stream(side.cuda_stream))
    cols, rows, radius = 2 * K.TW + 5, K.TH + 3, (2, 1)
    a = K.raster_cells(ec.Int16, cols, rows, 0x6A9)
    m = K.mask_bytes("hashed", cols, rows, 0x6AA)
    t_src, t_mask = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(m.copy()).cuda()
    t_sum = torch.zeros(cols * rows, dtype=torch.float64, device="cuda")
    t_conv = torch.zeros(cols * rows, dtype=torch.float64, device="cuda")
    t_om = [torch.zeros(cols * rows, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    before, after = C.c_int64(), C.c_int64()
    ec._ffi.check(L.ec_stat_get(b"pool_allocs", C.byref(before)))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        w = np.ascontiguousarray(K.weights(*radius))
        ec._ffi.check(L.ec_focal(R.SUM, ec.Int16, t_src.data_ptr(), t_mask.data_ptr(), cols, rows, 2, 1, 0, t_sum.data_ptr(), t_om[0].data_ptr(), s))
        ec._ffi.check(L.ec_focal_convolve(ec.Int16, t_src.data_ptr(), t_mask.data_ptr(), cols, rows, w.ctypes.data_as(C.POINTER(C.c_double)), 2, 1, 0,
                                          t_conv.data_ptr(), t_om[1].data_ptr(), s))
        w[...] = 0.0   # gone before the replay: the weights travel in the captured kernel arguments
    for trial in range(2):
        if trial:
            a = K.raster_cells(ec.Int16, cols, rows, 0x6A9 + trial)
            t_src.copy_(torch.from_numpy(a.copy()))
        g.replay()
        torch.cuda.synchronize()
        exp, ev = R.focal(R.SUM, a, m, 2, 1)
        cexp, cev = R.convolve(a, m, K.weights(*radius))
        assert same_cells(t_sum.cpu().numpy(), exp) and np.array_equal(t_om[0].cpu().numpy(), ev.ravel())
        assert same_cells(t_conv.cpu().numpy(), cexp) and np.array_equal(t_om[1].cpu().numpy(), cev.ravel())
    ec._ffi.check(L.ec_stat_get(b"pool_allocs", C.byref(after)))
    assert after.value == before.value
