"""The Python surface of the moving-window operations: CellBuffer.focal / .convolve, MaskedCellBuffer.focal / .convolve, Mask.dilate /
.erode — result types, when a mask comes back, the spellings of the operation, and the morphology of masks against plain numpy."""
import numpy as np
import pytest

import focal_cases as K
import focal_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(K.UINT[a.dtype.itemsize])


def test_result_types_and_when_a_mask_comes_back(ec):
    cols, rows = 70, 40
    for ct in range(10):
        a = K.raster_cells(ct, cols, rows, 0x9A + ct)
        m = K.mask_bytes("hashed", cols, rows, 0x9B)
        buf = ec.CellBuffer.from_vec(a.ravel())
        mb = ec.MaskedCellBuffer(ec.CellBuffer.from_vec(a.ravel()), ec.Mask.new(m.ravel()))
        for name, op in R.OPS.items():
            out_ct = ec.Float64 if name in ("sum", "mean") else ct
            got = buf.focal(cols, name, radius=(2, 1))
            assert isinstance(got, ec.CellBuffer) and got.cell_type() == out_ct and got.len() == cols * rows
            exp, ev = R.focal(op, a, None, 2, 1)
            assert np.array_equal(bits(got.to_numpy()), bits(exp).ravel()), (ct, name)
            assert np.array_equal(bits(buf.focal(cols, op, (2, 1)).to_numpy()), bits(exp).ravel())   # the constant, radius by position
            whole = buf.focal(cols, name, radius=(2, 1), whole=True)
            exp, ev = R.focal(op, a, None, 2, 1, whole=True)
            assert isinstance(whole, ec.MaskedCellBuffer) and whole.cell_type() == out_ct
            assert np.array_equal(bits(whole.buffer().to_numpy()), bits(exp).ravel()) and np.array_equal(whole.mask().to_numpy(), ev.ravel())
            assert whole.counts() == ((cols - 4) * (rows - 2), cols * rows - (cols - 4) * (rows - 2))
            got = mb.focal(cols, name)   # the default radius (1, 1)
            exp, ev = R.focal(op, a, m, 1, 1)
            assert isinstance(got, ec.MaskedCellBuffer) and got.cell_type() == out_ct
            assert np.array_equal(bits(got.buffer().to_numpy()), bits(exp).ravel()) and np.array_equal(got.mask().to_numpy(), ev.ravel())
        w = K.weights(2, 1)
        got = buf.convolve(cols, w)
        assert isinstance(got, ec.CellBuffer) and got.cell_type() == ec.Float64
        assert np.array_equal(bits(got.to_numpy()), bits(R.convolve(a, None, w)[0]).ravel())
        got = buf.convolve(cols, w.tolist(), normalize=True, whole=True)
        exp, ev = R.convolve(a, None, w, True, True)
        assert isinstance(got, ec.MaskedCellBuffer) and np.array_equal(bits(got.buffer().to_numpy()), bits(exp).ravel())
        assert np.array_equal(got.mask().to_numpy(), ev.ravel())
        got = mb.convolve(cols, w, normalize=True)
        exp, ev = R.convolve(a, m, w, True, False)
        assert np.array_equal(bits(got.buffer().to_numpy()), bits(exp).ravel()) and np.array_equal(got.mask().to_numpy(), ev.ravel())


def test_refusals_of_the_python_forms(ec):
    buf = ec.CellBuffer.from_vec(np.arange(12, dtype=np.uint8))
    with pytest.raises(ec.EcError, match="median"):
        buf.focal(4, "median")
    with pytest.raises(ec.EcError, match="odd shape"):
        buf.convolve(4, np.ones((2, 3)))
    with pytest.raises(ec.EcError, match="odd shape"):
        buf.convolve(4, np.ones(3))
    with pytest.raises(ec.EcError, match="EC_FOCAL_RADIUS_CAP"):
        buf.focal(4, "sum", radius=(8, 0))
    with pytest.raises(ec.EcError, match="EC_FOCAL_RADIUS_CAP"):
        buf.convolve(4, np.ones((17, 1)))
    with pytest.raises(AssertionError):
        buf.focal(5, "sum")   # 12 cells are no raster of rows of 5
    assert ec.CellBuffer.from_vec(np.zeros(0, np.uint8)).focal(0, "max").len() == 0


def numpy_dilate(m, rx, ry):
    """any byte of the clipped footprint set, by plain loops over the offsets"""
    rows, cols = m.shape
    out = np.zeros_like(m)
    for dy in range(-ry, ry + 1):
        for dx in range(-rx, rx + 1):
            ys, xs = slice(max(0, dy), rows + min(0, dy)), slice(max(0, dx), cols + min(0, dx))
            yd, xd = slice(max(0, -dy), rows + min(0, -dy)), slice(max(0, -dx), cols + min(0, -dx))
            out[yd, xd] |= m[ys, xs]
    return out


def numpy_erode(m, rx, ry):
    """all bytes of the CLIPPED footprint set: a cell outside the raster does not count against"""
    return 1 - numpy_dilate(1 - m, rx, ry)


def test_dilate_and_erode_of_a_mask(ec):
    cols, rows = 70, 40
    m = (K.hashed_bytes(cols * rows, 0xD11A) % 10 < 2).astype(np.uint8).reshape(rows, cols)   # 20 % set
    dense = (K.hashed_bytes(cols * rows, 0xE20D) % 10 < 9).astype(np.uint8).reshape(rows, cols)
    for radius in ((1, 1), (3, 0), (0, 2), (7, 7), (0, 0)):
        for src in (m, dense):
            mask = ec.Mask.new(src.ravel())
            d, e = mask.dilate(cols, radius), mask.erode(cols, radius)
            assert isinstance(d, ec.Mask) and d.len() == cols * rows
            assert np.array_equal(d.to_numpy().reshape(rows, cols), numpy_dilate(src, *radius)), radius
            assert np.array_equal(e.to_numpy().reshape(rows, cols), numpy_erode(src, *radius)), radius
    mask = ec.Mask.new(m.ravel())
    assert np.array_equal(mask.dilate(cols).to_numpy(), numpy_dilate(m, 1, 1).ravel())   # the default radius
    # bytes other than 1 count as set, and the result's bytes are the extremes of the source's
    odd = ec.Mask(4, ec.CellBuffer.from_vec(np.array([0, 7, 0, 0], np.uint8)).mem)
    assert odd.dilate(4, (1, 0)).to_numpy().astype(bool).tolist() == [True, True, True, False]


def test_closing_keeps_every_set_cell(ec):
    """erode(dilate(m)) — the morphological closing — never clears a cell of m"""
    cols, rows = 70, 40
    for seed in (1, 2):
        m = (K.hashed_bytes(cols * rows, 0xC105E + seed) % 10 < 3).astype(np.uint8).reshape(rows, cols)
        mask = ec.Mask.new(m.ravel())
        for radius in ((1, 1), (2, 3), (7, 7)):
            closed = mask.dilate(cols, radius).erode(cols, radius).to_numpy().reshape(rows, cols)
            assert (closed[m != 0] != 0).all(), radius
            assert np.array_equal(closed, numpy_erode(numpy_dilate(m, *radius), *radius))
            assert (mask & mask.dilate(cols, radius)).counts() == mask.counts()


def test_cpp_mirror_focal_program():
    """erased-cells_amd/host/test_focal_mirror.cpp: the C++ mirror's focal / convolve / dilate / erode on cells worked out by hand"""
    import os
    import subprocess
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "erased-cells_amd", "host")
    binary = os.path.join(host, "test_focal_mirror")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", host, "-s", "test_focal_mirror"])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
