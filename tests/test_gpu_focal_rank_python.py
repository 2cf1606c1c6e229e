"""The Python surface of the window order statistics: CellBuffer / MaskedCellBuffer .focal_rank, .focal_median and .focal_majority —
result types, when a mask comes back (what `.focal(cols, "min", ...)` returns for the same receiver), the spellings of q, method and
radius, a median that removes a planted outlier and a majority that removes a planted single-cell class — and the C++ mirror's program."""
import numpy as np
import pytest

import focal_rank_cases as K
import focal_rank_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(K.UINT[a.dtype.itemsize])


def same(got, exp, ec):
    """a CellBuffer against the reference's cells, or a MaskedCellBuffer against its cells and mask bytes"""
    if isinstance(got, ec.MaskedCellBuffer):
        return np.array_equal(bits(got.buffer().to_numpy()), bits(exp[0]).ravel()) and np.array_equal(got.mask().to_numpy(), exp[1].ravel())
    return np.array_equal(bits(got.to_numpy()), bits(exp[0]).ravel())


def test_the_six_methods_against_the_reference(ec):
    cols, rows = 70, 40
    for ct in range(10):
        a = K.rank_raster(ct, cols, rows, 0x9A + ct)
        c = K.class_raster(ct, cols, rows, 0x9C + ct)
        m = K.mask_bytes("hashed", cols, rows, 0x9B)
        for src, majority in ((a, False), (c, True)):
            buf = ec.CellBuffer.from_vec(src.ravel())
            mb = ec.MaskedCellBuffer(ec.CellBuffer.from_vec(src.ravel()), ec.Mask.new(m.ravel()))
            plain, masked = R.ordered(src, None, 2, 1), R.ordered(src, m, 1, 1)
            like = buf.focal(cols, "min", radius=(2, 1))
            if majority:
                got = buf.focal_majority(cols, radius=(2, 1))
                assert type(got) is type(like) is ec.CellBuffer and got.cell_type() == ct and got.len() == cols * rows
                assert same(got, R.majority_pick(plain, False, src.dtype), ec), ct
                whole = buf.focal_majority(cols, (2, 1), True)
                assert isinstance(whole, ec.MaskedCellBuffer) and same(whole, R.majority_pick(plain, True, src.dtype), ec)
                got = mb.focal_majority(cols)   # the default radius (1, 1)
                assert isinstance(got, ec.MaskedCellBuffer) and got.cell_type() == ct and same(got, R.majority_pick(masked, False, src.dtype), ec)
                assert same(mb.focal_majority(cols, whole=True), R.majority_pick(masked, True, src.dtype), ec)
                continue
            got = buf.focal_rank(cols, (9, 10), "upper", radius=(2, 1))
            assert type(got) is type(like) is ec.CellBuffer and got.cell_type() == ct and got.len() == cols * rows
            assert same(got, R.pick(plain, 9, 10, R.UPPER, False, src.dtype), ec), ct
            assert same(buf.focal_rank(cols, radius=(2, 1)), R.pick(plain, 1, 2, R.LOWER, False, src.dtype), ec)   # the defaults: the lower median
            assert same(buf.focal_rank(cols, 0, radius=(2, 1)), (bits(like.to_numpy()), None), ec)                # q = 0: focal "min"
            assert same(buf.focal_rank(cols, 1, ec._ffi.EC_RANK_UPPER, [2, 1]), (bits(buf.focal(cols, "max", (2, 1)).to_numpy()), None), ec)
            whole = buf.focal_rank(cols, (1, 4), radius=(2, 1), whole=True)
            assert isinstance(whole, ec.MaskedCellBuffer) and whole.cell_type() == ct and same(whole, R.pick(plain, 1, 4, R.LOWER, True, src.dtype), ec)
            assert whole.counts() == ((cols - 4) * (rows - 2), cols * rows - (cols - 4) * (rows - 2))
            for method, number in (("lower", R.LOWER), ("upper", R.UPPER)):
                got = buf.focal_median(cols, (2, 1), method)
                assert isinstance(got, ec.CellBuffer) and same(got, R.pick(plain, 1, 2, number, False, src.dtype), ec)
                got = mb.focal_median(cols, method=method)   # the default radius (1, 1)
                assert isinstance(got, ec.MaskedCellBuffer) and got.cell_type() == ct and same(got, R.pick(masked, 1, 2, number, False, src.dtype), ec)
            assert same(mb.focal_rank(cols, (1, 3), "upper", whole=True), R.pick(masked, 1, 3, R.UPPER, True, src.dtype), ec)
            assert same(mb.focal_median(cols, whole=True), R.pick(masked, 1, 2, R.LOWER, True, src.dtype), ec)


def test_refusals_of_the_python_forms(ec):
    buf = ec.CellBuffer.from_vec(np.arange(12, dtype=np.uint8))
    for bad_q in (0.5, (1, 0), (3, 2), (1, 65536), "median", (1, 2, 3), True):
        with pytest.raises(ec.EcError):
            buf.focal_rank(4, bad_q)
    for bad_method in ("middle", 2, -1, None, True):
        with pytest.raises(ec.EcError, match="method"):
            buf.focal_rank(4, (1, 2), bad_method)
        with pytest.raises(ec.EcError, match="method"):
            buf.focal_median(4, method=bad_method)
    with pytest.raises(ec.EcError, match="EC_FOCAL_RADIUS_CAP"):
        buf.focal_median(4, radius=(8, 0))
    with pytest.raises(ec.EcError, match="EC_FOCAL_RANK_MAX_TAPS"):
        buf.focal_median(4, radius=(4, 4))
    with pytest.raises(ec.EcError, match="EC_FOCAL_RANK_MAX_TAPS"):
        buf.focal_majority(4, radius=(7, 2))
    with pytest.raises(AssertionError):
        buf.focal_majority(5)   # 12 cells are no raster of rows of 5
    empty = ec.CellBuffer.from_vec(np.zeros(0, np.uint8))
    assert empty.focal_median(0).len() == 0 and empty.focal_majority(0).len() == 0


def test_a_median_removes_a_planted_outlier(ec):
    """a smooth ramp with single hot and dead cells: the 3 x 3 median brings every one of them back between its neighbours, where the
    mean smears it over nine cells and the maximum spreads it"""
    cols, rows = 2 * K.TW + 5, K.TH + 7
    y, x = np.mgrid[0:rows, 0:cols]
    ramp = (1000 + 3 * x + 5 * y).astype(np.uint16)
    a = ramp.copy()
    spots = [(0, 0), (3, 7), (K.TH - 1, K.TW - 1), (K.TH, K.TW), (rows - 1, cols - 1), (9, 2 * K.TW)]
    for k, (i, j) in enumerate(spots):
        a[i, j] = 65535 if k % 2 == 0 else 0
    got = ec.CellBuffer.from_vec(a.ravel()).focal_median(cols).to_numpy().reshape(rows, cols)
    assert np.array_equal(got, R.focal_rank(a, None, 1, 1, 1, 2, R.LOWER)[0])
    assert got.max() < 65535 and got.min() > 0
    for i, j in spots:
        near = ramp[max(0, i - 1):i + 2, max(0, j - 1):j + 2]
        assert near.min() <= got[i, j] <= near.max(), (i, j)
    smeared = ec.CellBuffer.from_vec(a.ravel()).focal(cols, "mean").to_numpy().reshape(rows, cols)
    assert abs(smeared[3, 8] - float(ramp[3, 8])) > 100 and abs(float(got[3, 8]) - float(ramp[3, 8])) <= 8


def test_a_majority_removes_a_planted_single_cell_class(ec):
    """a two-class map (the boundary a straight column) with single cells of a third class: the 3 x 3 majority removes every one of them
    and leaves the map as it was, the boundary included"""
    cols, rows = K.TW + 9, K.TH + 3
    classes = np.where(np.arange(cols)[None, :] < K.TW + 2, 3, 8).astype(np.uint8) * np.ones((rows, 1), np.uint8)
    a = classes.copy()
    for i, j in [(0, 0), (2, 5), (K.TH, K.TW), (K.TH - 1, K.TW + 1), (rows - 1, cols - 1), (rows - 1, 10)]:
        a[i, j] = 200
    got = ec.CellBuffer.from_vec(a.ravel()).focal_majority(cols).to_numpy().reshape(rows, cols)
    assert np.array_equal(got, R.focal_majority(a, None, 1, 1)[0])
    assert (got != 200).all() and np.array_equal(got, classes)
    masked = ec.MaskedCellBuffer(ec.CellBuffer.from_vec(a.ravel()), ec.Mask.new((a != 200).astype(np.uint8).ravel())).focal_majority(cols)
    assert np.array_equal(masked.buffer().to_numpy().reshape(rows, cols), classes) and masked.counts() == (cols * rows, 0)


def test_cpp_mirror_focal_rank_program():
    """erased-cells_amd/host/test_focal_rank_mirror.cpp: the C++ mirror's focal_rank / focal_median / focal_majority on cells worked
    out by hand"""
    import os
    import subprocess
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "erased-cells_amd", "host")
    binary = os.path.join(host, "test_focal_rank_mirror")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", host, "-s", "test_focal_rank_mirror"])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
