"""tests/distance_ref.py, the reference of ec_distance, held to independent answers: scipy's Euclidean distance transform, a scalar
transcription of the header's rule, Mask.dilate's rule through tests/focal_ref.py, and cells worked out by hand."""
import numpy as np
import pytest

import distance_cases as K
import distance_ref as R
import focal_ref


def random_mask(rows, cols, per_thousand, seed):
    return (K.hashed(rows * cols, seed) % np.uint64(1000) < np.uint64(per_thousand)).reshape(rows, cols).astype(np.uint8)


MASKS = [random_mask(r, c, d, 0x5C1 + 31 * k) for k, (r, c, d) in enumerate(
    [(1, 1, 1000), (1, 17, 200), (23, 1, 200), (9, 13, 500), (31, 29, 100), (40, 64, 20), (65, 33, 5), (50, 50, 900), (12, 90, 300), (77, 5, 50)])]


def test_against_scipy():
    """numpy.rint(distance_transform_edt(~m) ** 2): scipy's f64 distances are exact square roots at these sizes, so the rounded square is
    the integer"""
    from scipy import ndimage
    for m in MASKS + [K.mask(c, r, p) for (c, r, p) in ((65, 131, "random1"), (129, 63, "diagonal"), (257, 300, "random001"), (64, 3, "checkerboard"))]:
        d2, any_target = R.squared(m)
        if not any_target:
            assert (d2 == -1).all()
            continue
        want = np.rint(ndimage.distance_transform_edt(m == 0) ** 2).astype(np.int64)
        assert np.array_equal(d2, want), m.shape


def scalar_rule(m, max_sq, out_type):
    """the header's rule, cell by cell and target by target, in Python integers"""
    rows, cols = m.shape
    targets = [(y, x) for y in range(rows) for x in range(cols) if m[y, x] != 0]
    cells = np.zeros((rows, cols), np.uint32 if out_type == R.U32 else np.float64)
    valid = np.zeros((rows, cols), np.uint8)
    for i in range(rows):
        for j in range(cols):
            if not targets:
                continue
            d2 = min((i - y) ** 2 + (j - x) ** 2 for (y, x) in targets)
            if d2 <= max_sq:
                valid[i, j] = 1
                cells[i, j] = d2 if out_type == R.U32 else np.sqrt(np.float64(d2))
    return cells, valid


def test_against_a_scalar_transcription_of_the_rule():
    for m in MASKS[:5] + [np.zeros((4, 6), np.uint8), np.full((3, 5), 7, np.uint8)]:
        for max_sq in (0, 1, 2, 9, 10, R.UNLIMITED):
            for out_type in (R.U32, R.F64):
                got, gv = R.distance(m, max_sq, out_type)
                exp, ev = scalar_rule(m, max_sq, out_type)
                assert got.dtype == exp.dtype and np.array_equal(got.view(np.uint8), exp.view(np.uint8)) and np.array_equal(gv, ev), (m.shape, max_sq, out_type)


def test_against_the_dilation():
    """d2 <= 2 is the 3 x 3 dilation and d2 <= 1 the 4-neighbourhood, by Mask.dilate's rule (ec_focal MAX over the bytes, clipped)"""
    for m in MASKS:
        binary = (m != 0).astype(np.uint8)
        square = focal_ref.focal(focal_ref.MAX, binary, None, 1, 1)[0]
        assert np.array_equal(R.distance(m, 2, R.U32)[1], (np.asarray(square).reshape(m.shape) != 0).astype(np.uint8)), m.shape
        rows, cols = m.shape
        pad = np.pad(binary, 1)
        cross = pad[1:-1, 1:-1] | pad[:-2, 1:-1] | pad[2:, 1:-1] | pad[1:-1, :-2] | pad[1:-1, 2:]
        assert np.array_equal(R.distance(m, 1, R.U32)[1], cross), m.shape


def test_cells_worked_out_by_hand():
    m = np.array([[1, 0, 0, 0],
                  [0, 0, 0, 0],
                  [0, 0, 0, 9]], np.uint8)
    d2, any_target = R.squared(m)
    assert any_target and d2.tolist() == [[0, 1, 4, 4], [1, 2, 2, 1], [4, 4, 1, 0]]
    cells, valid = R.distance(m, R.UNLIMITED, R.F64)
    assert cells.dtype == np.float64 and cells[1, 1] == np.sqrt(2.0) and cells[0, 2] == 2.0 and valid.all() and valid.dtype == np.uint8
    # d2 == max_sq is inside, max_sq + 1 outside; an invalid cell holds zero bits
    cells, valid = R.distance(m, 2, R.U32)
    assert cells.dtype == np.uint32 and cells.tolist() == [[0, 1, 0, 0], [1, 2, 2, 1], [0, 0, 1, 0]] and valid.tolist() == [[1, 1, 0, 0], [1, 1, 1, 1], [0, 0, 1, 1]]
    cells, valid = R.distance(m, 1, R.F64)
    assert valid.tolist() == [[1, 1, 0, 0], [1, 0, 0, 1], [0, 0, 1, 1]] and cells.view(np.uint64)[valid == 0].max() == 0
    assert R.distance(m, 0, R.U32)[1].tolist() == [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]]
    # the empty mask: no cell is valid, whatever the limit; the full mask: every d2 is 0
    for max_sq in (0, 5, R.UNLIMITED):
        cells, valid = R.distance(np.zeros((3, 4), np.uint8), max_sq, R.F64)
        assert not valid.any() and not cells.view(np.uint64).any()
        cells, valid = R.distance(np.full((3, 4), 255, np.uint8), max_sq, R.U32)
        assert valid.all() and not cells.any()
    # the raster does not wrap, and the largest d2 of a line is (n - 1)^2
    line = np.zeros((1, 32768), np.uint8)
    line[0, 0] = 1
    d2, _ = R.squared(line)
    assert d2[0, -1] == 32767 ** 2 and d2[0, 1] == 1 and R.distance(line)[0][0, -1] == 32767.0
    far = K.squared(32768, 2, "corner11")[0]
    assert far[0, 0] == 32767 ** 2 + 1 and far[1, 0] == 32767 ** 2


def test_every_case_is_within_the_budget_and_says_what_it_names():
    for cols, rows, pattern in K.cases():
        m = K.mask(cols, rows, pattern)
        assert m.shape == (rows, cols) and m.dtype == np.uint8 and cols * rows * max(1, int((m != 0).sum())) <= R.BUDGET
    assert not K.mask(65, 131, "none").any() and K.mask(65, 131, "all").all()
    assert set(np.unique(K.mask(129, 129, "all"))) == {1, 2, 0x80, 0xFF}          # a target is any nonzero byte
    assert (K.mask(129, 129, "last-column-one")[:, :-1] == 0).all() and (K.mask(129, 129, "last-column-one") != 0).sum() == 1
    for p in ("corner00", "corner01", "corner10", "corner11", "centre", "edge-left", "edge-right"):
        assert (K.mask(129, 129, p) != 0).sum() == 1
    assert K.mask(129, 129, "edge-left")[K.W - 1, K.T - 1] and K.mask(129, 129, "edge-right")[K.W, K.T]
    assert (K.mask(129, 65, "full-row") != 0).sum() == 129 and (K.mask(129, 65, "full-column") != 0).sum() == 65
    g0 = [int(np.flatnonzero(K.mask(65, 131, "decreasing-g")[:, x])[0]) for x in range(40)]
    assert all(a > b for a, b in zip(g0, g0[1:]))                                # g of row 0 falls strictly along the row
    assert set(K.patterns_of((129, 129))) == set(K.PATTERNS) and {"random50", "random1", "random001"} <= set(K.PATTERNS)
    assert {(1, 32768), (32768, 1), (32768, 2), (257, 300), (1, 1)} <= set(K.SHAPES)
