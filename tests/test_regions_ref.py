"""tests/regions_ref.py, the flood-fill reference of ec_regions, held to answers it shares no step with: scipy.ndimage.label per class
(whose numbering for a single class is the first cell in raster order), a scalar union-find transcription of the header's rule, and
cells worked out by hand."""
import numpy as np
import pytest
from scipy import ndimage

import regions_cases as K
import regions_ref as R

STRUCT = {4: ndimage.generate_binary_structure(2, 1), 8: ndimage.generate_binary_structure(2, 2)}


def by_union_find(cells, valid, connectivity):
    """the header's rule, transcribed: join every pair of neighbouring, valid, equal cells; the root is the least index of a set"""
    rows, cols = np.shape(cells if cells is not None else valid)
    key = R.bits(cells).ravel() if cells is not None else np.zeros(rows * cols, np.uint64)
    ok = np.asarray(valid).ravel() != 0 if valid is not None else np.ones(rows * cols, bool)
    up = list(range(rows * cols))

    def find(i):
        while up[i] != i:
            up[i] = up[up[i]]
            i = up[i]
        return i

    for y in range(rows):
        for x in range(cols):
            for y2, x2 in ((y, x + 1), (y + 1, x)) + (((y + 1, x + 1), (y + 1, x - 1)) if connectivity == 8 else ()):
                if (connectivity == 4 and abs(y - y2) + abs(x - x2) != 1) or (connectivity == 8 and max(abs(y - y2), abs(x - x2)) != 1):
                    continue
                if not (0 <= y2 < rows and 0 <= x2 < cols):
                    continue
                i, j = y * cols + x, y2 * cols + x2
                if ok[i] and ok[j] and key[i] == key[j]:
                    a, b = find(i), find(j)
                    up[max(a, b)] = min(a, b)
    root = np.array([find(i) if ok[i] else -1 for i in range(rows * cols)], np.int64)
    size = np.where(root >= 0, np.bincount(root[root >= 0], minlength=rows * cols)[np.maximum(root, 0)], 0)
    return root.reshape(rows, cols), size.reshape(rows, cols)


def test_a_single_class_is_scipys_label_array():
    rng = np.random.default_rng(0x5C1)
    for k in range(120):
        rows, cols = rng.integers(1, 40, 2)
        m = rng.random((rows, cols)) < rng.choice([0.3, 0.59, 0.8])
        for c in (4, 8):
            want, count = ndimage.label(m, STRUCT[c])
            labels, mask, kept = R.regions(None, m.astype(np.uint8), c, R.DENSE)
            assert kept == count and np.array_equal(labels, want) and np.array_equal(mask, m.astype(np.uint8)), (k, c)


def test_several_classes_against_scipy_up_to_the_order_preserving_renaming():
    rng = np.random.default_rng(0x5C2)
    for k in range(40):
        rows, cols = rng.integers(1, 30, 2)
        cells = rng.integers(0, 3, (rows, cols)).astype(np.uint16)
        valid = (rng.random((rows, cols)) < 0.9).astype(np.uint8) if k % 2 else None
        for c in (4, 8):
            root, size = R.fill(cells, valid, c)
            first = {}                       # (class, scipy's label) -> the least index it covers
            name = np.full((rows, cols), -1, np.int64)
            for cls in range(3):
                lab, count = ndimage.label((cells == cls) & (valid != 0 if valid is not None else True), STRUCT[c])
                for l in range(1, count + 1):
                    at = np.flatnonzero(lab.ravel() == l)
                    first[(cls, l)] = at[0]
                    name.ravel()[at] = at[0]
                    assert np.all(size.ravel()[at] == at.size)
            assert np.array_equal(root, name), (k, c)
            labels, _, kept = R.finish(root, size, R.DENSE)
            order = sorted(first.values())
            assert kept == len(order) and np.array_equal(labels, np.where(root >= 0, np.searchsorted(order, np.maximum(root, 0)) + 1, 0))


def test_against_the_union_find_transcription():
    for case in K.cases([(K.TW + 1, 3), (5, K.TH + 1), (17, 19), (1, 1), (1, 9), (9, 1)]):
        cols, rows, pattern, mask = case
        for c in (4, 8):
            for got, want in zip(K.filled(case, c), by_union_find(K.cells(cols, rows, pattern), K.valid(cols, rows, mask), c)):
                assert np.array_equal(got, want), (case, c)
            if pattern in K.BINARY:
                for got, want in zip(K.filled(case, c, "mask"), by_union_find(None, K.mask_form(case), c)):
                    assert np.array_equal(got, want), (case, c, "mask form")


def lab(cells, valid=None, c=4, numbering=R.DENSE, min_cells=0):
    labels, mask, k = R.regions(None if cells is None else np.array(cells), None if valid is None else np.array(valid, np.uint8), c, numbering, min_cells)
    return labels.tolist(), mask.tolist(), k


def test_cells_worked_out_by_hand():
    u = [[1, 0, 1], [1, 0, 1], [1, 1, 1]]            # a U whose arms meet only in the last row
    assert lab(None, u) == ([[1, 0, 1], [1, 0, 1], [1, 1, 1]], u, 1)
    assert lab(None, u, numbering=R.ROOT)[0] == [[1, 0, 1], [1, 0, 1], [1, 1, 1]]
    assert lab(u)[0] == [[1, 2, 1], [1, 2, 1], [1, 1, 1]] and lab(u, numbering=R.ROOT)[0] == [[1, 2, 1], [1, 2, 1], [1, 1, 1]]
    pair = [[1, 0], [0, 1]]                          # a diagonal pair: two regions under 4, one under 8
    assert lab(None, pair) == ([[1, 0], [0, 2]], pair, 2) and lab(None, pair, c=8) == ([[1, 0], [0, 1]], pair, 1)
    assert lab(None, pair, numbering=R.ROOT)[0] == [[1, 0], [0, 4]]
    anti = [[0, 1], [1, 0]]
    assert lab(None, anti) == ([[0, 1], [2, 0]], anti, 2) and lab(None, anti, c=8) == ([[0, 1], [1, 0]], anti, 1)
    end = [[0, 0, 1], [1, 0, 0]]                     # the row end does not wrap: indices 2 and 3 are not neighbours
    assert lab(None, end, c=8) == ([[0, 0, 1], [2, 0, 0]], end, 2)
    zeros = np.array([[0.0, -0.0, 0.0]])             # -0.0 beside +0.0: different bits, different classes
    assert lab(zeros)[0] == [[1, 2, 3]] and lab(zeros.astype(np.float32))[0] == [[1, 2, 3]]
    nans = np.array([[0x7FC00000, 0x7FC00000, 0x7FC00001, 0x7FC00000]], np.uint32).view(np.float32)   # two NaN payloads
    assert lab(nans)[0] == [[1, 1, 2, 3]]
    assert lab([[7]]) == ([[1]], [[1]], 1) and lab(None, [[0]]) == ([[0]], [[0]], 0) and lab([[7]], [[0]]) == ([[0]], [[0]], 0)
    # the sieve: size >= min_cells; dropped regions take no dense number, and K counts the kept ones under either numbering
    m = [[1, 0, 1, 1, 0, 1, 1, 1]]
    assert lab(None, m, min_cells=2) == ([[0, 0, 1, 1, 0, 2, 2, 2]], [[0, 0, 1, 1, 0, 1, 1, 1]], 2)
    assert lab(None, m, min_cells=3) == ([[0, 0, 0, 0, 0, 1, 1, 1]], [[0, 0, 0, 0, 0, 1, 1, 1]], 1)
    assert lab(None, m, min_cells=3, numbering=R.ROOT) == ([[0, 0, 0, 0, 0, 6, 6, 6]], [[0, 0, 0, 0, 0, 1, 1, 1]], 1)
    assert lab(None, m, min_cells=1) == lab(None, m) == ([[1, 0, 2, 2, 0, 3, 3, 3]], m, 3) and lab(None, m, min_cells=4)[2] == 0
    # without validity bytes the labels are the same: zero bits wherever there is no kept region
    labels, none, k = R.regions(None, np.array(m, np.uint8), 4, R.DENSE, 3, dst_mask=False)
    assert labels.tolist() == [[0, 0, 0, 0, 0, 1, 1, 1]] and none is None and k == 1


def test_the_patterns_are_what_their_names_say():
    c = K.TW + 1
    r = K.TH + 1
    n = c * r
    case = lambda p: (c, r, p, "none")
    assert R.finish(*K.filled(case("checkerboard"), 4))[2] == n and R.finish(*K.filled(case("checkerboard"), 8))[2] == 2
    for p in ("serpentine", "spiral", "comb-last-row", "comb-last-column"):
        for conn in (4, 8):
            root, size = K.filled(case(p), conn, "mask")
            assert set(np.unique(root)) == {-1, 0} and size.max() == (root == 0).sum() > n // 3, p   # one region, rooted in tile 0
    for p in ("diagonal-stripes", "anti-diagonal-stripes"):
        assert R.finish(*K.filled(case(p), 4, "mask"))[2] > 10 * R.finish(*K.filled(case(p), 8, "mask"))[2]
    assert R.finish(*K.filled(case("all"), 4))[2] == 1 and R.finish(*K.filled(case("none"), 4, "mask"))[2] == 0
    for p, dt in (("wide2", np.uint16), ("wide4", np.uint32), ("wide8", np.uint64)):
        a = K.cells(c, r, p)
        assert a.dtype == dt and len(np.unique(a)) == 3 and len(np.unique(a & dt((1 << (8 * (a.itemsize - 1))) - 1))) == 1
    assert K.cells(c, r, "float-specials").dtype == np.float32
    seam = K.valid(c, r, "seam")
    assert not seam[K.TH - 1].any() and not seam[:, K.TW - 1].any() and seam[0, 0] and seam[K.TH, K.TW]
    for cols, rows, pattern, mask in K.cases():
        assert cols * rows <= R.BUDGET
