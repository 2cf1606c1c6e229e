"""The inputs of tests/regions_cases.py expose each modelled mistake of the kernels of ec_regions — shown without a GPU.

`model` below is the labelling as the kernels run it (csrc/ec_regions_cell.hpp, ec_regions_kernels.hpp), in numpy and plain Python:
the joins of neighbouring, valid, equal cells sorted into those inside a tile of TW x TH cells and those across a seam; a union-find
over the first (parent[i] = the least cell of i's piece of the tile), then over the second; the flattening; the sizes at the roots; the
sieve; the dense numbers as a scan over blocks of SCAN cells; K; the stored cell.  One mistake can be switched on at a time.  The
fault-free model equals tests/regions_ref.py on every case; every mistake changes at least one label, mask byte or K of at least one
case and form that the GPU tests run."""
import numpy as np
import pytest

import regions_cases as K
import regions_ref as R

TW, TH, SCAN = K.TW, K.TH, K.SCAN
UNWRITTEN = int(np.array([R.UNWRITTEN] * 4, np.uint8).view(np.int32)[0])   # a label no store reached (the GPU tests pre-fill their outputs)

FAULTS = ["right-seam-unjoined", "bottom-seam-unjoined", "diagonal-seam-unjoined", "anti-diagonal-seam-unjoined", "corner-tile-forgotten",
          "diagonals-joined-under-4", "joined-across-the-row-end", "mask-ignored", "numeric-equality", "low-bytes-only", "one-level-of-compression",
          "sizes-per-tile", "sieve-off-by-one", "dense-out-of-root-order", "dense-counts-dropped", "scan-carry-dropped", "k-counts-dropped",
          "dropped-keeps-its-label", "zero-bits-not-written"]


def joins(cells, valid, connectivity, fault):
    """(i, j, across): the index pairs of joined neighbours, i < j, and whether the pair lies across a seam"""
    rows, cols = np.shape(cells if cells is not None else valid)
    n = rows * cols
    ok = np.ones((rows, cols), bool) if valid is None or fault == "mask-ignored" else np.asarray(valid) != 0
    if cells is None:
        equal = lambda a, b: np.ones(a.shape, bool)
    elif fault == "numeric-equality":
        equal = lambda a, b: cells.ravel()[a] == cells.ravel()[b]
    else:
        key = R.bits(cells).ravel()
        if fault == "low-bytes-only":
            key = key & np.uint64((1 << (8 * max(1, cells.dtype.itemsize - 1))) - 1) if cells.dtype.itemsize > 1 else key
        equal = lambda a, b: key[a] == key[b]
    y, x = np.mgrid[0:rows, 0:cols]
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 or fault == "diagonals-joined-under-4" else [])
    out = []
    for dy, dx in steps:
        inside = (y + dy < rows) & (x + dx >= 0) & (x + dx < cols)
        a = (y * cols + x)[inside]
        b = a + dy * cols + dx
        over_x = ((x // TW) != ((x + dx) // TW))[inside]
        over_y = ((y // TH) != ((y + dy) // TH))[inside]
        keep = ok.ravel()[a] & ok.ravel()[b] & equal(a, b)
        if fault == "right-seam-unjoined" and (dy, dx) == (0, 1):
            keep &= ~over_x
        if fault == "bottom-seam-unjoined" and (dy, dx) == (1, 0):
            keep &= ~over_y
        if fault == "diagonal-seam-unjoined" and (dy, dx) == (1, 1):
            keep &= ~(over_x | over_y)
        if fault == "anti-diagonal-seam-unjoined" and (dy, dx) == (1, -1):
            keep &= ~(over_x | over_y)
        if fault == "corner-tile-forgotten" and dy == 1 and dx != 0:
            keep &= ~(over_x & over_y)
        out.append((a[keep], b[keep], (over_x | over_y)[keep]))
    if fault == "joined-across-the-row-end":     # index i + 1 taken for the right neighbour without looking at the column
        a = (np.arange(1, rows) * cols - 1)
        keep = ok.ravel()[a] & ok.ravel()[a + 1] & equal(a, a + 1)
        out.append((a[keep], a[keep] + 1, np.ones(int(keep.sum()), bool)))
    i, j, across = (np.concatenate(p) for p in zip(*out))
    return i, j, across, ok.ravel(), n


def unite(parent, pairs, halve):
    for a, b in pairs:
        while parent[a] != a:
            if halve:
                parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            if halve:
                parent[b] = parent[parent[b]]
            b = parent[b]
        if a != b:
            parent[max(a, b)] = min(a, b)


def parents(cells, valid, connectivity, fault):
    """(root per cell as the flatten kernel leaves it, the tile-local root per cell, valid)"""
    i, j, across, ok, n = joins(cells, valid, connectivity, fault)
    parent = list(range(n))
    unite(parent, zip(i[~across].tolist(), j[~across].tolist()), True)
    for c in range(n):                                   # the tile kernel's last step: parent[i] = the tile-local root
        r = c
        while parent[r] != r:
            r = parent[r]
        parent[c] = r
    piece = np.array(parent, np.int64)
    unite(parent, zip(i[across].tolist(), j[across].tolist()), False)
    if fault == "one-level-of-compression":
        root = np.array([parent[parent[c]] for c in range(n)], np.int64)
    else:
        root = np.empty(n, np.int64)
        for c in range(n):
            r = c
            while parent[r] != r:
                r = parent[r]
            root[c] = r
    return root, piece, ok


def store(root, piece, ok, shape, numbering, min_cells, dst_mask, fault):
    n = root.size
    at = piece if fault == "sizes-per-tile" else root    # where a cell's count is added
    count = np.bincount(at[ok], minlength=n)
    is_root = ok & (root == np.arange(n))
    need = min(min_cells, 0xFFFFFFFF)
    kept_root = is_root & ((count > need) if fault == "sieve-off-by-one" and need > 1 else (need <= 1) | (count >= need))
    k = int(is_root.sum() if fault == "k-counts-dropped" else kept_root.sum())
    number = np.zeros(n, np.int64)
    flags = is_root if fault == "dense-counts-dropped" else kept_root
    if fault == "dense-out-of-root-order":               # numbered down the columns instead of along the rows
        order = np.argsort((np.arange(n) % shape[1]) * shape[0] + np.arange(n) // shape[1], kind="stable")
        number[order] = np.cumsum(flags[order])
    elif fault == "scan-carry-dropped":
        for b in range(0, n, SCAN):
            number[b:b + SCAN] = np.cumsum(flags[b:b + SCAN])
    else:
        number = np.cumsum(flags)
    number = np.where(kept_root, number, 0)
    r = np.maximum(root, 0)
    kept = ok & kept_root[r]
    label = np.where(kept, number[r] if numbering == K.DENSE else root + 1, 0)
    if fault == "dropped-keeps-its-label" and numbering == K.ROOT:   # a dropped region has no dense number to keep
        label = np.where(ok, root + 1, 0)
    if fault == "zero-bits-not-written" and not dst_mask:
        label = np.where(kept, label, UNWRITTEN)
    return label.astype(np.int32).reshape(shape), (kept.astype(np.uint8).reshape(shape) if dst_mask else None), k


def forms(case):
    """(connectivity, numbering, min_cells, dst_mask) as tests/test_gpu_regions.py runs a case: everything with validity bytes, and the
    dense labels of one connectivity without them"""
    out = [(c, numbering, m, True) for c in (4, 8) for numbering in (K.ROOT, K.DENSE) for m in K.sieves(case)]
    return out + [(4 if len(case[2]) % 2 else 8, K.DENSE, m, False) for m in (0, 2, 5)]


def differs(case, fault, memo):
    cols, rows, pattern, mask = case
    for c, numbering, min_cells, dst_mask in forms(case):
        if (c, fault) not in memo:
            memo.clear()
            memo[(c, fault)] = parents(K.cells(cols, rows, pattern), K.valid(cols, rows, mask), c, fault)
        got = store(*memo[(c, fault)], (rows, cols), numbering, min_cells, dst_mask, fault)
        want = K.expected(case, c, numbering, min_cells, dst_mask=dst_mask)
        if got[2] != want[2] or not np.array_equal(got[0], want[0]) or (dst_mask and not np.array_equal(got[1], want[1])):
            return True
    return False


QUICK = [s for s in K.SMALL if s[0] * s[1] <= (K.TW + 1) * (2 * K.TH + 1)] + [(32768, 1)]


def test_the_fault_free_model_is_the_reference():
    for case in K.cases(QUICK + [(2 * K.TW + 1, 2 * K.TH + 1)]):
        assert not differs(case, None, {}), case
    for case in [(257, 300, "random59", "none"), (257, 300, "spiral", "random10"), (32768, 2, "serpentine", "none"), (1, 32768, "all", "seam")]:
        assert not differs(case, None, {}), case
    # and in the mask form
    for case in K.cases([(K.TW + 1, K.TH + 1)]):
        if case[2] in K.BINARY:
            for c in (4, 8):
                got = store(*parents(None, K.mask_form(case), c, None), (case[1], case[0]), K.DENSE, 2, True, None)
                want = K.expected(case, c, K.DENSE, 2, "mask")
                assert got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (case, c)


@pytest.mark.parametrize("fault", FAULTS)
def test_every_modelled_mistake_changes_a_case(fault):
    """the first case that shows it is named; the small shapes come first, so the search is short"""
    shapes = [(2 * K.TW + 1, 2 * K.TH + 1), (K.TW + 1, K.TH + 1), (K.TW + 1, 2 * K.TH + 1)] + QUICK
    for case in K.cases(shapes):
        if differs(case, fault, {}):
            return
    pytest.fail(f"no case of tests/regions_cases.py shows '{fault}'")
