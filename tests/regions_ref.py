"""The reference of ec_regions (include/erased_cells.h): a flood fill from every unvisited valid cell in raster order.

The cell a fill starts from is the least row-major index of its region — the rule's ROOT — and the fills start in increasing
order of root, which is the order of the DENSE numbers: both numberings come out by construction.  Sizes are the fills' cell counts,
the sieve keeps `size >= min_cells`, and the mask form (cells None) takes every valid cell as equal to every other.  Nothing here
knows of tiles, seams, parents or scans: it shares no step with the kernels.

Plain Python and numpy; imports nothing from the library.  tests/test_regions_ref.py holds it to independent answers."""
import numpy as np

ROOT, DENSE = 0, 1         # EC_REGIONS_ROOT, EC_REGIONS_DENSE
MAX_SIDE = 32768           # EC_REGIONS_MAX_SIDE
BUDGET = 120_000           # cells one fill-all may visit: the cases are chosen within it
UNWRITTEN = 0xA5           # what the GPU tests pre-fill their outputs with


def bits(cells):
    """the cells' bits as uint64: equality of cells is equality of these"""
    a = np.ascontiguousarray(cells)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).astype(np.uint64)


def fill(cells, valid, connectivity):
    """(root, size): for every cell of a 2-D raster the root of its region (-1: not valid) and that region's size (0: not valid).
    cells: a 2-D array of any cell type, or None (the mask form); valid: a 2-D array, nonzero = valid, or None (all valid)."""
    assert connectivity in (4, 8) and (cells is not None or valid is not None)
    shape = np.shape(cells if cells is not None else valid)
    rows, cols = shape
    assert len(shape) == 2 and 1 <= rows <= MAX_SIDE and 1 <= cols <= MAX_SIDE and rows * cols <= BUDGET
    n = rows * cols
    key = bits(cells).ravel().tolist() if cells is not None else [0] * n
    ok = (np.asarray(valid).ravel() != 0).tolist() if valid is not None else [True] * n
    steps = [(0, -1), (0, 1), (-1, 0), (1, 0)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    root, size = [-1] * n, [0] * n
    for start in range(n):
        if not ok[start] or root[start] >= 0:
            continue
        root[start] = start
        region, k = [start], key[start]
        for i in region:                       # the list grows while it is walked
            y, x = divmod(i, cols)
            for dy, dx in steps:
                yy, xx = y + dy, x + dx
                if 0 <= yy < rows and 0 <= xx < cols:       # the raster does not wrap
                    j = yy * cols + xx
                    if ok[j] and root[j] < 0 and key[j] == k:
                        root[j] = start
                        region.append(j)
        for i in region:
            size[i] = len(region)
    return np.array(root, np.int64).reshape(rows, cols), np.array(size, np.int64).reshape(rows, cols)


def finish(root, size, numbering=DENSE, min_cells=0, dst_mask=True):
    """(labels as int32, mask bytes, K) as ec_regions stores them, from fill()'s answer.  dst_mask False: the call without validity
    bytes — the labels are the same (zero bits at every cell without a kept region), the mask comes back None."""
    assert numbering in (ROOT, DENSE) and 0 <= min_cells < 1 << 64
    kept = (root >= 0) & (size >= min_cells)
    roots = np.unique(root[kept])                      # ascending: the order of the dense numbers
    if numbering == ROOT:
        labels = np.where(kept, root + 1, 0)
    else:
        labels = np.where(kept, np.searchsorted(roots, np.where(kept, root, 0)) + 1, 0)
    assert labels.min() >= 0 and labels.max() < 2 ** 31
    return labels.astype(np.int32), (kept.astype(np.uint8) if dst_mask else None), int(roots.size)


def regions(cells, valid, connectivity=4, numbering=DENSE, min_cells=0, dst_mask=True):
    return finish(*fill(cells, valid, connectivity), numbering, min_cells, dst_mask)
