"""The reference of ec_distance (include/erased_cells.h): brute force in exact integers.

    d2(i, j) = min over targets (y, x) of (i - y)^2 + (j - x)^2        a target: mask[y, x] != 0

taken over ALL targets for every cell, in chunks of cells (int64 throughout: no rounding anywhere), with the validity and output
rules of the header on top.  Nothing here knows of columns, rows, parabolas or stacks: it shares no step with the kernels.

Plain numpy; imports nothing from the library.  tests/test_distance_ref.py holds it to independent answers."""
import numpy as np

U32, F64 = 2, 9            # EC_U32, EC_F64
UNLIMITED = 0xFFFFFFFF     # EC_DISTANCE_UNLIMITED
MAX_SIDE = 32768           # EC_DISTANCE_MAX_SIDE
BUDGET = 6 * 10 ** 8       # cells x targets one call may compare: the cases are chosen within it
CHUNK = 1 << 22            # cells x targets compared at a time


def squared(mask):
    """(d2, any): the int64 squared distances of a 2-D mask (all -1 without a target), and whether it has a target"""
    m = np.asarray(mask)
    assert m.ndim == 2 and 1 <= m.shape[0] <= MAX_SIDE and 1 <= m.shape[1] <= MAX_SIDE
    rows, cols = m.shape
    ty, tx = np.nonzero(m)
    if ty.size == 0:
        return np.full((rows, cols), -1, np.int64), False
    assert rows * cols * ty.size <= BUDGET, f"{cols} x {rows} cells against {ty.size} targets is beyond the brute force's budget"
    ty, tx = ty.astype(np.int64), tx.astype(np.int64)
    cells = np.arange(rows * cols, dtype=np.int64)
    out = np.empty(rows * cols, np.int64)
    step = max(1, CHUNK // ty.size)
    for at in range(0, cells.size, step):
        c = cells[at:at + step]
        i, j = c // cols, c % cols
        out[at:at + step] = ((i[:, None] - ty[None, :]) ** 2 + (j[:, None] - tx[None, :]) ** 2).min(axis=1)
    return out.reshape(rows, cols), True


def finish(d2, any_target, max_sq=UNLIMITED, out_type=F64):
    """(cells, mask bytes) as ec_distance stores them, from squared()'s answer: a cell is valid iff a target exists and
    d2 <= max_sq; a valid cell holds d2 as a u32 or its correctly rounded f64 square root, an invalid one zero bits"""
    assert out_type in (U32, F64) and 0 <= max_sq <= UNLIMITED
    valid = (d2 <= max_sq) if any_target else np.zeros(d2.shape, bool)
    kept = np.where(valid, d2, 0)
    assert kept.min() >= 0 and kept.max() < 2 ** 31
    cells = kept.astype(np.uint32) if out_type == U32 else np.sqrt(kept.astype(np.float64))   # IEEE sqrt: correctly rounded
    return cells, valid.astype(np.uint8)


def distance(mask, max_sq=UNLIMITED, out_type=F64):
    return finish(*squared(mask), max_sq, out_type)
