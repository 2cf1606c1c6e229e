"""The rule of ec_focal_rank / ec_focal_majority (include/erased_cells.h) restated in numpy, for the tests to compare the kernels with.

Per output cell the taps of its footprint are gathered — shifted views of the raster padded by the radius, tap k = dy * (2 rx + 1) + dx
of every output cell at once, a cell outside the raster or under a cleared mask byte being no tap — and stable-sorted by the
reference's total order, the taps first; `focal_rank` keeps the one at position r(count), r in Python's integer arithmetic, and
`focal_majority` counts, for every tap, the taps of the same key, and keeps the least key of the greatest count.  It knows no networks,
buckets, sentinels or tiles.  `ordered(a, mask, rx, ry)` is the expensive half, shared by the calls that differ only in (num, den,
method, whole).

Imports nothing from the library.  tests/test_focal_rank_ref.py holds this file to independent answers.
"""
import numpy as np

LOWER, UPPER = 0, 1
MAX_TAPS, MAX_DEN = 64, 65535
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def words(a):
    """the cells' bits, zero-extended to 64"""
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize]).astype(np.uint64)


def order_key(a):
    """uint64 keys whose unsigned order is the reference's total order of the cells (src/value.rs:248-265): integers natural, floats
    by total_cmp (-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN).  A bijection on the cell's bits."""
    a = np.asarray(a)
    w = words(a)
    width = 8 * a.dtype.itemsize
    top = np.uint64(1 << (width - 1))
    ones = np.uint64((1 << width) - 1)
    if a.dtype.kind == "f":
        return np.where(w & top != 0, ~w & ones, w | top)
    if a.dtype.kind == "i":
        return w ^ top
    return w


def position(num, den, method, c):
    """r of the header for c >= 1 taps"""
    assert 1 <= den <= MAX_DEN and 0 <= num <= den and method in (LOWER, UPPER) and c >= 1
    return (num * (c - 1)) // den if method == LOWER else (num * (c - 1) + den - 1) // den


def gather(a, mask, rx, ry):
    """(bits[K, rows, cols], key[K, rows, cols], tap[K, rows, cols]) for the K = (2 ry + 1)(2 rx + 1) footprint positions, row-major"""
    a = np.asarray(a)
    rows, cols = a.shape
    assert (2 * rx + 1) * (2 * ry + 1) <= MAX_TAPS
    pb = np.zeros((rows + 2 * ry, cols + 2 * rx), np.uint64)
    pk = np.zeros(pb.shape, np.uint64)
    pt = np.zeros(pb.shape, bool)
    pb[ry:ry + rows, rx:rx + cols] = words(a)
    pk[ry:ry + rows, rx:rx + cols] = order_key(a)
    pt[ry:ry + rows, rx:rx + cols] = True if mask is None else (np.asarray(mask).reshape(rows, cols) != 0)
    views = [(dy, dx) for dy in range(2 * ry + 1) for dx in range(2 * rx + 1)]
    cut = lambda p: np.stack([p[dy:dy + rows, dx:dx + cols] for dy, dx in views])
    return cut(pb), cut(pk), cut(pt)


def ordered(a, mask, rx, ry):
    """(bits, key, count): bits and keys of every cell's footprint in the rule's order — the count taps first, ascending by key — and
    the tap count.  Two stable sorts: by key, then by "no tap"."""
    bits, key, tap = gather(a, mask, rx, ry)
    first = np.argsort(key, axis=0, kind="stable")
    no_tap = ~np.take_along_axis(tap, first, axis=0)
    order = np.take_along_axis(first, np.argsort(no_tap, axis=0, kind="stable"), axis=0)
    return np.take_along_axis(bits, order, axis=0), np.take_along_axis(key, order, axis=0), tap.sum(axis=0)


def _finish(picked, count, full, whole, dtype):
    valid = (count == full) if whole else (count > 0)
    out = np.where(valid, picked, np.uint64(0)).astype(UINT[np.dtype(dtype).itemsize]).view(dtype)   # an invalid cell: all-zero bits
    return out, valid.astype(np.uint8)


def pick(od, num, den, method, whole, dtype):
    bits, _, count = od
    table = np.array([0] + [position(num, den, method, c) for c in range(1, MAX_TAPS + 1)], np.int64)
    r = table[count]
    return _finish(np.take_along_axis(bits, r[None], axis=0)[0], count, bits.shape[0], whole, dtype)


def focal_rank(a, mask, rx, ry, num, den, method, whole=False):
    """-> (rows x cols cells of a's type, rows x cols mask bytes)"""
    a = np.asarray(a)
    return pick(ordered(a, mask, rx, ry), num, den, method, whole, a.dtype)


def majority_pick(od, whole, dtype):
    bits, key, count = od
    k = bits.shape[0]
    is_tap = np.arange(k).reshape(k, 1, 1) < count[None]
    freq = np.zeros(key.shape, np.int64)
    for j in range(k):                                 # how many taps hold the key of the tap at position p
        freq += (key == key[j][None]) & is_tap[j][None]
    freq = np.where(is_tap, freq, 0)
    best = np.argmax(freq, axis=0)                     # the first position of the greatest count: the least key, the order being ascending
    return _finish(np.take_along_axis(bits, best[None], axis=0)[0], count, k, whole, dtype)


def focal_majority(a, mask, rx, ry, whole=False):
    """-> (rows x cols cells of a's type, rows x cols mask bytes)"""
    a = np.asarray(a)
    return majority_pick(ordered(a, mask, rx, ry), whole, a.dtype)
