"""The inputs that the GPU tests of ec_regions run (tests/test_gpu_regions.py, test_gpu_regions_bounds.py,
test_gpu_regions_python.py), shared with tests/test_regions_faults.py, which shows without a GPU that these very inputs expose each
modelled mistake of the kernels.

Plain numpy; imports nothing from the library.  The kernels' constants are restated here (csrc/ec_regions_cell.hpp;
tests/test_regions_args.py checks that the two files agree): TW x TH the tile one workgroup labels in LDS, SCAN the cells of one block
of the reduce-then-scan that numbers the roots.

A case is (cols, rows, pattern, mask): `cells(cols, rows, pattern)` gives its class raster, `valid(cols, rows, mask)` its validity
bytes or None.  The patterns in BINARY have the classes 0 and 1 and also run in the MASK FORM, where the cells are the validity:
`mask_form(case)`.  Every case is within the budget of the flood fill (regions_ref.BUDGET cells); the largest rasters run a choice of
the patterns, the ones whose regions are long.
"""
import functools

import numpy as np

import regions_ref as R

TW = 32        # kRegTileW
TH = 32        # kRegTileH
SCAN = 2048    # kRegScanCells
ROOT, DENSE = R.ROOT, R.DENSE

SIZES_W = sorted({1, TW - 1, TW, TW + 1, 2 * TW + 1})
SIZES_H = sorted({1, TH - 1, TH, TH + 1, 2 * TH + 1})
# (cols, rows)
LINES = [(1, 1)] + [(n, 1) for n in SIZES_W if n > 1] + [(1, n) for n in SIZES_H if n > 1]
SQUARES = [(w, h) for w, h in zip(SIZES_W, SIZES_H) if w > 1]
OBLONGS = [(TW + 1, 2 * TH + 1), (2 * TW + 1, TH - 1), (TW, 3), (3, TH + 1), (2 * TW, TH), (TW - 1, TH + 1)]
SMALL = LINES + SQUARES + OBLONGS
BIG = [(257, 300)]
LONG = [(32768, 1), (1, 32768), (32768, 2)]      # 1024 tiles in a row: the longest chain of seams a raster can have
SHAPES = SMALL + BIG + LONG

BINARY = ("all", "none", "checkerboard", "random30", "random59", "random80", "serpentine", "spiral", "comb-last-row", "comb-last-column",
          "diagonal-stripes", "anti-diagonal-stripes")
PATTERNS = BINARY + ("rings", "random3", "wide2", "wide4", "wide8", "float-specials")
MASKS = ("none", "random10", "seam")


def hashed(n, seed):
    """n reproducible uint64 (splitmix64 of seed + index)"""
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _random(cols, rows, per_cent, seed):
    return (hashed(cols * rows, seed) % np.uint64(100) < np.uint64(per_cent)).reshape(rows, cols)


def _spiral(cols, rows):
    """one path of width 1 from (0, 0) inwards, a gap of one cell between its turns: its root is in tile 0 and it crosses every seam"""
    m = np.zeros((rows, cols), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    free = lambda a, b: not (0 <= a < rows and 0 <= b < cols) or not m[a, b]
    while True:
        moved = False
        while 0 <= y + dy < rows and 0 <= x + dx < cols and not m[y + dy, x + dx] and free(y + 2 * dy, x + 2 * dx):
            y, x, moved = y + dy, x + dx, True
            m[y, x] = True
        if not moved:
            return m
        dy, dx = dx, -dy


def _pattern(cols, rows, name):
    y, x = np.mgrid[0:rows, 0:cols]
    if name == "all":
        return np.ones((rows, cols), bool)
    if name == "none":
        return np.zeros((rows, cols), bool)
    if name == "checkerboard":                 # n regions under 4, two under 8
        return (x + y) % 2 == 0
    if name == "random30":
        return _random(cols, rows, 30, 0x5E30)
    if name == "random59":                     # the percolation threshold: tortuous clusters that span many tiles
        return _random(cols, rows, 59, 0x5E59)
    if name == "random80":
        return _random(cols, rows, 80, 0x5E80)
    if name == "serpentine":                   # every other row, joined at alternating ends: one region through every seam, root in tile 0
        return (y % 2 == 0) | (x == np.where((y // 2) % 2 == 0, cols - 1, 0))
    if name == "spiral":
        return _spiral(cols, rows)
    if name == "comb-last-row":                # teeth that meet only in the last row: the root is learned last
        return (x % 2 == 0) | (y == rows - 1)
    if name == "comb-last-column":
        return (y % 2 == 0) | (x == cols - 1)
    if name == "diagonal-stripes":             # lines under 8, single cells under 4
        return (x - y) % 3 == 0
    if name == "anti-diagonal-stripes":
        return (x + y) % 3 == 0
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def cells(cols, rows, pattern):
    """the class raster of a case, (rows, cols), read-only"""
    n = cols * rows
    if pattern in BINARY:
        out = _pattern(cols, rows, pattern).astype(np.uint8)
    elif pattern == "rings":                   # concentric rings of alternating class
        y, x = np.mgrid[0:rows, 0:cols]
        out = (np.maximum(abs(y - rows // 2), abs(x - cols // 2)) % 2).astype(np.uint8)
    elif pattern == "random3":
        out = (hashed(n, 0xC1A5) % np.uint64(3)).astype(np.uint8).reshape(rows, cols)
    elif pattern in ("wide2", "wide4", "wide8"):   # three classes that differ only in the cell's top byte
        dt = {"wide2": np.uint16, "wide4": np.uint32, "wide8": np.uint64}[pattern]
        top = 8 * (np.dtype(dt).itemsize - 1)
        out = ((hashed(n, 0x70B0) % np.uint64(3)) << np.uint64(top) | np.uint64(0x34)).astype(dt).reshape(rows, cols)
    elif pattern == "float-specials":          # f32: +0.0 and -0.0 are different classes, a NaN equals only the NaN of the same payload
        table = np.array([0x00000000, 0x80000000, 0x7FC00000, 0x7FC00001, 0x3F800000], np.uint32).view(np.float32)
        out = table[(hashed(n, 0xF10A) % np.uint64(5)).astype(np.intp)].reshape(rows, cols)
    else:
        raise KeyError(pattern)
    assert out.shape == (rows, cols)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def valid(cols, rows, mask):
    """the validity bytes of a case, (rows, cols) uint8 and read-only, or None: a valid cell is any nonzero byte, so they are 1, 2, 0x80
    and 0xFF"""
    if mask == "none":
        return None
    if mask == "random10":
        ok = ~_random(cols, rows, 10, 0x1A5C)
    elif mask == "seam":                       # one invalid column and row exactly on a seam: the last of the first tile
        y, x = np.mgrid[0:rows, 0:cols]
        ok = (x != TW - 1) & (y != TH - 1)
    else:
        raise KeyError(mask)
    values = np.array([1, 2, 0x80, 0xFF], np.uint8)[(hashed(cols * rows, 0xB17E) % np.uint64(4)).astype(np.intp)].reshape(rows, cols)
    out = np.where(ok, values, 0).astype(np.uint8)
    out.setflags(write=False)
    return out


def patterns_of(shape):
    if shape in BIG:
        return ["all", "random59", "serpentine", "spiral", "comb-last-row", "comb-last-column", "rings", "random3", "wide8"]
    if shape in LONG:
        return ["all", "checkerboard", "random59", "serpentine", "random3"]
    return list(PATTERNS)


def cases(shapes=None):
    """every (shape, pattern) without a mask and with one of the two masks, taken in turn"""
    out = []
    for s, (c, r) in enumerate(SHAPES if shapes is None else shapes):
        for p, pattern in enumerate(patterns_of((c, r))):
            out += [(c, r, pattern, "none"), (c, r, pattern, MASKS[1 + (s + p) % 2])]
    return out


def mask_form(case):
    """the mask of a binary case in the mask form (src NULL): set where the pattern is and the case's mask allows it"""
    cols, rows, pattern, mask = case
    assert pattern in BINARY
    v = valid(cols, rows, mask)
    out = np.where(cells(cols, rows, pattern) != 0, np.uint8(1) if v is None else v, 0).astype(np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def filled(case, connectivity, form="cells"):
    """the reference's (root, size) of a case: computed once, shared, read-only"""
    cols, rows, pattern, mask = case
    if form == "mask":
        root, size = R.fill(None, mask_form(case), connectivity)
    else:
        root, size = R.fill(cells(cols, rows, pattern), valid(cols, rows, mask), connectivity)
    root.setflags(write=False)
    size.setflags(write=False)
    return root, size


def expected(case, connectivity, numbering, min_cells, form="cells", dst_mask=True):
    return R.finish(*filled(case, connectivity, form), numbering, min_cells, dst_mask)


def sieves(case):
    """min_cells of a case: everything, 2, 5, and a value above the largest region"""
    return [0, 2, 5, case[0] * case[1] + 1]
