"""The inputs that the GPU tests of ec_distance run (tests/test_gpu_distance.py, test_gpu_distance_bounds.py,
test_gpu_distance_python.py), shared with tests/test_distance_faults.py, which shows without a GPU that these very inputs expose each
modelled mistake of the kernels.

Plain numpy; imports nothing from the library.  The kernels' constants are restated here (csrc/ec_distance_line.hpp;
tests/test_distance_args.py checks that the two files agree): W lines per wave, T the side of the staging tiles, CHUNK the rows a
column sweep loads together.

A case is (shape, pattern): `mask(cols, rows, pattern)` gives its bytes.  Every case is within the budget of the brute-force
reference (distance_ref.BUDGET); the dense patterns are therefore left off the largest rasters, where the sparse ones give the long
chains and the large distances those rasters are there for.
"""
import functools

import numpy as np

import distance_ref as R

W = 64        # kDistLines
T = 64        # kDistTile
CHUNK = 8     # kDistChunk
INF = 0xFFFF  # kDistInf
UNLIMITED = R.UNLIMITED

SIZES = sorted({1, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T + 1})
# (cols, rows)
LINES = [(1, 1)] + [(n, 1) for n in SIZES if n > 1] + [(1, n) for n in SIZES if n > 1]
SQUARES = [(n, n) for n in SIZES if n > 1]
OBLONGS = [(T + 1, 2 * W + 3), (2 * W + 3, T + 1), (2 * T + 1, W - 1), (W - 1, 2 * T + 1), (T, 3), (3, T + 1), (CHUNK + 1, 2 * CHUNK + 1)]
SMALL = LINES + SQUARES + OBLONGS                      # everything up to 2T + 1 a side (and 2W + 3)
BIG = [(257, 300)]
LONG = [(32768, 1), (1, 32768), (32768, 2)]            # the full chain length and the largest d2 on one axis; the far corner
SHAPES = SMALL + BIG + LONG

DENSE = ("all", "checkerboard", "random50")


def hashed(n, seed):
    """n reproducible uint64 (splitmix64 of seed + index)"""
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _random(cols, rows, per_million, seed):
    return (hashed(cols * rows, seed) % np.uint64(1000000) < np.uint64(per_million)).reshape(rows, cols)


def _single(cols, rows, y, x):
    m = np.zeros((rows, cols), bool)
    m[min(max(y, 0), rows - 1), min(max(x, 0), cols - 1)] = True
    return m


def _pattern(cols, rows, name):
    y, x = np.mgrid[0:rows, 0:cols]
    if name == "none":
        return np.zeros((rows, cols), bool)
    if name == "all":
        return np.ones((rows, cols), bool)
    if name == "corner00":
        return _single(cols, rows, 0, 0)
    if name == "corner01":
        return _single(cols, rows, 0, cols - 1)
    if name == "corner10":
        return _single(cols, rows, rows - 1, 0)
    if name == "corner11":
        return _single(cols, rows, rows - 1, cols - 1)
    if name == "centre":
        return _single(cols, rows, rows // 2, cols // 2)
    if name == "edge-left":        # the last column of the first tile, the last row of the first wave
        return _single(cols, rows, W - 1, T - 1)
    if name == "edge-right":       # the first column of the second tile, the first row of the second wave
        return _single(cols, rows, W, T)
    if name == "full-row":
        return y == rows // 3
    if name == "full-column":
        return x == (2 * cols) // 3
    if name == "last-column-one":  # every other column has no target: g is INF there
        return _single(cols, rows, rows // 2, cols - 1)
    if name == "checkerboard":
        return (x + y) % 2 == 0
    if name == "diagonal":
        return x * rows // cols == y if cols >= rows else y * cols // rows == x
    if name == "decreasing-g":     # in row 0 g falls steeply from left to right (3 a column): a new parabola there pops the earlier ones
        return (y == rows - 1 - 3 * x) | ((x == cols - 1) & (y == 0))
    if name == "constant-g":       # one row of targets at the bottom: g is constant along every row, every parabola is kept
        return y == rows - 1
    if name == "random50":
        return _random(cols, rows, 500000, 0xD150)
    if name == "random1":
        return _random(cols, rows, 10000, 0xD101)
    if name == "random001":
        return _random(cols, rows, 100, 0xD001)
    raise KeyError(name)


PATTERNS = ["none", "all", "corner00", "corner01", "corner10", "corner11", "centre", "edge-left", "edge-right", "full-row", "full-column",
            "last-column-one", "checkerboard", "diagonal", "decreasing-g", "constant-g", "random50", "random1", "random001"]


def patterns_of(shape):
    """the patterns run at `shape`: all of them up to 2T + 1 a side; the largest rasters without the dense ones (the reference's
    budget), the long lines also without the ones that put a target into every column"""
    if shape in BIG:
        return [p for p in PATTERNS if p not in DENSE]
    if shape in LONG:
        return ["none", "corner00", "corner11", "centre", "last-column-one", "random1", "random001"]
    return PATTERNS


@functools.lru_cache(maxsize=None)
def mask(cols, rows, pattern):
    """the mask bytes of a case, (rows, cols) uint8, read-only: a target is any nonzero byte, so they are 1, 2, 0x80 and 0xFF"""
    m = _pattern(cols, rows, pattern)
    assert m.shape == (rows, cols)
    values = np.array([1, 2, 0x80, 0xFF], np.uint8)[(hashed(cols * rows, 0xB17E) % np.uint64(4)).astype(np.intp)].reshape(rows, cols)
    out = np.where(m, values, 0).astype(np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def squared(cols, rows, pattern):
    """the reference's (d2, any) of a case: computed once, shared, read-only"""
    d2, any_target = R.squared(mask(cols, rows, pattern))
    d2.setflags(write=False)
    return d2, any_target


def expected(cols, rows, pattern, max_sq=UNLIMITED, out_type=R.F64):
    return R.finish(*squared(cols, rows, pattern), max_sq, out_type)


def cases(shapes=None):
    return [(c, r, p) for (c, r) in (SHAPES if shapes is None else shapes) for p in patterns_of((c, r))]


def limits(cols, rows, pattern):
    """max_sq values of a case: 0, 1, 2, a value that occurs, that value - 1, and no limit"""
    d2, _ = squared(cols, rows, pattern)
    occurs = int(np.median(d2[d2 > 0])) if (d2 > 0).any() else 5
    nearest = d2[d2 >= occurs].min() if (d2 >= occurs).any() else occurs
    return [0, 1, 2, int(nearest), int(nearest) - 1, UNLIMITED]
