"""The inputs and shapes that the GPU tests of ec_focal_rank / ec_focal_majority run (tests/test_gpu_focal_rank.py,
test_gpu_focal_rank_bounds.py, test_gpu_focal_rank_python.py), shared with tests/test_focal_rank_faults.py, which shows without a GPU
that these very inputs expose each modelled mistake of the kernel.

Plain numpy; imports nothing from the library.  TW x TH is the output tile of the kernels (csrc/ec_focal_kernels.hpp;
tests/test_focal_rank_args.py checks that the two files agree).  Shapes come from focal_cases.axis_values per axis: below, at and above
the radius, the footprint and the tile.
"""
from collections import Counter

import numpy as np

import focal_cases as K
from focal_cases import MASK_KINDS, NP_DTYPES, TH, TW, UINT, hashed_bytes, hashed_u64, mask_bytes, shapes  # noqa: F401

MAX_TAPS = 64
# (rx, ry): every bucket of the sorting network — 1, 3 -> 4, 5 -> 8, 9 and 15 -> 16, 21 and 25 -> 32, 45, 49 and 63 -> 64 taps — the
# widest and the tallest footprints, and footprints that are not square in both directions
RADII = [(0, 0), (1, 0), (0, 2), (1, 1), (2, 1), (1, 3), (2, 2), (3, 3), (3, 4), (4, 3), (7, 0), (0, 7), (7, 1), (1, 7)]
REFUSED_RADII = [(4, 4), (7, 2), (2, 7), (7, 7), (3, 5)]   # 81, 75, 75, 225 and 77 taps
LOWER, UPPER = 0, 1
# (num, den, method): the two ends, both medians and a high quantile rounded up
QS = [(0, 1, LOWER), (1, 2, LOWER), (1, 2, UPPER), (9, 10, UPPER), (1, 1, LOWER)]
WORD_FORM_TYPES = (0, 5, 8, 9)   # u8, i16, f32, f64: a 1- and a 2-byte cell (32-bit words), a 4-byte cell (64-bit words), an 8-byte cell (pairs)
F32, F64, U64, I64 = 8, 9, 3, 7


def taps(radius):
    return (2 * radius[0] + 1) * (2 * radius[1] + 1)


def bucket(radius):
    """the tap count rounded up to a power of two: the network that sorts the footprint (focal_rank_bucket of ec_focal_rank_cell.hpp)"""
    b = 1
    while b < taps(radius):
        b *= 2
    return b


assert all(taps(r) <= MAX_TAPS for r in RADII) and all(taps(r) > MAX_TAPS for r in REFUSED_RADII)
assert {bucket(r) for r in RADII} == {1, 4, 8, 16, 32, 64}
assert {(0, 0), (1, 1), (2, 1), (1, 3), (3, 3), (3, 4), (4, 3), (7, 0), (0, 7), (7, 1), (1, 7)} <= set(RADII)


def extremes(ct):
    """bit patterns at the two ends of the total order of cell type ct: for a u64 the maximum, for floats the all-ones NaNs of both
    signs — what a sentinel has to sort above — and the type's least cell"""
    dt = NP_DTYPES[ct]
    u = UINT[dt.itemsize]
    ones = (1 << (8 * dt.itemsize)) - 1
    if dt.kind == "f":
        pats = [ones >> 1, ones]                                     # +NaN with every payload bit set (the greatest key), its negative (the least)
    elif dt.kind == "u":
        pats = [ones, 0]
    else:
        pats = [ones >> 1, (ones >> 1) + 1]                          # the maximum and the minimum
    return np.array(pats, dtype=u).view(dt)


def rank_raster(ct, cols, rows, seed, raw=False):
    """focal_cases.raster_cells with the extremes of the type planted: about every ninth cell is the greatest or the least cell of
    the total order, so they meet raster edges, tile seams and masked-out neighbours.  1-byte cells tie everywhere by themselves."""
    a = K.raster_cells(ct, cols, rows, seed, raw).copy()
    h = hashed_u64(cols * rows, seed ^ 0xE17).reshape(rows, cols)
    ex = extremes(ct)
    a[h % np.uint64(9) == 0] = ex[0]
    a[h % np.uint64(23) == 1] = ex[1]
    if a.dtype.kind == "f" and a.size > 3:                            # both zeros side by side, whatever was planted there
        a.reshape(-1)[a.size // 2 - 1:a.size // 2 + 1] = (0.0, -0.0)
    return a


def palette(ct):
    """the classes of a class raster of cell type ct.  Floats: -0.0 beside 0.0 and two NaNs that differ in their payload only — four
    different keys — and the all-ones NaN; integers: 0, 1 and the ends of the type."""
    dt = NP_DTYPES[ct]
    u = UINT[dt.itemsize]
    if dt.kind == "f":
        one_nan = np.array([np.nan], dtype=dt).view(u)[0]
        pats = np.array([np.array([-0.0], dt).view(u)[0], 0, one_nan, one_nan | u(1), extremes(ct).view(u)[0]], dtype=u)
        return pats.view(dt)
    return np.concatenate([np.array([0, 1, 7], dtype=dt), extremes(ct)])


def class_raster(ct, cols, rows, seed):
    """a classified raster: patches of one class about 4 x 3 cells large with every sixth cell a hashed other class, so footprints with
    a strict majority, with a tie for the greatest frequency and with no repeated class at all occur"""
    pal = palette(ct)
    h = hashed_u64(cols * rows, seed ^ 0xC1A5).reshape(rows, cols)
    y, x = np.mgrid[0:rows, 0:cols]
    patch = (y // 3 * 2 + x // 4 + (seed & 3)) % len(pal)
    idx = np.where(h % np.uint64(6) == 0, (h >> np.uint64(8)) % np.uint64(len(pal)), patch.astype(np.uint64)).astype(np.int64)
    return pal[idx]


def _check_class_rasters():
    """what the docstrings promise, counted with collections.Counter on a small raster of every cell type"""
    for ct in range(10):
        a = class_raster(ct, 23, 11, 0x77 + ct)
        bits = a.view(UINT[a.dtype.itemsize])
        strict = tie = 0
        for i in range(1, a.shape[0] - 1):
            for j in range(1, a.shape[1] - 1):
                top = Counter(bits[i - 1:i + 2, j - 1:j + 2].ravel().tolist()).most_common(2)
                strict += top[0][1] >= 5
                tie += len(top) == 2 and top[0][1] == top[1][1]
        assert strict > 10 and tie > 3, (ct, strict, tie)
        if a.dtype.kind == "f":
            flat = a.ravel()
            zeros = (flat == 0)
            sign = np.signbit(flat)
            beside = zeros[:-1] & zeros[1:] & (sign[:-1] != sign[1:])
            assert beside.any(), ct                                       # -0.0 beside 0.0
            assert len(set(bits.ravel()[np.isnan(flat)].tolist())) >= 3, ct   # NaNs that differ in their payload only


_check_class_rasters()


def sources(ct, kind, cols, rows, raw=False):
    """(rank raster, class raster, mask or None) of one case of tests/test_gpu_focal_rank.py: cell type, mask kind (None: no mask), shape"""
    seed = 0xF0CA + 131 * ct + cols + 1000 * rows
    m = mask_bytes(kind, cols, rows, 0x5EED + cols + 7 * rows) if kind is not None else None
    return rank_raster(ct, cols, rows, seed, raw), class_raster(ct, cols, rows, seed + 1), m


def impulse_positions(cols, rows):
    return K.impulse_positions(cols, rows)
