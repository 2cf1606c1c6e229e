"""The shapes, the spots and the closed forms of tests/test_gpu_large_rasters.py: rasters past 2^32 cells, past 2^31 and 2^32 bytes of
output, at 2^24 workgroups in one launch and at ec_distance's documented maximum — and the mistakes such sizes expose, restated over
the spots so that tests/test_large_cases.py can show, without a GPU, that the spots see each of them.

Nothing here comes from the library: plain Python and numpy over indices.

The mistakes modelled, each as "which source cell does the kernel really read for cell i" or "which cells does the launch write":
  cell index mod 2^32 (loads / stores); byte offset mod 2^32 and mod 2^31; y * cols formed in 32 bits; tiles numbered 2^24 and above
  never run; the grid taken mod 2^24; a launch that runs only the first 2^24 - 1 workgroups.
The one-workgroup-per-tile kernels number their tiles from both ends (even workgroups from the front, odd ones from the back), so a
launch cut short loses tiles in the MIDDLE of the raster; the boundary spots therefore cover the middle as well as both ends, and
the tile models are stated for both numberings."""
import math

import numpy as np

TWO24, TWO31, TWO32 = 1 << 24, 1 << 31, 1 << 32
BLOCK = 256                                  # lanes per workgroup: a dispatch holds at most (2^32 - 1) // 256 of them

# ---- the hashed input streams: name -> (cell type 0 = u8 / 1 = u16, seed, lo, hi) of ec_synth_fill / oracle.eco.fill_u8 / fill_u16.
# Mask streams are u8 cells 0 / 1.  The seeds are chosen (tests/test_large_cases.py asserts it) so that at least half of the spot cells
# past a boundary differ from the cell 2^32 places earlier — for a 0 / 1 stream that is a property of the seed, not a certainty.
STREAMS = {
    "a": (0, 0x1A26E001, 1, 200), "a2": (0, 0x1A26E002, 1, 200), "b": (1, 0x1A26E003, 1, 400),
    "ma": (0, 0x21001A26E011, 0, 1), "mb": (0, 0x29001A26E011, 0, 1), "msel": (0, 0x2A001A26E011, 0, 1),
    "zones": (0, 0x1A26E021, 0, 5), "classes": (0, 0x1A26E022, 0, 3), "wide": (1, 0x1A26E023, 0, 60000),
}

# ---- 1-D families: more than 2^32 cells ------------------------------------------------------------------------------------------
SIDE = 65537
N = SIDE * SIDE                              # 4 295 098 369 = 2^32 + 131 073, odd
SPOT = 100003
SHORT = 4099                                 # a pure-Python reference may use spots this short


def spots(n=N, length=SPOT):
    """(offset, cells): the start, a stretch that straddles cell 2^32, the last 5 cells before it with what follows, the tail"""
    if length >= 70000:
        offs = [0, TWO32 - 70000, TWO32 - 5, n - length]
    else:
        offs = [0, TWO32 - length // 2, TWO32 - 5, n - length]
    return [(o, min(length, n - o)) for o in offs]


def short_spots(n=N):
    return spots(n, SHORT)


# the f64 byte-offset case: byte 2^31 of the output is cell 2^28, byte 2^32 is cell 2^29
N_F64 = (1 << 29) + 4101


def f64_spots(n=N_F64, length=SHORT):
    return [(0, length), ((1 << 28) - length // 2, length), ((1 << 29) - length // 2, length), (n - length, length)]


def blocks(n, length=SHORT):
    """the three hashed blocks planted into a constant raster for the reductions: at 0, over cell 2^32 - 1, at the tail (the last two are one
    block when n == 2^32)"""
    out = [(0, length)]
    mid = TWO32 - 1 - length // 2
    out.append((mid, min(length, n - mid)))
    if n - length >= mid + out[1][1]:
        out.append((n - length, length))
    return out


# ---- 2-D families: 65537 x 65537 ----------------------------------------------------------------------------------------------------
WIN_ROWS, WIN_COLS = 40, 200
WRAP_ROW = 65535                             # 65535 * 65537 = 2^32 - 1: row 65535 is the first whose cells pass 2^32


def windows(cols=SIDE, rows=SIDE):
    """(y0, x0, h, w): the four corners and the first and the last rows at a middle column.  The row pair where y * cols passes 2^32,
    y = 65535 and 65536, is the raster's last two rows: the three windows on the last rows hold it at the first, a middle and the last column."""
    h, w = min(WIN_ROWS, rows), min(WIN_COLS, cols)
    xm = (cols - w) // 2
    out = [(0, 0, h, w), (0, xm, h, w), (0, cols - w, h, w), (rows - h, 0, h, w), (rows - h, xm, h, w), (rows - h, cols - w, h, w)]
    assert all(0 <= y and y + h <= rows and 0 <= x and x + w <= cols for y, x, _, _ in out)
    return out


def enlarged(win, rx, ry, cols, rows):
    """the window enlarged by the radius and clipped to the raster -> (y0, x0, h, w) of the sub-raster and the window's place (dy, dx) in it.
    A reference run on the sub-raster is right on every cell of the window: where the enlargement was clipped, the edge is the raster's own."""
    y0, x0, h, w = win
    ya, xa = max(0, y0 - ry), max(0, x0 - rx)
    yb, xb = min(rows, y0 + h + ry), min(cols, x0 + w + rx)
    return (ya, xa, yb - ya, xb - xa), (y0 - ya, x0 - xa)


# the resample window: a one-row raster of 2^32 + 4101 columns, read around cell 2^32
RESAMPLE_COLS = TWO32 + 4101
RESAMPLE_WINDOW = (TWO32 - 2048, 4096)       # (x, w): 4096 cells from 2^32 - 2048, delivered as 1024 (Average by 4, Bilinear)

# ---- the 2^24-workgroup boundary ----------------------------------------------------------------------------------------------------
TW, TH = 64, 16                              # the focal families' tile (ec_focal_kernels.hpp; ec_focal_rank uses the same)
MAX_GROUPS = (TWO32 - 1) // BLOCK            # 16 777 215 = 2^24 - 1 workgroups of 256 lanes in one dispatch


def boundary_shapes():
    """(cols, rows): 2^24 + 1 tiles in one column; 2 x (2^23 + 1) tiles, the second tile column one cell wide"""
    return [(1, TH * TWO24 + 5), (TW + 1, TH * (TWO24 // 2) + 3)]


def tiles_of(cols, rows):
    return -(-cols // TW), -(-rows // TH)


def boundary_row_spots(cols, rows):
    """[(first row, rows)], every one whole rows: the first 64 rows, the tile rows around tile number 2^24 (in a one-column raster:
    rows 16 * (2^24 - 2) to 16 * (2^24 + 1) + 5), the tile rows in the middle of the raster — where the workgroups numbered last put
    their tiles under the two-front numbering — and the last 64 rows"""
    tx, ty = tiles_of(cols, rows)
    edge = TWO24 // tx                       # the tile row that holds tile number 2^24
    mid = (tx * ty // 2) // tx               # the tile row of the tiles the last workgroups take
    out = [(0, 64)]
    for t in (mid, edge):
        lo, hi = max(0, TH * (t - 2)), min(rows, TH * (t + 2) + 5)
        if hi > lo:
            out.append((lo, hi - lo))
    out.append((rows - 64, 64))
    merged = []
    for lo, ln in sorted(set(out)):
        if merged and lo <= merged[-1][0] + merged[-1][1]:
            plo, pln = merged[-1]
            merged[-1] = (plo, max(plo + pln, lo + ln) - plo)
        else:
            merged.append((lo, ln))
    return merged


def two_front_tile(group, groups):
    """the tile workgroup `group` of a launch of `groups` takes (ec_binop_kernels.hpp): even ones from the front, odd ones from the back"""
    return groups - 1 - (group >> 1) if group & 1 else group >> 1


def tiles_run(model, tiles, numbering):
    """the set of tiles a faulty launch of `tiles` workgroups still runs, as a predicate tile -> bool.
    model: "above_2_24_never" | "grid_mod_2_24" | "first_2_24_minus_1";  numbering: "plain" | "two_front" """
    limit = {"above_2_24_never": TWO24, "grid_mod_2_24": tiles % TWO24, "first_2_24_minus_1": TWO24 - 1}[model]
    limit = min(limit, tiles)
    if numbering == "plain":
        return lambda t: t < limit
    front, back = (limit + 1) // 2, limit // 2    # groups 0, 2, 4 … take tiles 0 .. front; groups 1, 3, … take tiles - 1 down
    return lambda t: t < front or t >= tiles - back


def rows_unwritten(model, numbering, cols, rows, row_spots):
    """how many whole spot rows a faulty launch leaves unwritten in at least one tile column"""
    tx, ty = tiles_of(cols, rows)
    ran = tiles_run(model, tx * ty, numbering)
    lost = 0
    for lo, ln in row_spots:
        for y in range(lo, lo + ln):
            if not all(ran((y // TH) * tx + c) for c in range(tx)):
                lost += 1
    return lost


# ---- the wrap models over indices ----------------------------------------------------------------------------------------------------
def wrapped_index(i, width, mod_bytes):
    """the cell a kernel reaches for cell i of `width`-byte cells when its BYTE offset is taken mod `mod_bytes`; width 1 and 2^32: the cell index
    itself mod 2^32"""
    i = np.asarray(i, dtype=np.uint64)
    return (i * np.uint64(width) % np.uint64(mod_bytes)) // np.uint64(width)


def wrapped_row_start(y, cols):
    """y * cols formed in 32 bits"""
    return (int(y) * int(cols)) % TWO32


def share_past(off, ln, boundary):
    """cells of the spot at or past the boundary"""
    return max(0, off + ln - max(off, boundary))


# ---- ec_distance at its maximum ------------------------------------------------------------------------------------------------------
DIST_SIDE = 32768
DIST_LINES_ROWS = (0, 1, 16383, 16384, 32766, 32767)
DIST_LINES_COLS = (0, 32767)
DIST_MAX_SQ = 20000 * 20000                  # cuts the disc around (0, 0): both axes and the interior have cells on either side
DIST_MASKS = ("corner", "two_corners", "top_row")


def distance_targets(name, side=DIST_SIDE):
    """the target cells (y, x) of a mask, or "top_row" """
    return {"corner": [(0, 0)], "two_corners": [(0, 0), (side - 1, side - 1)], "top_row": "top_row"}[name]


def distance_sq(name, ys, xs, side=DIST_SIDE):
    """d2 at the cells (ys, xs) (broadcast), exact int64: the closed forms"""
    ys, xs = np.asarray(ys, dtype=np.int64), np.asarray(xs, dtype=np.int64)
    ys, xs = np.broadcast_arrays(ys, xs)
    if name == "top_row":
        return ys * ys + 0 * xs
    d = ys * ys + xs * xs
    if name == "two_corners":
        fy, fx = side - 1 - ys, side - 1 - xs
        d = np.minimum(d, fy * fy + fx * fx)
    return d


def distance_expected(name, ys, xs, max_sq, out_f64, side=DIST_SIDE):
    """-> (cells, mask bytes) at (ys, xs): include/erased_cells.h's rule on the closed form.  F64 is math.sqrt of the same integers."""
    d2 = distance_sq(name, ys, xs, side)
    assert int(d2.max()) < TWO31
    valid = d2 <= (max_sq if max_sq is not None else 0xFFFFFFFF)
    if out_f64:
        cells = np.array([math.sqrt(int(v)) for v in d2.ravel()], dtype=np.float64).reshape(d2.shape)
    else:
        cells = d2.astype(np.uint32)
    return np.where(valid, cells, cells.dtype.type(0)), valid.astype(np.uint8)


def distance_lines(side=DIST_SIDE):
    """[(ys, xs)] index arrays of the whole rows and columns compared"""
    full = np.arange(side, dtype=np.int64)
    return [(np.full(side, r, dtype=np.int64), full) for r in DIST_LINES_ROWS] + [(full, np.full(side, c, dtype=np.int64)) for c in DIST_LINES_COLS]


# ---- the reductions' closed forms ----------------------------------------------------------------------------------------------------
def constant_moments(value, count):
    """(count, sum, sum of squares) of `count` cells that all hold the integer `value`: exact Python integers"""
    return count, value * count, value * value * count
