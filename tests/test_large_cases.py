"""The spots of tests/test_gpu_large_rasters.py (tests/large_cases.py) expose every mistake the large shapes are there for — shown here
on the CPU, with the very inputs the GPU file uses (oracle.eco's host generator at the spots' offsets): each mistake is restated in
plain Python or numpy over the spot slices, and the cells the GPU file expects differ from the cells the mistake would leave.

For a wrap model "differ" means that at least half of the spot cells past the boundary change; for a launch that loses tiles, that
whole spot rows stay unwritten (the GPU file pre-fills every output with a pattern no result holds)."""
import numpy as np
import pytest

import large_cases as K
from oracle import eco


def stream(name, off, ln):
    ct, seed, lo, hi = K.STREAMS[name]
    return (eco.fill_u8 if ct == 0 else eco.fill_u16)(ln, seed, base=off, lo=lo, hi=hi)


def changed_share(name, idx, wrapped):
    """share of the consecutive cells `idx` whose hashed value differs from the value at `wrapped` (consecutive but for a few jumps)"""
    a = stream(name, int(idx[0]), idx.size)
    w = wrapped.astype(np.int64)
    cuts = [0] + [int(k) + 1 for k in np.flatnonzero(np.diff(w) != 1)] + [idx.size]
    assert len(cuts) <= 4
    b = np.concatenate([stream(name, int(w[lo]), hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])])
    return float((a != b).mean())


def test_the_spots_sit_where_the_boundaries_are():
    assert K.N == 65537 ** 2 == K.TWO32 + 131073
    for sp in (K.spots(), K.short_spots()):
        (o0, l0), (o1, l1), (o2, l2), (o3, l3) = sp
        assert o0 == 0 and o1 < K.TWO32 < o1 + l1 and o2 == K.TWO32 - 5 and o2 + l2 > K.TWO32 and o3 + l3 == K.N
        assert min(l0, l1, l2, l3) >= K.SHORT
    assert [o for o, _ in K.spots()] == [0, K.TWO32 - 70000, K.TWO32 - 5, K.N - 100003]
    f = K.f64_spots()
    assert f[1][0] * 8 < K.TWO31 < (f[1][0] + f[1][1]) * 8 and f[2][0] * 8 < K.TWO32 < (f[2][0] + f[2][1]) * 8 and f[3][0] + f[3][1] == K.N_F64
    for n in (K.TWO32, K.N):
        b = K.blocks(n)
        assert b[0][0] == 0 and b[-1][0] + b[-1][1] == n and any(o <= K.TWO32 - 1 < o + ln for o, ln in b)
        assert all(b[k][0] + b[k][1] <= b[k + 1][0] for k in range(len(b) - 1))
    assert K.WRAP_ROW * K.SIDE == K.TWO32 - 1 and (K.WRAP_ROW + 1) * K.SIDE > K.TWO32
    wins = K.windows()
    assert K.WRAP_ROW + 1 == K.SIDE - 1   # the row pair is the raster's last two rows
    assert len(wins) == 6 and sum(1 for y, x, h, w in wins if y <= K.WRAP_ROW and y + h == K.SIDE) == 3
    x, w = K.RESAMPLE_WINDOW
    assert x < K.TWO32 < x + w <= K.RESAMPLE_COLS


@pytest.mark.parametrize("name", sorted(K.STREAMS))
def test_a_cell_index_taken_mod_2_32_changes_the_cells_past_it(name):
    """loads: cell i reads the cell 2^32 places earlier.  stores: the value of cell i lands 2^32 places earlier, in the first spot,
    and cell i keeps the pre-fill.  Both are seen when the hashed cells i and i - 2^32 differ."""
    for off, ln in K.spots()[1:]:
        past = K.share_past(off, ln, K.TWO32)
        assert past >= 5
        idx = np.arange(off + ln - past, off + ln, dtype=np.uint64)
        wrapped = K.wrapped_index(idx, 1, K.TWO32)
        assert int(wrapped[0]) == int(idx[0]) - K.TWO32
        assert changed_share(name, idx, wrapped) >= 0.5, (name, off)
    # the landing places of the wrapped stores lie inside the first spot
    assert K.N - K.TWO32 > K.spots()[0][1] and K.wrapped_index(np.uint64(K.TWO32), 1, K.TWO32) == 0


@pytest.mark.parametrize("width,mod", [(2, K.TWO32), (2, K.TWO31), (8, K.TWO32), (8, K.TWO31)])
def test_a_byte_offset_taken_mod_2_32_or_2_31_changes_the_cells_past_it(width, mod):
    """2-byte outputs at the 1-D spots (byte 2^32 is cell 2^31: every spot but the first lies past it), 8-byte outputs at the f64 case's"""
    if width == 2:
        sp, names = K.spots()[1:], ("a", "b")
    else:
        sp, names = [s for s in K.f64_spots() if (s[0] + s[1]) * 8 > mod], ("wide",)
        assert len(sp) >= (2 if mod == K.TWO32 else 3)
    for off, ln in sp:
        first = max(off, mod // width)
        idx = np.arange(first, off + ln, dtype=np.uint64)
        wrapped = K.wrapped_index(idx, width, mod)
        assert (wrapped != idx).all()
        for name in names:
            assert changed_share(name, idx, wrapped) >= 0.5, (name, off, width, mod)


@pytest.mark.parametrize("name", ["a", "ma", "classes"])
def test_y_times_cols_in_32_bits_changes_the_rows_past_it(name):
    cols = K.SIDE
    seen = 0
    for y0, x0, h, w in K.windows():
        for y in range(y0, y0 + h):
            start = K.wrapped_row_start(y, cols)
            if start == y * cols:
                continue
            idx = np.arange(y * cols + x0, y * cols + x0 + w, dtype=np.uint64)
            wrapped = np.arange(start + x0, start + x0 + w, dtype=np.uint64)
            assert changed_share(name, idx, wrapped) >= 0.5 - 0.2 * (name != "a"), (name, y, x0)   # one row of 200 cells of a 0 / 1 stream
            seen += 1
    assert seen == 3   # row 65536, the only one whose start passes 32 bits, in the three windows on the last rows
    # over all those rows together the 0 / 1 streams change in half of the cells as well
    total = changed = 0
    for y0, x0, h, w in K.windows():
        for y in range(max(y0, K.WRAP_ROW + 1), y0 + h):
            a, b = stream(name, y * cols + x0, w), stream(name, K.wrapped_row_start(y, cols) + x0, w)
            total, changed = total + w, changed + int((a != b).sum())
    assert changed * 2 >= total


@pytest.mark.parametrize("numbering", ["plain", "two_front"])
@pytest.mark.parametrize("model", ["above_2_24_never", "grid_mod_2_24", "first_2_24_minus_1"])
def test_a_launch_that_loses_tiles_leaves_spot_rows_unwritten(model, numbering):
    for cols, rows in K.boundary_shapes():
        tx, ty = K.tiles_of(cols, rows)
        assert tx * ty > K.TWO24 >= K.MAX_GROUPS + 1
        spots = K.boundary_row_spots(cols, rows)
        assert spots[0] == (0, 64) and spots[-1][0] <= rows - 64 and sum(spots[-1]) == rows and sum(ln for _, ln in spots) <= 400
        assert K.rows_unwritten(model, numbering, cols, rows, spots) >= 1, (cols, rows)
    # the issue's rows for the one-column raster are among the spots
    cols, rows = K.boundary_shapes()[0]
    lo, hi = K.TH * (K.TWO24 - 2), min(rows, K.TH * (K.TWO24 + 1) + 5)   # to the raster's end
    assert any(s <= lo and hi <= s + ln for s, ln in K.boundary_row_spots(cols, rows))


def test_what_the_runtime_did_is_the_grid_mod_2_24_model():
    """measured: a launch of 2^24 + 1 workgroups ran one workgroup, tile 0 — 256 * (2^24 + 1) mod 2^32 = 256 work-items"""
    cols, rows = K.boundary_shapes()[0]
    ran = K.tiles_run("grid_mod_2_24", K.TWO24 + 1, "two_front")
    assert ran(0) and not ran(1) and not ran(K.TWO24)
    assert (K.BLOCK * (K.TWO24 + 1)) % K.TWO32 == K.BLOCK and K.MAX_GROUPS == K.TWO24 - 1


def test_two_front_numbering_is_a_bijection():
    for groups in (1, 2, 3, 8, 9):
        assert sorted(K.two_front_tile(g, groups) for g in range(groups)) == list(range(groups))


def test_distance_closed_forms_against_brute_force():
    side = 9
    ys, xs = np.mgrid[0:side, 0:side]
    for name in K.DIST_MASKS:
        t = K.distance_targets(name, side)
        targets = [(0, x) for x in range(side)] if t == "top_row" else t
        brute = np.min([(ys - ty) ** 2 + (xs - tx) ** 2 for ty, tx in targets], axis=0)
        assert np.array_equal(K.distance_sq(name, ys, xs, side), brute), name
    cells, valid = K.distance_expected("corner", ys, xs, 10, True, side)
    assert valid[0, 3] == 1 and valid[1, 3] == 1 and valid[2, 3] == 0 and cells[2, 3] == 0.0 and cells[0, 3] == 3.0
    # the cut of the large case leaves cells on either side on both axes and inside, and the largest d2 fits 31 bits
    d = K.distance_sq("corner", [0, 0, K.DIST_SIDE - 1, 14142, 14143], [19999, 20001, K.DIST_SIDE - 1, 14142, 14143])
    assert d[0] <= K.DIST_MAX_SQ < d[1] and d[3] <= K.DIST_MAX_SQ < d[4] and int(d[2]) == 2 * 32767 ** 2 < K.TWO31
