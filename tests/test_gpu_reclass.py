"""ec_reclass on the GPU, bit for bit against tests/reclass_ref.py (which knows no thresholds and is held to the oracle's
predicate by tests/test_reclass_ref.py): every cell type against breaks of its own type, of Float64 and of a type from the far side
of the lattice, both `right`, an output type per width and all ten for one raster type, the break counts at the edges of the
search's step count, masked and not, validity bytes with zeros, dst_mask given and not, EVERY cell of the 1- and 2-byte types,
tables no cell reaches, and the special cells of the wide types.  Sizes are a few tiles (T = 256 x 2 x CPL cells), lengths leave
a ragged tail."""
import numpy as np
import pytest

import reclass_ref as Q
from vectors import rand_cells

pytestmark = pytest.mark.gpu

CROSS = {Q.U8: Q.I64, Q.U16: Q.I8, Q.U32: Q.F32, Q.U64: Q.I64, Q.I8: Q.U64, Q.I16: Q.U32, Q.I32: Q.U64, Q.I64: Q.U64, Q.F32: Q.I64, Q.F64: Q.U64}
ONE_PER_WIDTH = (Q.U8, Q.I16, Q.F32, Q.F64)
STEP_EDGES = (1, 2, 3, 7, 8, 9, 127, 128, 254, 255)


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def bits(a):
    return np.ascontiguousarray(a).view(Q.WORD[a.dtype.itemsize])


def class_values(dt, n_classes, seed):
    """n_classes cells of type dt, special values among them, and a nodata value that is none of them where the type has room"""
    v = rand_cells(dt, n_classes, 4200 + seed)
    v[: min(n_classes, 3)] = np.array([1, 0, 2], Q.NP[dt])[: min(n_classes, 3)]
    return v, np.array([201], np.int64).astype(Q.NP[dt])[0]


def check(ec, t, x, mask, bt, breaks, right, dt, valid, want_mask, what):
    """one launch of ec_reclass through the Python mirror's internal call, against reclass_ref.reclass"""
    B = ec.buffer
    values, nodata = class_values(dt, len(breaks) + 1, len(breaks) + dt)
    table = ec.ReclassTable(t, np.asarray(breaks, Q.NP[bt]), values, right=right, valid=valid, nodata=nodata if mask is not None else None)
    assert (table.ct, table.bt, table.dt) == (t, bt, dt)
    buf = ec.CellBuffer.from_vec(x)
    m = ec.Mask.new(mask.astype(bool)) if mask is not None else None
    out, om = B._reclass(buf, m, table, want_mask)
    want, want_ok = Q.reclass(t, x, mask, bt, breaks, right, dt, values, valid, nodata if mask is not None else None)
    got = out.to_numpy()
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, (what, f"{bad.size} cells differ, first at {bad[0]} of {x.size}: cell {x[bad[0]]!r} got {got[bad[0]]!r} want {want[bad[0]]!r}")
    if want_mask:
        gm = om.to_numpy().astype(np.uint8)
        assert np.array_equal(gm, want_ok), (what, "dst_mask", int(np.flatnonzero(gm != want_ok)[0]))
    return table


def some_valid(n_classes, seed):
    v = (np.random.default_rng(seed).random(n_classes) < 0.7).astype(np.uint8)
    v[0], v[-1] = 0, 1
    if n_classes > 2:
        v[1] = 7     # any non-zero byte is valid
    return v


def every_type_cases(t):
    """(bt, breaks, cells, mask) of test_every_type_three_break_types_both_sides — tests/test_reclass_faults.py shows that these
    inputs expose each modelled mistake"""
    for bt in (t, Q.F64, CROSS[t]):
        for nb in (7, 40):
            breaks = Q.gpu_tables(t, bt, nb, seed=t)
            x = Q.gpu_inputs(t, bt, breaks, n_random=3 * Q.tile(t, Q.U8) // 2 if Q.size_of(t) > 1 else 2 * Q.tile(t, Q.U8))
            x = x[:Q.tail_len(x.size)]
            yield bt, breaks, x, Q.gpu_masks(x.size, seed=t)


@pytest.mark.parametrize("t", range(Q.NT), ids=Q.NAMES)
def test_every_type_three_break_types_both_sides(ec, t):
    k = 0
    for bt, breaks, x, mask in every_type_cases(t):
        for right in (False, True):
            dt = ONE_PER_WIDTH[k % 4]
            masked, with_valid, want_mask = k % 2 == 1, k % 3 != 0, (k % 3 != 0 or k % 4 < 2)
            k += 1
            check(ec, t, x, mask if masked else None, bt, breaks, right, dt, some_valid(len(breaks) + 1, k) if with_valid else None, want_mask,
                  (Q.NAMES[t], Q.NAMES[bt], len(breaks), "right", right, Q.NAMES[dt], "masked", masked, "valid", with_valid, "dst_mask", want_mask))


def test_all_ten_output_types(ec):
    t, bt = Q.F32, Q.F64
    breaks = Q.gpu_tables(t, bt, 9)
    x = Q.gpu_inputs(t, bt, breaks, n_random=3 * Q.tile(t, Q.F64) + 7)
    mask = Q.gpu_masks(x.size)
    for dt in range(Q.NT):
        check(ec, t, x, None, bt, breaks, False, dt, None, False, ("unmasked ->", Q.NAMES[dt]))
        check(ec, t, x, mask, bt, breaks, True, dt, some_valid(10, dt), True, ("masked ->", Q.NAMES[dt]))


@pytest.mark.parametrize("nb", STEP_EDGES)
def test_the_edges_of_the_search_step_count(ec, nb):
    for t, dt in ((Q.U16, Q.U8), (Q.F32, Q.I16), (Q.I64, Q.F64), (Q.U32, Q.U8), (Q.U8, Q.U8)):
        breaks = Q.gpu_tables(t, t, nb, seed=nb)
        assert breaks.size == nb
        x = Q.gpu_inputs(t, t, breaks, n_random=Q.tile(t, dt) + 7)
        for right in (False, True):
            tab = check(ec, t, x, None, t, breaks, right, dt, None, False, (Q.NAMES[t], nb, right))
            assert Q.parse(tab.bytes())["n_reached"] in (nb, nb - 1)   # right = 1: a break at the type's greatest cell is past every cell


@pytest.mark.parametrize("t", (Q.U8, Q.I8, Q.U16, Q.I16), ids=lambda t: Q.NAMES[t])
def test_every_cell_of_the_narrow_types(ec, t):
    info = np.iinfo(Q.NP[t])
    every = np.arange(info.min, info.max + 1).astype(Q.NP[t])
    if every.size == 256:   # the whole type 33 times over and a ragged tail: more than one tile of 8192 cells
        x = np.concatenate([np.tile(every, 33), every[:15]])
    else:
        x = np.concatenate([every, every[::-1][:15]])
    mask = Q.gpu_masks(x.size, seed=3)
    for bt in (t, Q.F64, CROSS[t]):
        for nb in (255, 3):
            breaks = Q.gpu_tables(t, bt, nb, seed=nb)
            for right in (False, True):
                check(ec, t, x, None, bt, breaks, right, Q.U8, None, False, (Q.NAMES[t], Q.NAMES[bt], nb, right))
            check(ec, t, x, mask, bt, breaks, True, Q.I16, some_valid(len(breaks) + 1, nb), True, (Q.NAMES[t], Q.NAMES[bt], nb, "masked"))


def test_tables_no_cell_reaches(ec):
    """n_reached == 0 because every break lies above every cell (class 0 everywhere), and thresholds all at the least key because
    every break lies below (the top class everywhere)"""
    for t, bt, above, below in ((Q.U8, Q.F64, [300.0, 1e9], [-7.5, -0.5]), (Q.I16, Q.I64, [2**15, 2**40], [-2**40, -2**15 - 1]),
                                (Q.U32, Q.F64, [2.0**32, 2.0**33], [-2.0, -1.0]), (Q.I8, Q.U64, [128, 2**63], None), (Q.U64, Q.I8, None, [-128, -1])):
        x = rand_cells(t, 2 * Q.tile(t, Q.U8) + 11, 8, specials=True)
        for breaks in (above, below):
            if breaks is None:
                continue
            for right in (False, True):
                tab = Q.parse(check(ec, t, x, None, bt, breaks, right, Q.U8, None, False, (Q.NAMES[t], breaks, right)).bytes())
                assert tab["n_reached"] == (0 if breaks is above else 2)
            check(ec, t, x, Q.gpu_masks(x.size), bt, breaks, False, Q.F32, [1, 0, 1], True, (Q.NAMES[t], breaks, "masked"))


@pytest.mark.parametrize("t", (Q.U32, Q.U64, Q.I32, Q.I64, Q.F32, Q.F64), ids=lambda t: Q.NAMES[t])
def test_the_special_cells_of_the_wide_types(ec, t):
    """2^24 +- 1, 2^53 +- 1, the limits, +-0.0, +-inf, NaNs of both signs and the neighbours of all of them, against breaks AT them"""
    sp = Q.special_cells(t)
    x = np.concatenate([sp, Q.neighbours(t, sp), rand_cells(t, Q.tile(t, Q.U8), 12)])
    for bt in (t, Q.F64, Q.U64, Q.I64, Q.F32):
        with np.errstate(all="ignore"):
            cand = np.concatenate([sp.astype(Q.NP[bt]), Q.special_cells(bt)])
        if Q.NP[bt].kind == "f":
            cand = cand[~np.isnan(cand)]
        _, key = Q._in_union(t, np.zeros(0, Q.NP[t]), bt, cand)
        breaks = cand[np.unique(key, return_index=True)[1]][:255]
        for right in (False, True):
            check(ec, t, x, None, bt, breaks, right, Q.U8, None, False, (Q.NAMES[t], Q.NAMES[bt], right))
    if Q.NP[t].kind == "f":   # the header's two examples
        inf = Q.NP[t].type(np.inf)
        values = np.arange(3, dtype=np.uint8)
        top = ec.CellBuffer.from_vec(x).reclassify(np.array([0.5, inf], Q.NP[t]), values, right=True).to_numpy()
        assert np.array_equal(top == 2, np.isnan(x) & ~np.signbit(x))
        bottom = ec.CellBuffer.from_vec(x).reclassify(np.array([-inf, 0.5], Q.NP[t]), values).to_numpy()
        assert np.array_equal(bottom == 0, np.isnan(x) & np.signbit(x))


def test_a_nan_under_a_cleared_mask_byte_leaves_no_trace(ec):
    x = np.full(5000, np.nan, np.float64)
    x[::2] = 0.3
    mask = (~np.isnan(x)).astype(np.uint8)
    got = ec.MaskedCellBuffer(ec.CellBuffer.from_vec(x), ec.Mask.new(mask.astype(bool))).reclassify([0.2, 0.4], np.array([1.5, 2.5, 3.5]), nodata=-9999.0)
    assert np.array_equal(got.buffer().to_numpy(), np.where(mask, 2.5, -9999.0)) and np.array_equal(got.mask().to_numpy().astype(np.uint8), mask)


def test_one_table_many_launches(ec):
    """the uploaded record is reused across launches and left as it was"""
    t = ec.ReclassTable(ec.UInt16, [100, 1000, 10000], np.array([0, 1, 2, 3], np.uint8))
    before = t.bytes()
    for n in (1, 15, 4096, 4097, 3 * 4096 + 7):
        x = rand_cells(Q.U16, n, n)
        assert np.array_equal(ec.CellBuffer.from_vec(x).reclassify(t).to_numpy(), np.digitize(x, [100, 1000, 10000]).astype(np.uint8))
    assert np.array_equal(ec.buffer._download(t.mem, np.uint8, Q.TABLE_BYTES), np.frombuffer(before, np.uint8))
