"""Every kernel family past 2^32 cells, past 2^31 and 2^32 bytes of output, at 2^24 workgroups in one launch and, for ec_distance,
at its documented maximum — on one MI355X.  The existing suite runs these families on rasters of a few tiles; here they run at the
sizes the library exists for, and the results are compared bit for bit with the same references at SPOTS (tests/large_cases.py: the
start, both sides of every boundary, the tail).  tests/test_large_cases.py shows on the CPU that the spots see every modelled mistake:
a 32-bit cell index or byte offset, y * cols in 32 bits, a launch that loses the tiles numbered 2^24 and above.

Inputs are generated on the device (ec_synth_fill) and their slices are checked against oracle.eco's host generator.  Every output
buffer is first filled through ec_fill with a pattern the result cannot hold at that cell (asserted per spot), so a cell that was
never written shows.  Nothing is sampled inside a spot.  No test holds more than 64 GiB of device memory.

What the runtime does with more than 2^24 - 1 workgroups of 256 lanes in one launch (DESIGN.md "Launches past 2^24 workgroups"): it
reports success and runs grid * 256 mod 2^32 work-items.  The one-workgroup-per-tile families therefore cut such a job into several
launches, and the streaming families refuse it; both are tested here."""
import ctypes as C

import numpy as np
import pytest

import cast_ref
import compare_ref as CMP
import composite_rank_ref as RANK
import composite_ref as COMP
import focal_rank_ref as FR
import focal_ref as F
import large_cases as K
import reclass_ref as RC
import resample_ref as RS
import stats_ref as SR
from oracle import eco

pytestmark = pytest.mark.gpu

U8, U16, U32, I8, I16, F64 = 0, 1, 2, 4, 5, 9
WHOLE = 1
OK, ARG = 0, 6
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
SEED = 0x1A26E000


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


@pytest.fixture(autouse=True)
def trimmed(ec):
    """every test gives its device memory back: the next one starts from an empty pool"""
    yield
    ec.synchronize()
    ec._ffi.check(ec.lib().ec_pool_trim(0))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def chk(ec, st):
    ec._ffi.check(st)


def synth(ec, ct, n, seed, lo, hi):
    b = ec.CellBuffer.empty(n, ct)
    chk(ec, ec.lib().ec_synth_fill(ct, b.mem.ptr, n, seed, 0, float(lo), float(hi), ec.stream()))
    return b


def synth_mask(ec, n, seed):
    """mask bytes 0 / 1 from the u8 generator, so that oracle.eco restates them"""
    m = ec.Mask.empty(n)
    chk(ec, ec.lib().ec_synth_fill(U8, m.mem.ptr, n, seed, 0, 0.0, 1.0, ec.stream()))
    return m


def host(ct, off, ln, seed, lo, hi):
    return (eco.fill_u8 if ct == U8 else eco.fill_u16)(ln, seed, base=off, lo=lo, hi=hi)


def filled(ec, ct, n, value):
    """an output buffer of n cells holding `value` everywhere (ec_fill)"""
    return ec.CellBuffer.fill(n, ec.CellValue(ct, value))


def filled_mask(ec, n):
    """an output mask holding the byte 2, which no kernel writes"""
    m = ec.Mask.empty(n)
    v = ec.CellValue(U8, 2).to_ec()
    chk(ec, ec.lib().ec_fill(U8, m.mem.ptr, n, C.byref(v), ec.stream()))
    return m


def same(got, exp, prefill, what):
    """bit for bit, and no expected cell equals `prefill`, what the buffer held in every cell before the call"""
    got, exp = np.asarray(got).ravel(), np.asarray(exp).ravel()
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    pre = bits(np.array([prefill], dtype=exp.dtype))[0]
    assert not (bits(exp) == pre).any(), (what, "the pre-fill pattern is a possible result")
    if not np.array_equal(bits(got), bits(exp)):
        j = int(np.flatnonzero(bits(got) != bits(exp))[0])
        unwritten = int((bits(got) == pre).sum())
        raise AssertionError(f"{what}: first difference at cell {j} of the spot: got {got[j]!r} expected {exp[j]!r}; {unwritten} cells still hold the pre-fill")


def nan_filled(ec, n):
    return filled(ec, F64, n, float("nan"))


def prefill_of(buf):
    """what ec_fill left in every cell of a freshly filled buffer: its cell 0"""
    return buf.shard(0, 1).to_numpy()[0]


# ------------------------------------------------------------------------------------------------------------ the 2^24 boundary
def focal_call(ec, what, ct, src, smask, cols, rows, radius, flags, out, om, weights=None):
    L = ec.lib()
    sm, dm = (smask.mem.ptr if smask is not None else None), (om.mem.ptr if om is not None else None)
    rx, ry = radius
    if what == "convolve":
        w = np.ascontiguousarray(weights, dtype=np.float64)
        return L.ec_focal_convolve(ct, src.mem.ptr, sm, cols, rows, w.ctypes.data_as(C.POINTER(C.c_double)), rx, ry, flags, out.mem.ptr, dm, ec.stream())
    if what == "median":
        return L.ec_focal_rank(ct, src.mem.ptr, sm, cols, rows, rx, ry, 1, 2, 0, flags, out.mem.ptr, dm, ec.stream())
    if what == "majority":
        return L.ec_focal_majority(ct, src.mem.ptr, sm, cols, rows, rx, ry, flags, out.mem.ptr, dm, ec.stream())
    return L.ec_focal(what, ct, src.mem.ptr, sm, cols, rows, rx, ry, flags, out.mem.ptr, dm, ec.stream())


def focal_expected(what, a, m, radius, flags, weights=None):
    rx, ry = radius
    whole = bool(flags & WHOLE)
    if what == "convolve":
        return F.convolve(a, m, weights, False, whole)
    if what == "median":
        return FR.focal_rank(a, m, rx, ry, 1, 2, 0, whole)
    if what == "majority":
        return FR.focal_majority(a, m, rx, ry, whole)
    return F.focal(what, a, m, rx, ry, whole)


WEIGHTS3 = np.array([[0.25, -1.0, 0.5], [2.0, 1.0, -0.125], [0.75, 3.0, -2.0]])
# (what, masked, radius, flags, source range): every focal-family entry point once; ec_focal all four operations, masked and not
BOUNDARY_CASES = [(op, masked, (2, 3), 0, (1, 200)) for op in (F.SUM, F.MEAN, F.MIN, F.MAX) for masked in (False, True)] + [
    ("convolve", False, (1, 1), 0, (1, 200)), ("median", False, (0, 1), 0, (1, 200)), ("majority", False, (1, 1), 0, (1, 4))]
BOUNDARY_IDS = [f"{['sum', 'mean', 'min', 'max'][c[0]] if isinstance(c[0], int) else c[0]}{'-masked' if c[1] else ''}" for c in BOUNDARY_CASES]


def run_focal_at_rows(ec, what, masked, radius, flags, src_range, cols, rows, row_spots, seed):
    """one call over the whole raster; every cell and mask byte of the spot rows against the reference run on those rows enlarged by ry"""
    n = cols * rows
    lo, hi = src_range
    src = synth(ec, U8, n, seed, lo, hi)
    smask = synth_mask(ec, n, seed + 1) if masked else None
    summing = what in (F.SUM, F.MEAN, "convolve")
    out = nan_filled(ec, n) if summing else filled(ec, U8, n, 255)
    om = filled_mask(ec, n) if masked else None
    pre = prefill_of(out)
    weights = WEIGHTS3 if what == "convolve" else None
    assert focal_call(ec, what, U8, src, smask, cols, rows, radius, flags, out, om, weights) == OK
    ry = radius[1]
    for r0, nr in row_spots:
        a0, a1 = max(0, r0 - ry), min(rows, r0 + nr + ry)
        ha = host(U8, a0 * cols, (a1 - a0) * cols, seed, lo, hi)
        assert np.array_equal(src.shard(a0 * cols, ha.size).to_numpy(), ha)
        hm = None
        if masked:
            hm = host(U8, a0 * cols, (a1 - a0) * cols, seed + 1, 0, 1)
            assert np.array_equal(smask.shard(a0 * cols, hm.size).to_numpy(), hm)
            hm = hm.reshape(a1 - a0, cols)
        exp, ev = focal_expected(what, ha.reshape(a1 - a0, cols), hm, radius, flags, weights)
        keep = slice(r0 - a0, r0 - a0 + nr)
        same(out.shard(r0 * cols, nr * cols).to_numpy(), exp[keep], pre, (what, masked, cols, rows, r0))
        if om is not None:
            same(om.shard(r0 * cols, nr * cols).to_numpy(), ev[keep], np.uint8(2), (what, masked, cols, rows, r0, "mask"))
    return out, om


@pytest.mark.parametrize("case", BOUNDARY_CASES, ids=BOUNDARY_IDS)
def test_one_column_of_2_24_plus_1_tiles(ec, case):
    """cols = 1, rows = 16 * 2^24 + 5: 2^24 + 1 tiles, one more workgroup than a launch holds.  The first parametrised case is the
    probe of what the runtime does with such a grid; the job is cut into two launches."""
    what, masked, radius, flags, src_range = case
    cols, rows = K.boundary_shapes()[0]
    assert K.tiles_of(cols, rows) == (1, K.TWO24 + 1)
    spots = K.boundary_row_spots(cols, rows)
    out, om = run_focal_at_rows(ec, what, masked, radius, flags, src_range, cols, rows, spots, SEED + 0x100)
    if om is not None:   # no mask byte anywhere still holds the pre-fill: counted on the device
        assert om.to_numpy().max() <= 1


def test_two_tile_columns_of_2_23_plus_1_tile_rows_max(ec):
    """cols = 65, rows = 16 * 2^23 + 3: 2^24 + 2 tiles in two tile columns, the second one cell wide"""
    cols, rows = K.boundary_shapes()[1]
    assert K.tiles_of(cols, rows) == (2, K.TWO24 // 2 + 1)
    run_focal_at_rows(ec, F.MAX, False, (2, 3), 0, (1, 200), cols, rows, K.boundary_row_spots(cols, rows), SEED + 0x110)


def test_the_streaming_families_refuse_what_one_launch_cannot_hold(ec):
    """from sizes alone, on small arenas that stay untouched: a binop, a scalar binop, a masked binop, a map and a one-pass tree over
    more tiles than a launch holds are EC_ERR_ARG before any device work, with a message that names the limit"""
    from arena import Arena
    L, s = ec.lib(), ec.stream()
    knob = C.c_int64(0)
    chk(ec, L.ec_stat_get(b"tune.unaligned_vector", C.byref(knob)))
    assert knob.value == 1   # the default: every launch below takes a tile kernel, whose launcher refuses; none takes a grid-stride one
    a, b, m, om = (Arena(4096, seed=k, ec=ec).hold(np.full(4096, k, np.uint8)) for k in (1, 2, 4, 5))
    out = Arena(4096 * 8, seed=3, ec=ec).hold(np.zeros(4096, np.float64))
    huge = (K.MAX_GROUPS + 1) * 8192          # 2^24 map tiles of 8 KiB of u8 cells; more than 2^24 tiles of every binop and tree kernel
    v = ec.CellValue(F64, 2.5).to_ec()
    dt = (C.c_uint8 * 4)(U8, U8, U8, U8)
    p = (C.c_void_p * 4)(a.ptr, b.ptr, a.ptr, b.ptr)
    sc = (ec._ffi.EcValue * 4)()
    refused = [
        L.ec_binop(ec.DIV, U8, a.ptr, U8, b.ptr, huge, out.ptr, s),
        L.ec_binop_scalar(ec.MUL, U8, a.ptr, huge, C.byref(v), out.ptr, s),
        L.ec_masked_binop(ec.ADD, U8, a.ptr, m.ptr, U8, b.ptr, m.ptr, huge, out.ptr, om.ptr, s),
        L.ec_mask_not(m.ptr, huge, om.ptr, s),
        L.ec_fused(ec.SUB, ec.DIV, ec.ADD, dt, p, sc, huge, out.ptr, s),
    ]
    assert refused == [ARG] * len(refused)
    with pytest.raises(ec._ffi.EcError, match="16777215"):
        chk(ec, L.ec_mask_not(m.ptr, huge, om.ptr, s))
    ec.synchronize()
    for arena in (a, b, out, m, om):
        arena.check_unchanged("a refused call")


# ------------------------------------------------------------------------------------------------------------ 1-D families
def stream_buf(ec, name, n):
    ct, seed, lo, hi = K.STREAMS[name]
    if hi == 1 and ct == U8:
        return synth_mask(ec, n, seed)
    return synth(ec, ct, n, seed, lo, hi)


def stream_host(name, off, ln):
    ct, seed, lo, hi = K.STREAMS[name]
    return host(ct, off, ln, seed, lo, hi)


class Inputs:
    """device buffers of named streams (tests/large_cases.py STREAMS) over n cells and their host slices at the spots; every slice
    downloaded once and checked against the host generator"""

    def __init__(self, ec, n, names, spots):
        self.ec, self.n, self.spots = ec, n, spots
        self.dev = {name: stream_buf(ec, name, n) for name in names}
        self.at = {name: [stream_host(name, off, ln) for off, ln in spots] for name in names}
        for name in names:
            for (off, ln), h in zip(spots, self.at[name]):
                assert np.array_equal(self.dev[name].shard(off, ln).to_numpy(), h), (name, off)

    def ptr(self, name):
        return self.dev[name].mem.ptr

    def check(self, out, expected, prefill, what):
        """out: a CellBuffer or Mask; expected(k) -> the cells of spot k"""
        for k, (off, ln) in enumerate(self.spots):
            same(out.shard(off, ln).to_numpy(), expected(k), prefill, (what, off))


@pytest.fixture(scope="class")
def one_d(ec):
    inp = Inputs(ec, K.N, ("a", "a2", "b", "ma", "mb"), K.spots())
    yield inp
    inp.dev.clear()


MASK_PRE = np.uint8(2)


class TestOneDimensionalFamiliesPast2_32Cells:
    """n = 65537^2 cells: u8 `a`, `a2` in 1 .. 200, u16 `b` in 1 .. 400, masks `ma`, `mb`; about 26 GB of inputs for the class"""

    def test_compare_with_a_buffer_and_with_a_scalar(self, ec, one_d):
        L, n = ec.lib(), one_d.n
        out = filled_mask(ec, n)
        chk(ec, L.ec_compare(CMP.LT, U8, one_d.ptr("a"), one_d.ptr("ma"), U16, one_d.ptr("b"), None, n, out.mem.ptr, ec.stream()))
        one_d.check(out, lambda k: CMP.masked_relation(CMP.LT, U8, one_d.at["a"][k], one_d.at["ma"][k], U16, one_d.at["b"][k], None), MASK_PRE, "compare")
        out = filled_mask(ec, n)
        v = ec.CellValue(U8, 100).to_ec()
        chk(ec, L.ec_compare_scalar(CMP.GE, U8, one_d.ptr("a"), None, n, C.byref(v), out.mem.ptr, ec.stream()))
        one_d.check(out, lambda k: CMP.relation(CMP.GE, U8, one_d.at["a"][k], U8, np.full(one_d.at["a"][k].size, 100, np.uint8)), MASK_PRE, "compare_scalar")

    def test_select_and_masked_select(self, ec, one_d):
        L, n = ec.lib(), one_d.n
        at = one_d.at
        out = filled(ec, U8, n, 255)
        chk(ec, L.ec_select(U8, one_d.ptr("a"), one_d.ptr("a2"), one_d.ptr("ma"), n, out.mem.ptr, ec.stream()))
        one_d.check(out, lambda k: CMP.select(at["ma"][k], at["a"][k], at["a2"][k]), np.uint8(255), "select")
        out, om = filled(ec, U8, n, 255), filled_mask(ec, n)
        sel = stream_buf(ec, "msel", n)
        hsel = [stream_host("msel", off, ln) for off, ln in one_d.spots]
        chk(ec, L.ec_masked_select(U8, one_d.ptr("a"), one_d.ptr("ma"), one_d.ptr("a2"), one_d.ptr("mb"), sel.mem.ptr, n, out.mem.ptr, om.mem.ptr, ec.stream()))
        for k, (off, ln) in enumerate(one_d.spots):
            assert np.array_equal(sel.shard(off, ln).to_numpy(), hsel[k])
            cells, mask = CMP.masked_select(hsel[k], at["a"][k], at["ma"][k], at["a2"][k], at["mb"][k])
            same(out.shard(off, ln).to_numpy(), cells, np.uint8(255), ("masked_select", off))
            same(om.shard(off, ln).to_numpy(), mask, MASK_PRE, ("masked_select mask", off))

    @pytest.mark.parametrize("mode", cast_ref.MODES, ids=("as", "round"))
    def test_cast_u8_to_i8(self, ec, one_d, mode):
        out = filled(ec, I8, one_d.n, 0)   # cells are 1 .. 200: neither the wrap nor the clamp gives 0
        chk(ec, ec.lib().ec_cast(mode, U8, one_d.ptr("a"), I8, out.mem.ptr, one_d.n, ec.stream()))
        one_d.check(out, lambda k: cast_ref.cast(mode, U8, one_d.at["a"][k], I8), np.int8(0), ("cast", mode))

    def test_cast_scaled_u8_to_i16_under_a_mask(self, ec, one_d):
        out = filled(ec, I16, one_d.n, 32767)
        nd = ec.CellValue(I16, -32768).to_ec()
        chk(ec, ec.lib().ec_cast_scaled(U8, one_d.ptr("a"), one_d.ptr("ma"), one_d.n, 10.0, -1.0, I16, C.byref(nd), out.mem.ptr, ec.stream()))
        one_d.check(out, lambda k: cast_ref.scaled(U8, one_d.at["a"][k], one_d.at["ma"][k], 10.0, -1.0, I16, -32768), np.int16(32767), "cast_scaled")

    def test_classify_with_three_breaks(self, ec, one_d):
        breaks = np.array([50, 100, 150], np.uint8)
        table = ec.ReclassTable(U8, breaks, np.array([0, 1, 2, 3], np.uint8))
        out = filled(ec, U8, one_d.n, 255)
        chk(ec, ec.lib().ec_reclass(U8, one_d.ptr("a"), None, one_d.n, U8, table.mem.ptr, out.mem.ptr, None, ec.stream()))
        one_d.check(out, lambda k: RC.reclass(U8, one_d.at["a"][k], None, U8, breaks, False, U8, [0, 1, 2, 3])[0], np.uint8(255), "classify")

    def test_reclassify_under_a_mask_with_a_dropped_class(self, ec, one_d):
        breaks, values, valid = np.array([50, 100, 150], np.uint8), np.array([10, 20, 65000, 40], np.uint16), [1, 1, 0, 1]
        table = ec.ReclassTable(U8, breaks, values, valid=valid, nodata=65000)
        out, om = filled(ec, U16, one_d.n, 65535), filled_mask(ec, one_d.n)
        chk(ec, ec.lib().ec_reclass(U8, one_d.ptr("a"), one_d.ptr("ma"), one_d.n, U16, table.mem.ptr, out.mem.ptr, om.mem.ptr, ec.stream()))
        exp = [RC.reclass(U8, one_d.at["a"][k], one_d.at["ma"][k], U8, breaks, False, U16, values, valid, 65000) for k in range(len(one_d.spots))]
        one_d.check(out, lambda k: exp[k][0], np.uint16(65535), "reclassify")
        one_d.check(om, lambda k: exp[k][1], MASK_PRE, "reclassify mask")

    def test_zonal_broadcast_into_u16(self, ec, one_d):
        n = one_d.n
        zones = stream_buf(ec, "zones", n)   # ids 0 .. 5 against 4 zones: 4 and 5 belong to none
        table = np.array([1000, 2000, 3000, 4000], np.uint16)
        tab = ec.CellBuffer.from_vec(table)
        out, om = filled(ec, U16, n, 65535), filled_mask(ec, n)
        chk(ec, ec.lib().ec_zonal_broadcast(U8, zones.mem.ptr, n, 4, U16, tab.mem.ptr, out.mem.ptr, om.mem.ptr, ec.stream()))
        for off, ln in one_d.spots:
            z = stream_host("zones", off, ln)
            assert np.array_equal(zones.shard(off, ln).to_numpy(), z)
            ok = z < 4
            same(out.shard(off, ln).to_numpy(), np.where(ok, table[np.minimum(z, 3)], np.uint16(0)), np.uint16(65535), ("broadcast", off))
            same(om.shard(off, ln).to_numpy(), ok.astype(np.uint8), MASK_PRE, ("broadcast mask", off))

    def test_composite_max_with_aux_over_two_layers(self, ec, one_d):
        n = one_d.n
        out, aux = filled(ec, U8, n, 255), filled(ec, U8, n, 77)
        lp = (C.c_void_p * 2)(one_d.ptr("a"), one_d.ptr("a2"))
        chk(ec, ec.lib().ec_composite(COMP.MAX, U8, lp, None, 2, n, 1, out.mem.ptr, None, aux.mem.ptr, ec.stream()))
        exp = [COMP.composite(COMP.MAX, U8, [one_d.at["a"][k], one_d.at["a2"][k]], None, 1) for k in range(len(one_d.spots))]
        one_d.check(out, lambda k: exp[k][0].astype(np.uint8), np.uint8(255), "composite max")
        one_d.check(aux, lambda k: exp[k][2], np.uint8(77), "composite aux")

    def test_composite_median_over_three_masked_layers(self, ec, one_d):
        n = one_d.n
        out, om = filled(ec, U8, n, 255), filled_mask(ec, n)
        names = (("a", "ma"), ("a2", "mb"), ("a", "mb"))
        lp = (C.c_void_p * 3)(*[one_d.ptr(c) for c, _ in names])
        mp = (C.c_void_p * 3)(*[one_d.ptr(m) for _, m in names])
        chk(ec, ec.lib().ec_composite_rank(U8, lp, mp, 3, n, 1, 2, RANK.LOWER, 1, out.mem.ptr, om.mem.ptr, None, ec.stream()))
        exp = [RANK.composite_rank(U8, [one_d.at[c][k] for c, _ in names], [one_d.at[m][k] for _, m in names], 1, 2, RANK.LOWER, 1)
               for k in range(len(one_d.spots))]
        one_d.check(out, lambda k: exp[k][0], np.uint8(255), "composite median")
        one_d.check(om, lambda k: exp[k][1], MASK_PRE, "composite median mask")

    def test_mask_and_or_not_and_mask_select(self, ec, one_d):
        L, n, at = ec.lib(), one_d.n, one_d.at
        for call, ref in ((L.ec_mask_and, eco.mask_and), (L.ec_mask_or, eco.mask_or)):
            out = filled_mask(ec, n)
            chk(ec, call(one_d.ptr("ma"), one_d.ptr("mb"), n, out.mem.ptr, ec.stream()))
            one_d.check(out, lambda k: ref(at["ma"][k], at["mb"][k]), MASK_PRE, ref.__name__)
        out = filled_mask(ec, n)
        chk(ec, L.ec_mask_not(one_d.ptr("ma"), n, out.mem.ptr, ec.stream()))
        one_d.check(out, lambda k: eco.mask_not(at["ma"][k]), MASK_PRE, "mask_not")
        out = filled(ec, U8, n, 255)
        nd = ec.CellValue(U8, 250).to_ec()
        chk(ec, L.ec_mask_select(U8, one_d.ptr("a"), one_d.ptr("ma"), n, C.byref(nd), out.mem.ptr, ec.stream()))
        one_d.check(out, lambda k: eco.mask_select(at["a"][k], at["ma"][k], eco.ND_VALUE, eco.Value.of(eco.U8, 250)), np.uint8(255), "mask_select")

    def test_ndvi_fused_and_as_a_program_on_the_interpreter_and_the_built_in_kernel(self, ec, one_d):
        """(a - a2) / (a + a2) over u8 into 34 GB of f64, three ways, each into the same pre-filled buffer.  The three are compared with
        the oracle at the spots; two 34 GB results side by side would pass the 64 GiB cap, so they are not compared with each other."""
        L, n, at = ec.lib(), one_d.n, one_d.at
        exp = [eco.f_binop(eco.DIV, eco.f_binop(eco.SUB, at["a"][k], at["a2"][k]), eco.f_binop(eco.ADD, at["a"][k], at["a2"][k])) for k in range(len(one_d.spots))]
        out = ec.CellBuffer.empty(n, F64)
        nan = ec.CellValue(F64, float("nan")).to_ec()

        def refill():
            chk(ec, L.ec_fill(F64, out.mem.ptr, n, C.byref(nan), ec.stream()))
            return prefill_of(out)

        def stat(key):
            v = C.c_int64(0)
            chk(ec, L.ec_stat_get(key, C.byref(v)))
            return v.value

        pre = refill()
        dt = (C.c_uint8 * 4)(U8, U8, U8, U8)
        p = (C.c_void_p * 4)(one_d.ptr("a"), one_d.ptr("a2"), one_d.ptr("a"), one_d.ptr("a2"))
        chk(ec, L.ec_fused(ec.SUB, ec.DIV, ec.ADD, dt, p, None, n, out.mem.ptr, ec.stream()))
        one_d.check(out, lambda k: exp[k], pre, "fused ndvi")
        from erased_cells_hip._ffi import EcExprStep
        steps = (EcExprStep * 3)(EcExprStep(ec.SUB, 0, 1, 0), EcExprStep(ec.ADD, 0, 1, 1), EcExprStep(ec.DIV, 4, 5, 0))
        dt2, p2 = (C.c_uint8 * 2)(U8, U8), (C.c_void_p * 2)(one_d.ptr("a"), one_d.ptr("a2"))
        sc = (ec._ffi.EcValue * 1)()
        try:
            L.ec_tune_set(b"expr_jit", 0)
            for fixed, key in ((1, b"expr_fixed_launches"), (0, b"expr_interp_launches")):
                L.ec_tune_set(b"expr_fixed", fixed)
                pre, before = refill(), stat(key)
                chk(ec, L.ec_expr(dt2, p2, 2, sc, 0, steps, 3, n, out.mem.ptr, ec.stream()))
                assert stat(key) == before + 1
                one_d.check(out, lambda k: exp[k], pre, ("expr", key))
        finally:
            L.ec_tune_set(b"expr_jit", 1)
            L.ec_tune_set(b"expr_fixed", 1)

    def test_first_difference_and_buffer_cmp_report_a_cell_past_2_32(self, ec, one_d):
        L, n = ec.lib(), one_d.n
        other = one_d.dev["a"].clone()
        idx, order = C.c_uint64(0), C.c_int32(7)
        chk(ec, L.ec_first_difference(U8, one_d.ptr("a"), other.mem.ptr, n, C.byref(idx), ec.stream()))
        assert idx.value == n
        chk(ec, L.ec_buffer_cmp(U8, one_d.ptr("a"), n, U8, other.mem.ptr, n, C.byref(order), ec.stream()))
        assert order.value == 0
        at = K.TWO32 + 17
        was = int(one_d.dev["a"].get(at).value)
        assert was == int(stream_host("a", at, 1)[0])
        other.put(at, ec.CellValue(U8, was + 1))
        chk(ec, L.ec_first_difference(U8, one_d.ptr("a"), other.mem.ptr, n, C.byref(idx), ec.stream()))
        assert idx.value == at
        chk(ec, L.ec_buffer_cmp(U8, one_d.ptr("a"), n, U8, other.mem.ptr, n, C.byref(order), ec.stream()))
        assert order.value == -1
        chk(ec, L.ec_buffer_cmp(U8, other.mem.ptr, n, U8, one_d.ptr("a"), n, C.byref(order), ec.stream()))
        assert order.value == 1


def test_f64_output_past_2_31_and_2_32_bytes(ec):
    """n = 2^29 + 4101 u16 cells scaled into f64: the output's byte offset passes 2^31 at cell 2^28 and 2^32 at cell 2^29"""
    n, spots = K.N_F64, K.f64_spots()
    inp = Inputs(ec, n, ("wide",), spots)
    out = nan_filled(ec, n)
    pre = prefill_of(out)
    chk(ec, ec.lib().ec_cast_scaled(U16, inp.ptr("wide"), None, n, 0.37, 100.25, F64, None, out.mem.ptr, ec.stream()))
    inp.check(out, lambda k: cast_ref.scaled(U16, inp.at["wide"][k], None, 0.37, 100.25, F64), pre, "cast_scaled u16 -> f64")


# ------------------------------------------------------------------------------------------------------------ reductions
def plant(ec, buf, blocks, cells_of):
    """uploads cells_of(off, ln) over each block of `buf`; -> the host blocks"""
    out = []
    for off, ln in blocks:
        h = np.ascontiguousarray(cells_of(off, ln))
        part = buf.shard(off, ln)
        chk(ec, ec.lib().ec_upload(part.mem.ptr, h.ctypes.data_as(C.c_void_p), h.nbytes, ec.stream()))
        out.append(h)
    ec.synchronize()
    return out


def stats_of(ec, s):
    return {"count": int(s.count), "min": ec.CellValue.from_ec(s.min).value, "max": ec.CellValue.from_ec(s.max).value, "sum": float(s.sum),
            "mean": float(s.mean), "stddev": float(s.stddev)}


def same_stats(got, exp, what):
    assert got["count"] == exp["count"] and got["min"] == exp["min"] and got["max"] == exp["max"], (what, got, exp)
    for key in ("sum", "mean", "stddev"):
        assert np.float64(got[key]).view(np.uint64) == np.float64(exp[key]).view(np.uint64), (what, key, got, exp)


def test_stats_of_2_32_u8_cells_the_accepted_maximum(ec):
    """a constant raster with three hashed blocks (at 0, over cell 2^32 - 1 which is the tail): the record is the constant's closed form plus
    stats_ref.record of the blocks, in exact integers"""
    L, n, const = ec.lib(), K.TWO32, 7
    buf = filled(ec, U8, n, const)
    blocks = K.blocks(n)
    hs = plant(ec, buf, blocks, lambda off, ln: stream_host("a", off, ln))
    rb = SR.record(SR.U8, np.concatenate(hs).tolist())
    cnt, s1, s2 = K.constant_moments(const, n - rb["count"])
    exp = dict(rb, count=n, sum=rb["sum"] + s1, sq=rb["sq"] + s2, min=min(rb["min"], const), max=max(rb["max"], const))
    assert cnt + rb["count"] == n
    rec_dev = ec.DeviceMem(64)
    chk(ec, L.ec_stats_device(U8, buf.mem.ptr, None, n, rec_dev.ptr, ec.stream()))
    rec = ec._ffi.EcMoments()
    chk(ec, L.ec_download(C.byref(rec), rec_dev.ptr, 64, ec.stream()))
    assert (rec.count, rec.kind, rec.dtype, rec.reserved) == (n, 0, U8, 0)
    assert (~rec.keys2[0], rec.keys2[1]) == (exp["min"], exp["max"])
    assert (rec.u.i.sum, rec.u.i.sq_lo + (rec.u.i.sq_hi << 64)) == (exp["sum"], exp["sq"])
    st = ec._ffi.EcStats()
    chk(ec, L.ec_stats_compute(U8, buf.mem.ptr, None, n, C.byref(st), ec.stream()))
    same_stats(stats_of(ec, st), SR.fold([exp]), "stats u8")
    assert L.ec_stats_compute(U8, buf.mem.ptr, None, n + 1, C.byref(st), ec.stream()) == ARG   # one more is refused: the documented bound


def test_stats_of_65537_squared_f32_cells(ec):
    """f32 cells that are integers within 512 of the pivot (cell 0): every partial sum of d and d * d is an exact integer below 2^53, so
    the record is the same in any order"""
    L, n, const = ec.lib(), K.N, 1000.0
    F32 = SR.F32
    buf = filled(ec, F32, n, const)
    blocks = K.blocks(n)
    hs = plant(ec, buf, blocks, lambda off, ln: (stream_host("b", off, ln).astype(np.float32) + np.float32(const - 200.0)))
    cells = np.concatenate(hs).astype(np.float64)
    pivot = float(hs[0][0])
    assert np.abs(cells - pivot).max() <= 512 and abs(const - pivot) <= 512
    d = (cells - pivot).astype(np.int64)
    dc, rest = int(const - pivot), n - cells.size
    s1, s2 = int(d.sum()) + dc * rest, int((d * d).sum()) + dc * dc * rest
    assert abs(s1) < 2 ** 53 and s2 < 2 ** 53
    mn, mx = float(min(cells.min(), const)), float(max(cells.max(), const))
    exp = {"count": n, "kind": 1, "dtype": F32, "min": mn, "max": mx, "pivot": pivot, "s1": float(s1), "s2": float(s2)}
    rec_dev = ec.DeviceMem(64)
    chk(ec, L.ec_stats_device(F32, buf.mem.ptr, None, n, rec_dev.ptr, ec.stream()))
    rec = ec._ffi.EcMoments()
    chk(ec, L.ec_download(C.byref(rec), rec_dev.ptr, 64, ec.stream()))
    assert (rec.count, rec.kind, rec.dtype) == (n, 1, F32)
    assert (~rec.keys2[0], rec.keys2[1]) == (SR.order_key(F32, mn), SR.order_key(F32, mx))
    assert (rec.u.f.pivot, rec.u.f.s1, rec.u.f.s2) == (pivot, float(s1), float(s2))
    st = ec._ffi.EcStats()
    chk(ec, L.ec_stats_compute(F32, buf.mem.ptr, None, n, C.byref(st), ec.stream()))
    same_stats(stats_of(ec, st), SR.fold([exp]), "stats f32")


def test_zonal_stats_of_2_32_cells(ec):
    """values and zones constant but for the same three blocks: zone 0 holds the constant cells and its share of the blocks, zones 1 .. 3
    only block cells"""
    L, n, const, zones_n = ec.lib(), K.TWO32, 7, 4
    vals, zones = filled(ec, U8, n, const), filled(ec, U8, n, 0)
    blocks = K.blocks(n)
    hv = np.concatenate(plant(ec, vals, blocks, lambda off, ln: stream_host("a", off, ln)))
    hz = np.concatenate(plant(ec, zones, blocks, lambda off, ln: stream_host("classes", off, ln)))
    out = (ec._ffi.EcStats * zones_n)()
    chk(ec, L.ec_zonal_stats_compute(U8, vals.mem.ptr, None, U8, zones.mem.ptr, n, zones_n, out, ec.stream()))
    for z in range(zones_n):
        r = SR.record(SR.U8, hv[hz == z].tolist())
        assert r["count"] > 100
        if z == 0:
            cnt, s1, s2 = K.constant_moments(const, n - hv.size)
            r = dict(r, count=r["count"] + cnt, sum=r["sum"] + s1, sq=r["sq"] + s2, min=min(r["min"], const), max=max(r["max"], const))
        same_stats(stats_of(ec, out[z]), SR.fold([r]), ("zonal", z))
    assert sum(int(out[z].count) for z in range(zones_n)) == n


# ------------------------------------------------------------------------------------------------------------ 2-D families
def sub_raster(fetch, cols, box):
    y0, x0, h, w = box
    return np.stack([fetch(y * cols + x0, w) for y in range(y0, y0 + h)])


@pytest.fixture(scope="class")
def two_d(ec):
    inp = Inputs(ec, K.N, ("a", "ma", "classes"), K.spots())
    yield inp
    inp.dev.clear()


class TestMovingWindowsOn65537Squared:
    """65537 x 65537 u8: the windows of tests/large_cases.py — the corners, the first rows, and the last rows, where y * cols passes 2^32"""

    def run(self, ec, two_d, what, src, mask, radius, flags, want_mask, weights=None):
        cols = rows = K.SIDE
        n = cols * rows
        summing = what in (F.SUM, F.MEAN, "convolve")
        out = nan_filled(ec, n) if summing else filled(ec, U8, n, 255)
        om = filled_mask(ec, n) if want_mask else None
        pre = prefill_of(out)
        smask = two_d.dev[mask] if mask else None
        assert focal_call(ec, what, U8, two_d.dev[src], smask, cols, rows, radius, flags, out, om, weights) == OK
        rx, ry = radius
        for win in K.windows():
            box, (dy, dx) = K.enlarged(win, rx, ry, cols, rows)
            ha = sub_raster(lambda off, ln: stream_host(src, off, ln), cols, box)
            assert np.array_equal(sub_raster(lambda off, ln: two_d.dev[src].shard(off, ln).to_numpy(), cols, box), ha)
            hm = None
            if mask:
                hm = sub_raster(lambda off, ln: stream_host(mask, off, ln), cols, box)
                assert np.array_equal(sub_raster(lambda off, ln: smask.shard(off, ln).to_numpy(), cols, box), hm)
            exp, ev = focal_expected(what, ha, hm, radius, flags, weights)
            y0, x0, h, w = win
            same(sub_raster(lambda off, ln: out.shard(off, ln).to_numpy(), cols, win), exp[dy:dy + h, dx:dx + w], pre, (what, win))
            if om is not None:
                same(sub_raster(lambda off, ln: om.shard(off, ln).to_numpy(), cols, win), ev[dy:dy + h, dx:dx + w], MASK_PRE, (what, win, "mask"))

    def test_focal_max_masked(self, ec, two_d):
        self.run(ec, two_d, F.MAX, "a", "ma", (2, 3), 0, True)

    def test_focal_sum_unmasked(self, ec, two_d):
        self.run(ec, two_d, F.SUM, "a", None, (2, 3), 0, False)

    def test_convolve_3x3_whole(self, ec, two_d):
        self.run(ec, two_d, "convolve", "a", None, (1, 1), WHOLE, True, WEIGHTS3)

    def test_focal_median_3x3(self, ec, two_d):
        self.run(ec, two_d, "median", "a", None, (1, 1), 0, False)

    def test_focal_majority_3x3_on_four_classes(self, ec, two_d):
        self.run(ec, two_d, "majority", "classes", None, (1, 1), 0, False)

    def test_mask_dilate(self, ec, two_d):
        """Mask.dilate is ec_focal MAX over the mask's bytes as u8 cells: the same call, into a pre-filled mask"""
        cols = rows = K.SIDE
        out = filled_mask(ec, cols * rows)
        src = two_d.dev["ma"]
        chk(ec, ec.lib().ec_focal(F.MAX, U8, src.mem.ptr, None, cols, rows, 1, 1, 0, out.mem.ptr, None, ec.stream()))
        for win in K.windows():
            box, (dy, dx) = K.enlarged(win, 1, 1, cols, rows)
            hm = sub_raster(lambda off, ln: stream_host("ma", off, ln), cols, box)
            exp, _ = F.focal(F.MAX, hm, None, 1, 1)
            y0, x0, h, w = win
            same(sub_raster(lambda off, ln: out.shard(off, ln).to_numpy(), cols, win), exp[dy:dy + h, dx:dx + w], MASK_PRE, ("dilate", win))


@pytest.mark.parametrize("alg,out_cols", [(RS.AVERAGE, 1024), (RS.BILINEAR, 1500)], ids=("average-by-4", "bilinear"))
def test_resample_reads_a_window_that_straddles_cell_2_32(ec, alg, out_cols):
    """a one-row raster of 2^32 + 4101 columns; 4096 cells from 2^32 - 2048 delivered as 1024 (an average of 4) and as 1500 (bilinear)"""
    cols = K.RESAMPLE_COLS
    x0, w = K.RESAMPLE_WINDOW
    ct, seed, lo, hi = K.STREAMS["a"]
    src = synth(ec, U8, cols, seed, lo, hi)
    h = host(U8, x0, w, seed, lo, hi)
    assert np.array_equal(src.shard(x0, w).to_numpy(), h)
    out = filled(ec, U8, out_cols, 255)   # no source mask, so no result mask: the entry point takes both or neither
    chk(ec, ec.lib().ec_window_resample(alg, U8, src.mem.ptr, None, cols, 1, x0, 0, w, 1, out_cols, 1, out.mem.ptr, None, ec.stream()))
    exp, ev = RS.resample(alg, h.reshape(1, w), None, 0, 0, w, 1, out_cols, 1)
    assert ev.all()
    same(out.to_numpy(), exp, np.uint8(255), ("resample", alg))


# ------------------------------------------------------------------------------------------------------------ ec_distance at its maximum
def distance_mask(ec, name, side):
    m = ec.Mask.fill(side * side, False)
    t = K.distance_targets(name, side)
    if t == "top_row":
        one = ec.CellValue(U8, 1).to_ec()
        chk(ec, ec.lib().ec_fill(U8, m.mem.ptr, side, C.byref(one), ec.stream()))
    else:
        for y, x in t:
            m.put(y * side + x, True)
    return m


def column_of(ec, ct, mem, side, x):
    """column x of a side x side raster as one array: cut on the device (ec_window), one download"""
    return ec.CellBuffer(ct, side * side, mem).window(side, window=(x, 0), window_size=(1, side)).to_numpy()


# (mask, max_sq or None, output type or None for the `within` form, the caller's workspace or the pooled one)
DISTANCE_CASES = [("corner", None, U32, True), ("two_corners", None, F64, False), ("top_row", None, U32, False), ("corner", K.DIST_MAX_SQ, F64, True),
                  ("two_corners", K.DIST_MAX_SQ, None, False)]


@pytest.mark.parametrize("case", DISTANCE_CASES, ids=[f"{c[0]}-{'cut' if c[1] else 'unlimited'}-{ {U32: 'u32', F64: 'f64', None: 'within'}[c[2]] }-{'own' if c[3] else 'pooled'}-workspace" for c in DISTANCE_CASES])
def test_distance_at_32768_squared(ec, case):
    """both axes at EC_DISTANCE_MAX_SIDE: d2 up to 2 * 32767^2, a workspace of gigabytes, 4 and 8 GiB of output; whole rows 0, 1, 16383,
    16384, 32766, 32767 and whole columns 0 and 32767 against the closed forms"""
    name, max_sq, out_type, own = case
    L, side = ec.lib(), K.DIST_SIDE
    n = side * side
    mask = distance_mask(ec, name, side)
    ws = ec.DeviceMem(L.ec_distance_workspace_bytes(side, side)) if own else None
    out = None if out_type is None else (nan_filled(ec, n) if out_type == F64 else filled(ec, U32, n, 0xFFFFFFFF))
    om = filled_mask(ec, n)
    pre = prefill_of(out) if out is not None else None
    chk(ec, L.ec_distance(mask.mem.ptr, side, side, max_sq if max_sq is not None else 0xFFFFFFFF, out_type if out_type is not None else U32,
                          out.mem.ptr if out is not None else None, om.mem.ptr, ws.ptr if ws is not None else None, ec.stream()))
    f64 = out_type == F64
    for r in K.DIST_LINES_ROWS:
        ys, xs = np.full(side, r, np.int64), np.arange(side, dtype=np.int64)
        cells, valid = K.distance_expected(name, ys, xs, max_sq, f64)
        if out is not None:
            same(out.shard(r * side, side).to_numpy(), cells, pre, (case, "row", r))
        same(om.shard(r * side, side).to_numpy(), valid, MASK_PRE, (case, "row", r, "mask"))
    for c in K.DIST_LINES_COLS:
        ys, xs = np.arange(side, dtype=np.int64), np.full(side, c, np.int64)
        cells, valid = K.distance_expected(name, ys, xs, max_sq, f64)
        if out is not None:
            same(column_of(ec, out_type, out.mem, side, c), cells, pre, (case, "column", c))
        same(column_of(ec, U8, om.mem, side, c), valid, MASK_PRE, (case, "column", c, "mask"))
