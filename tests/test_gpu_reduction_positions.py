"""The reductions against the oracle on inputs in which ONE cell holds each answer, planted at every place the kernel geometry
distinguishes (tests/reduction_cases.py: element slots, lanes, waves, in-flight loads, tile edges, the partial tile, the ragged
tail, the peeled head, workgroups, the finalize kernel's load slots, later rounds of the grid-stride loop).  The expected value
of every case is what the oracle returns for the same host array, and before the GPU is asked the oracle's answer is asserted to
BE the planted pair.  Everything is compared on bits and cell type; there is no tolerance.  One device buffer per (type, field):
windows are 16-byte-aligned shards of it (or start a chosen number of cells before a boundary), plants are written in place and
put back.  tests/test_reduction_inputs.py shows on the CPU that each fault model changes the answer of one of these cases."""
import ctypes as C
import os
from contextlib import contextmanager

import numpy as np
import pytest

import reduction_cases as rc
from oracle import eco

pytestmark = pytest.mark.gpu

NT = eco.NTYPES
S, R, K = (lambda k: k), (lambda k: 4 + k), (lambda k: 8 + k)


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


@pytest.fixture(scope="module")
def cus(ec):
    n = C.c_int32()
    ec._ffi.check(ec.lib().ec_device_info(C.byref(n), None, None, 0))
    return n.value


class DevPool:
    """reduction_cases.HostPool with its device twins."""

    def __init__(self, ec, ct, n, seed=5, kind="adjacent", masked=True):
        self.ec, self.ct = ec, ct
        self.host = rc.HostPool(ct, n, seed, kind, masked)
        self.plain = ec.CellBuffer.from_vec(self.host.plain)
        assert self.plain.mem.ptr % 16 == 0
        self.hidden = ec.CellBuffer.from_vec(self.host.hidden) if masked else None
        self.mask = ec.Mask.new(self.host.mask) if masked else None

    def _upload(self, mem, itemsize, dtype, off, edits):
        for start, vals in rc.runs(edits):
            a = np.array(vals, dtype=dtype)
            self.ec._ffi.check(self.ec.lib().ec_upload(mem.window((off + start) * itemsize, a.nbytes).ptr, a.ctypes.data_as(C.c_void_p), a.nbytes,
                                                      self.ec.buffer.stream()))

    @contextmanager
    def planted(self, ge, cells_edits, mask_edits, masked):
        """The edits (window indices -> bits) in the host arrays and on the device, put back on exit."""
        h = self.host
        off = h.offset(ge)
        hc, hm = h.arrays(masked)
        dc = self.hidden if masked else self.plain
        sz = hc.dtype.itemsize
        old_c = h.poke(hc, off, cells_edits)
        old_m = h.poke(hm, off, mask_edits) if masked else {}
        self._upload(dc.mem, sz, rc._UINT[sz], off, cells_edits)
        if masked:
            self._upload(self.mask.mem, 1, np.uint8, off, mask_edits)
        try:
            yield hc[off:off + ge.n], (hm[off:off + ge.n] if masked else None), dc.shard(off, ge.n), (self.mask.shard(off, ge.n) if masked else None)
        finally:
            h.poke(hc, off, old_c)
            self._upload(dc.mem, sz, rc._UINT[sz], off, old_c)
            if masked:
                h.poke(hm, off, old_m)
                self._upload(self.mask.mem, 1, np.uint8, off, old_m)


def _run_min_max(ec, pool, cases, context, api="min_max"):
    """Every case through the oracle (premise: it returns the planted pair) and the GPU; the failures of the group in one assert."""
    ct, bad = pool.ct, []
    for c in cases:
        ce, me, want = rc.case_edits(ct, c, pool.host.block)
        with pool.planted(c.window.ge, ce, me, c.masked) as (ha, hm, da, dm):
            emn, emx = eco.f_min_max(ha, hm)
            exp = (emn.bits(), emx.bits())
            for side in (0, 1):
                assert want[side] is None or exp[side] == want[side], f"generator: the oracle does not return the plant: {c.label()} {exp} {want}"
            mn, mx = (ec.MaskedCellBuffer(da, dm) if c.masked else da).min_max()
        got = (mn.bits(), mx.bits())
        if (mn.ct, mx.ct) != (ct, ct) or got != exp:
            bad.append(f"{eco.CT_NAMES[ct]} {context} {c.label()}: expected ({exp[0]:#x}, {exp[1]:#x}) got ({got[0]:#x}, {got[1]:#x})")
    print(f"reduction cases: {api} {eco.CT_NAMES[ct]} {context} {len(cases)}")
    assert not bad, f"{len(bad)} of {len(cases)} cases differ:\n" + "\n".join(bad[:12])


def _pool_for(ec, ct, cases, **kw):
    return DevPool(ec, ct, max(c.window.ge.n + c.window.ge.cpl for c in cases) + 2, **kw)


# ---------------------------------------------------------------- min_max: the vector kernel under every launch shape
@pytest.mark.parametrize("ct", range(NT))
def test_min_max_every_position_every_shape(ec, ct):
    """All ten types, plain and masked with decoys, every position class of every window (n in {1, 2, CPL-1, CPL, CPL+1}, the
    single-workgroup shortcut, two workgroups, 2.5 tiles with a full tail, every head length, 66 workgroups) at each reduce_shape."""
    by_shape = {shape: rc.min_max_cases(ct, shape) for shape in rc.SHAPES}
    pool = _pool_for(ec, ct, [c for cs in by_shape.values() for c in cs])
    for shape, cases in by_shape.items():
        with ec.tuned(reduce_shape=shape):
            _run_min_max(ec, pool, cases, f"reduce_shape={shape}")


@pytest.mark.parametrize("ct", range(NT))
def test_min_max_order_kinds(ec, ct):
    """The order itself: MIN / MAX, values adjacent to the band, the pairs f64 cannot tell apart, +-inf, NaNs of both signs with two
    payloads, signed zeros, subnormals — at one element slot, the tail, the head and the partial tile; once more with every load nt."""
    cases = rc.order_cases(ct)
    for kind in rc.kinds_of(ct):
        ks = [c for c in cases if c.kind == kind]
        pool = _pool_for(ec, ct, ks, kind=kind)
        _run_min_max(ec, pool, ks, "order kinds")
        if kind == "adjacent":
            with ec.tuned(mall_mb=0):
                _run_min_max(ec, pool, ks, "mall_mb=0")


@pytest.mark.parametrize("ct", range(NT))
def test_min_max_capped_grids_and_the_cellwise_kernel(ec, cus, ct):
    """Default shape under reduce_bpc = 1 (a window of 2 x CUs + 3 tiles: tiles only the second and the last round reach) and
    reduce_bpc = 100 (4096 workgroups: partial words 1023, 1024, 2047, 2048, 3071, 3072 and the last, i.e. the finalize kernel's four
    load slots and their wave boundaries); the cell-wise kernel (unaligned_vector = 0 at an odd offset) over its own classes."""
    cases = rc.capped_cases(ct, cus) + rc.cellwise_cases(ct, cus)
    pool = _pool_for(ec, ct, cases)
    for knobs in sorted({c.window.knobs for c in cases}):
        with ec.tuned(**dict(knobs)):
            _run_min_max(ec, pool, [c for c in cases if c.window.knobs == knobs], str(dict(knobs)))
    with ec.tuned(reduce_bpc=100):   # the small windows under the other two reduce_bpc values
        small = [c for c in rc.min_max_cases(ct, 0) if c.window.name in ("main", "two_workgroups_ragged", "head=1")]
        _run_min_max(ec, pool, small, "reduce_bpc=100")
        with ec.tuned(reduce_bpc=1):
            _run_min_max(ec, pool, small, "reduce_bpc=1")


# ---------------------------------------------------------------- first_difference / cmp
def _first_difference(ec, ct, a, b, n):
    idx = C.c_uint64()
    ec._ffi.check(ec.lib().ec_first_difference(ct, a.mem.ptr, b.mem.ptr, n, C.byref(idx), ec.buffer.stream()))
    return idx.value


@pytest.mark.parametrize("ct", [eco.U8, eco.I16, eco.F32, eco.U64])
def test_first_difference_every_position(ec, cus, ct):
    """Cell widths 1, 2, 4, 8: a sole difference at every position class (default grid, reduce_bpc 1 and 100, the cell-wise form), two
    differences of which the later one sits where the kernel looks first (a lower lane, an earlier load, a lower workgroup, the body
    against the head): the smaller index must come back, and `cmp` must order the buffers as the oracle does.  Equal at each length."""
    size = rc.dtype_of(ct).itemsize
    windows = [(w, ()) for w in rc.min_max_windows(size, 0)] + [(w, w.knobs) for w in rc.capped_windows(size, cus)]
    cw = rc.cellwise_window(size, cus)
    windows.append((rc.Window("cellwise", rc.Geometry(cw.ge.n, size, rc.RBLOCK, 1, 0, 4 * cus, 1), cw.classes), cw.knobs))
    nmax = max(w.ge.n for w, _ in windows) + 40
    host = rc.HostPool(ct, nmax, 8, masked=False)
    ha = host.plain
    da = ec.CellBuffer.from_vec(ha)
    db = da.clone()
    hb = ha.copy()
    U = rc._UINT[size]
    bad, ncases = [], 0

    def put(i, bits):
        rc.as_bits(hb)[i] = bits
        x = np.array([bits], U)
        ec._ffi.check(ec.lib().ec_upload(db.mem.window(i * size, size).ptr, x.ctypes.data_as(C.c_void_p), size, ec.buffer.stream()))

    for w, knobs in windows:
        ge = w.ge
        off = host.offset(ge)
        pos = rc.window_positions(w if ge.n > ge.cpl + 1 else rc.Window(w.name, ge, ("*",)))
        wa, wb, xa, xb = ha[off:off + ge.n], hb[off:off + ge.n], da.shard(off, ge.n), db.shard(off, ge.n)
        with ec.tuned(**dict(knobs)):
            assert _first_difference(ec, ct, xa, xb, ge.n) == ge.n and xa.cmp(xb) == eco.buffer_cmp(wa, wb) == 0, (w.name, "equal")
            plans = [((nm, i), ()) for nm, i in pos]
            # two differences, the later one where the kernel looks no later than at the first (rc.later_first_pairs, by construction)
            plans += [((nm, i), (later,)) for nm, i, later in rc.later_first_pairs(ge)]
            for (nm, i), later in plans:
                for q in (i,) + tuple(later):   # rc.sole_difference, cell by cell: cell i the larger in b, the later ones the smaller
                    put(off + q, rc.differing_bits(wa, q, q == i))
                exp_idx = i   # by construction; the oracle confirms it: cell i is the larger in b, every later difference the smaller
                got_idx, got_cmp, exp_cmp = _first_difference(ec, ct, xa, xb, ge.n), xa.cmp(xb), eco.buffer_cmp(wa, wb)
                assert exp_cmp == -1 and (ge.n > 1 << 22 or int(np.flatnonzero(rc.as_bits(wa) != rc.as_bits(wb))[0]) == i)
                for q in (i,) + tuple(later):
                    put(off + q, int(rc.as_bits(wa)[q]))
                ncases += 1
                if (got_idx, got_cmp) != (exp_idx, exp_cmp):
                    bad.append(f"{eco.CT_NAMES[ct]} {w.name} {dict(knobs)} {nm}[{i}] later {later}: expected index {exp_idx} cmp {exp_cmp}, got {got_idx} cmp {got_cmp}")
    print(f"reduction cases: first_difference/cmp {eco.CT_NAMES[ct]} {ncases}")
    assert not bad, f"{len(bad)} of {ncases} cases differ:\n" + "\n".join(bad[:12])


# ---------------------------------------------------------------- mask_counts / all
def test_mask_counts_every_position(ec, cus):
    """A sole true and a sole false cell at every position class through counts_one_launch 0, 1 and 2, single-workgroup and
    multi-workgroup lengths alternating on one stream (the ticket word must be back at zero between kernels of different grids),
    the capped grids under reduce_bpc 1 and 100, and the cell-wise form."""
    windows = [(w, ()) for w in rc.min_max_windows(1, 0)] + [(w, w.knobs) for w in rc.capped_windows(1, cus)]
    cw = rc.cellwise_window(1, cus)
    windows.append((rc.Window("cellwise", rc.Geometry(cw.ge.n, 1, rc.RBLOCK, 1, 0, 4 * cus, 1), cw.classes), cw.knobs))
    nmax = max(w.ge.n for w, _ in windows) + 40
    bad, ncases = [], 0
    for fill in (0, 1):
        host = np.full(nmax, fill, np.uint8)
        dev = ec.Mask.new(host)
        small = dev.shard(16, 1000)   # one workgroup, between the launches of the other windows
        for one in (0, 1, 2):
            for w, knobs in windows:
                ge = w.ge
                off = 16 - ge.head if ge.cpg is None else 17
                pos = rc.window_positions(w if ge.n > ge.cpl + 1 else rc.Window(w.name, ge, ("*",)))
                d = dev.shard(off, ge.n)
                with ec.tuned(counts_one_launch=one, **dict(knobs)):
                    for nm, i in pos:
                        host[off + i] = 1 - fill
                        dev.put(off + i, bool(1 - fill))
                        hw = host[off:off + ge.n]
                        exp = eco.mask_counts(hw) + (eco.mask_all(hw, True), eco.mask_all(hw, False))
                        assert exp[:2] == ((1, ge.n - 1) if fill == 0 else (ge.n - 1, 1))
                        got = d.counts() + (d.all(True), d.all(False))
                        ssmall, exp_small = small.counts(), eco.mask_counts(host[16:1016])   # a one-workgroup launch in between: it takes no ticket
                        host[off + i] = fill
                        dev.put(off + i, bool(fill))
                        ncases += 1
                        if got != exp or ssmall != exp_small:
                            bad.append(f"fill {fill} counts_one_launch {one} {w.name} {dict(knobs)} {nm}[{i}]: expected {exp} got {got}, small window expected {exp_small} got {ssmall}")
                    assert d.counts() == eco.mask_counts(host[off:off + ge.n]) and d.all(bool(fill)), (w.name, "flat")
    print(f"reduction cases: mask_counts/all {ncases}")
    assert not bad, f"{len(bad)} of {ncases} cases differ:\n" + "\n".join(bad[:12])


# ---------------------------------------------------------------- ec_expr_min_max: the interpreter (two passes) and the generated kernel
def _oracle_program(hs, scalars, steps):
    val = dict(enumerate(hs))
    for k, c in enumerate(scalars):
        val[8 + k] = np.full(len(hs[0]), float(c))
    last = None
    for op, a, b, dst in steps:
        val[4 + dst] = eco.f_binop(op, val[a], val[b])
        last = 4 + dst
    return val[last]


def _stat(ec, key):
    v = C.c_int64(0)
    assert ec.lib().ec_stat_get(key, C.byref(v)) == 0
    return v.value


IDENT = ([1.0], [(eco.MUL, S(0), K(0), 0)])   # s0 * 1.0: the cell as f64


def _sole_image(vals, mask, at, side_name, label):
    """The premise of a program case: the oracle's (min, max) of the program's f64 result, with the assertion that cell `at` is the
    ONLY valid cell that holds that side of it."""
    emn, emx = eco.f_min_max(vals, mask)
    want = (emn.bits(), emx.bits())
    valid = np.ones(vals.size, bool) if mask is None else np.asarray(mask).astype(bool)
    for side, i in enumerate(at):
        if i is not None:
            holders = np.flatnonzero((rc.as_bits(vals) == want[side]) & valid)
            assert holders.tolist() == [i], f"generator: {label}: the {side_name[side]} of the program's result is held by cells {holders[:4].tolist()}, planted at {i}"
    return want


@pytest.mark.parametrize("ct", range(NT))
def test_expr_min_max_every_position(ec, cus, ct):
    """`s0 * 1.0` carries the sole-extreme fields through as f64 (8-byte integers with plants 2^13 beyond the band, which survive the
    rounding): every lane, both cells of a pair, every load, the full against the guarded tile, the peeled head cell (1-byte cells
    at an odd offset) and the odd tail cell, a tile of the second round, workgroup 0 against the last — through expr_jit 0
    (interpreter + min_max of the temporary) and 2 (the generated reduce kernel).  Before the GPU is asked, the oracle's answer for
    the program is asserted to be held by the planted cells alone.  Float types also run every order kind at a reduced set of
    positions, so that the sign of a zero and the payload of a NaN ARE the answer."""
    assert os.environ.get("EC_EXPR_REDUCE_U") in (None, "4"), "the position classes assume the generated kernel's default of 4 pairs per lane"
    head = 1 if rc.dtype_of(ct).itemsize == 1 else 0
    kind = rc.expr_kind(ct)
    plans = []
    cases = []
    for w in rc.jit_windows(cus, head):
        cases += rc.rotate_cases(w, kind) + rc.rotate_cases(w, kind, masked=True)
    plans.append((kind, cases))
    if ct in rc.FLOATS:
        w0 = rc.jit_windows(cus, head)[0]
        reduced = rc.Window("jit_order", w0.ge, ("slot1", "lane5", "load3", "partial_inner", "tail0", "tile_last"))
        plans += [(k, rc.rotate_cases(reduced, k)) for k in rc.KINDS_FLOAT if k != kind]
    P = ec.fused
    scalars, steps = IDENT
    ncases = 0
    for kind_, cases in plans:
        pool = _pool_for(ec, ct, cases, kind=kind_, masked=kind_ == kind)
        for mode in (0, 2):
            bad = []
            with P.jit(mode):
                for c in cases:
                    ce, me, planted = rc.case_edits(ct, c, pool.host.block)
                    # 1-byte cells: the window starts one cell before a 16-byte boundary, at an odd address, so the head cell is peeled
                    with pool.planted(c.window.ge, ce, me, c.masked) as (ha, hm, da, dm):
                        at = [i if b is not None else None for i, b in zip((c.i_min, c.i_max), planted)]
                        exp = _sole_image(_oracle_program([ha], scalars, steps), hm, at, ("minimum", "maximum"), c.label())
                        j0 = _stat(ec, b"expr_jit_launches")
                        mn, mx = P.program_min_max([ec.MaskedCellBuffer(da, dm) if c.masked else da], scalars, steps)
                        assert (_stat(ec, b"expr_jit_launches") - j0 == 1) == (mode == 2)
                    ncases += 1
                    if (mn.ct, mn.bits(), mx.bits()) != (eco.F64, exp[0], exp[1]):
                        bad.append(f"{eco.CT_NAMES[ct]} expr_jit={mode} {c.label()}: expected ({exp[0]:#x}, {exp[1]:#x}) got ({mn.bits():#x}, {mx.bits():#x})")
            assert not bad, f"{len(bad)} cases differ:\n" + "\n".join(bad[:12])
    print(f"reduction cases: expr_min_max {eco.CT_NAMES[ct]} {ncases}")


def _poke(ec, buf, edits):
    """{cell index: bits} into a device buffer (or mask), one small upload per contiguous run."""
    sz = 1 if isinstance(buf, ec.Mask) else rc.dtype_of(buf.ct).itemsize
    for start, vals in rc.runs(edits):
        x = np.array(vals, dtype=rc._UINT[sz])
        ec._ffi.check(ec.lib().ec_upload(buf.mem.window(start * sz, x.nbytes).ptr, x.ctypes.data_as(C.c_void_p), x.nbytes, ec.buffer.stream()))


def test_expr_min_max_special_values_across_the_two_fold_paths(ec, cus):
    """The generated kernel folds a tile by VALUE when it holds no NaN and no zero and by KEY otherwise.  f64 fields: a sole -0.0, a
    NaN of either sign, or a zero in one lane of an otherwise ordinary tile; a sole extreme in an ordinary tile next to a special
    one; a NaN under a hidden cell of an ordinary tile, which must neither win nor change the answer; `s0 - s1` with s1 flat; NDVI
    over u16 with one cell pair planted.  One device buffer and one mask: the cells of a case are written in place and put back."""
    P = ec.fused
    ct = eco.F64
    tile = rc.JIT_BLOCK * rc.JIT_U * 2
    n = 3 * tile + 301
    a = rc.field_cells(ct, n, 12)
    v = rc.as_bits(a)
    mn_b, mx_b, _ = rc.plant_bits(ct, "adjacent", rc._band_block(ct, 12, "adjacent"))
    nan_neg, nan_pos, _ = rc.plant_bits(ct, "nan", rc._band_block(ct, 12, "nan"))
    specials = {"neg_zero": 1 << 63, "pos_zero": 0, "nan_neg": nan_neg, "nan_pos": nan_pos}
    bad, ncases = [], 0
    flat, ones = ec.CellBuffer.from_vec(np.zeros(n)), ec.Mask.fill(n, True)
    hm = np.ones(n, np.uint8)
    hm[tile // 2] = 0
    d, dmask = ec.CellBuffer.from_vec(a), ec.Mask.new(hm)
    for mode in (0, 2):
        with P.jit(mode):
            for name, bits in specials.items():
                for lane_cell in (tile + 2 * (rc.JIT_BLOCK + 77) + 1, 5, n - 1):      # tile 1 (key path) between two ordinary tiles; head of tile 0; the odd tail cell
                    for extreme_at in (3 * rc.JIT_BLOCK, 2 * tile + 9):                  # the sole extremes in ordinary tiles on either side
                        for masked in (False, True):
                            edits = {lane_cell: bits, extreme_at: mn_b, extreme_at + 1: mx_b}
                            if masked:
                                edits[tile // 2] = nan_neg | 0xFFFF                    # a NaN beyond every plant under the hidden cell of an ordinary tile
                            old = {i: int(v[i]) for i in edits}
                            for i, b in edits.items():
                                v[i] = b
                            _poke(ec, d, edits)
                            src = ec.MaskedCellBuffer(d, dmask) if masked else d
                            for scalars, steps, streams in ((IDENT[0], IDENT[1], [src]),
                                                            ([], [(eco.SUB, S(0), S(1), 0)], [src, ec.MaskedCellBuffer(flat, ones) if masked else flat])):
                                want = eco.f_min_max(_oracle_program([a] + [np.zeros(n)] * (len(streams) - 1), scalars, steps), hm if masked else None)
                                got = P.program_min_max(streams, scalars, steps)
                                ncases += 1
                                if (got[0].bits(), got[1].bits()) != (want[0].bits(), want[1].bits()):
                                    bad.append(f"expr_jit={mode} {name}@{lane_cell} extremes@{extreme_at} masked={masked} steps={steps}: expected "
                                               f"({want[0].bits():#x}, {want[1].bits():#x}) got ({got[0].bits():#x}, {got[1].bits():#x})")
                            for i, b in old.items():
                                v[i] = b
                            _poke(ec, d, old)
            # NDVI over u16: (nir - red) / (nir + red), one cell pair planted as the sole +1 and the sole -1
            ndvi = [(eco.SUB, S(0), S(1), 0), (eco.ADD, S(0), S(1), 1), (eco.DIV, R(0), R(1), 0)]
            rng = np.random.default_rng(5)
            nir, red = rng.integers(1000, 30000, n).astype(np.uint16), rng.integers(1000, 30000, n).astype(np.uint16)
            nir0, red0 = nir.copy(), red.copy()
            dn, dr = ec.CellBuffer.from_vec(nir), ec.CellBuffer.from_vec(red)
            w = rc.Window("ndvi", rc.Geometry(n, 2, rc.JIT_BLOCK, rc.JIT_U, 0, None, 2, False), ("*",))
            for c in rc.rotate_cases(w):
                for i, (x, y) in ((c.i_min, (0, 65535)), (c.i_max, (65535, 0))):
                    nir[i], red[i] = x, y
                    dn.put(i, np.uint16(x)), dr.put(i, np.uint16(y))
                exp = _sole_image(_oracle_program([nir, red], [], ndvi), None, (c.i_min, c.i_max), ("minimum", "maximum"), c.label())
                got = P.program_min_max([dn, dr], [], ndvi)
                for i in (c.i_min, c.i_max):
                    nir[i], red[i] = nir0[i], red0[i]
                    dn.put(i, nir0[i]), dr.put(i, red0[i])
                ncases += 1
                if (got[0].bits(), got[1].bits()) != exp:
                    bad.append(f"expr_jit={mode} NDVI {c.label()}: got ({got[0].value}, {got[1].value})")
    print(f"reduction cases: expr_min_max special values + NDVI {ncases}")
    assert not bad, f"{len(bad)} of {ncases} cases differ:\n" + "\n".join(bad[:12])


# ---------------------------------------------------------------- the shard group on one GPU
@pytest.mark.parametrize("G", [1, 3, 8])
def test_sharded_min_max_sole_extremes_in_every_shard_pair(ec, G):
    """`ec_sharded_min_max` and `ShardGroup.program_min_max`: the sole minimum in the first cell of shard s, the sole maximum in the
    last cell of shard t, for every (s, t) and all ten types; once per type masked with decoys.  8-byte integers take the plants that
    survive `as f64`; that each plant is the only holder is asserted for the cells and for their f64 image."""
    from erased_cells_hip import sharded
    rows, cols = 5 * G + 1, 1003
    n = rows * cols
    ranges = [sharded.shard_range(rows, cols, g, G) for g in range(G)]
    bad, ncases = [], 0
    with sharded.ShardGroup([0] * G, host_combine=G > 1) as g:
        for ct in range(NT):
            kind = rc.expr_kind(ct)
            for s in range(G):
                for t in range(G):
                    i_min, i_max = ranges[s][0], ranges[t][0] + ranges[t][1] - 1
                    label = f"G={G} {eco.CT_NAMES[ct]} min in shard {s} max in shard {t}"
                    a = rc.sole_extreme_cells(ct, n, i_min, i_max, 31, kind)
                    masked = (s, t) == (G - 1, 0)
                    mask = rc.hide_decoys(ct, a, [i_min, i_max]) if masked else None
                    want = _sole_image(a, mask, (i_min, i_max), ("minimum", "maximum"), label)
                    assert want == rc.plant_bits(ct, kind, rc._band_block(ct, 31, kind))[:2]
                    pwant = _sole_image(_oracle_program([a], *IDENT), mask, (i_min, i_max), ("minimum", "maximum"), label + " as f64")
                    sa = g.scatter(a, rows, cols)
                    sm = g.scatter(mask, rows, cols) if masked else None
                    try:
                        got = g.min_max(sa, sm)
                        pgot = g.program_min_max([sa], IDENT[0], IDENT[1], masks=[sm] if masked else None)
                    finally:
                        sa.free()
                        if sm is not None:
                            sm.free()
                    ncases += 2
                    if (got[0].ct, got[0].bits(), got[1].bits()) != (ct,) + want:
                        bad.append(f"{label} masked={masked}: expected {want} got {got}")
                    if (pgot[0].bits(), pgot[1].bits()) != pwant:
                        bad.append(f"{label} program masked={masked}: expected {pwant} got {pgot}")
    print(f"reduction cases: sharded min_max + program_min_max G={G} {ncases}")
    assert not bad, f"{len(bad)} of {ncases} cases differ:\n" + "\n".join(bad[:12])
