"""Every arithmetic path on the lattice of special operand pairs (tests/special_cases.py), each cell compared as bits against the set
the exact reference allows (tests/ieee_ref.py) — one bit pattern everywhere but in the two-answer cells (two different NaNs under
`+` or `*`), whose number is asserted to be what the value lists predict.  Nothing is compared by class.

The paths: `ec_binop` (direct, LDS-staged, cell-wise, every peel), `ec_masked_binop`, `ec_binop_scalar`, `ec_fused` / `ec_masked_fused`
(one-pass and convert-then-fuse), and `ec_expr` / `ec_masked_expr` three times over: the interpreter, the run-time compiled form and
the ahead-of-time kernels, each confirmed by its launch counter.  tests/test_special_cases.py shows that these inputs tell a wrong
cell rule from the right one."""
import ctypes as C
import functools

import numpy as np
import pytest

import ieee_ref as R
import special_cases as sc
from vectors import bits_of, rand_mask

pytestmark = pytest.mark.gpu

NT = 10
OPS = sc.OPS
NAMES = ["UInt8", "UInt16", "UInt32", "UInt64", "Int8", "Int16", "Int32", "Int64", "Float32", "Float64"]
S, RG, K = sc.S, sc.RG, sc.K


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def _stat(ec, key):
    v = C.c_int64(0)
    assert ec.lib().ec_stat_get(key, C.byref(v)) == 0, key
    return v.value


def _check(got, alts, what):
    """Every cell of `got` (f64) is, as bits, one of the allowed patterns of its column of `alts`."""
    g = bits_of(got)
    alts = np.atleast_2d(alts)
    assert g.shape[0] == alts.shape[1], (what, g.shape, alts.shape)
    ok = R.allowed(alts, g)
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {len(g)} cells differ; first at {i}: got {int(g[i]):#018x}, allowed "
                             f"{sorted({hex(int(x)) for x in alts[:, i]})}")


# ---------------------------------------------------------------- inputs on the host and on the device, expected cells: made once
_host = {}   # (what, layout, lt, rt[, op]) -> arrays; the large ones of a pair are dropped once no later test needs them (_forget)
_dev = {}


def _memo(key, make):
    if key not in _host:
        _host[key] = make()
    return _host[key]


def _layout(name, lt, rt):
    return _memo(("layout", name, lt, rt), lambda: sc.layout_a(lt, rt) + (None,) if name == "A" else
                 sc.layout_b(lt, rt) if name == "B" else sc.layout_c(lt, rt))


def _wide(name, lt, rt):
    return _memo(("wide", name, lt, rt), lambda: tuple(R.widen_vec(x) for x in _layout(name, lt, rt)[:2]))


def _want(name, lt, rt, op):
    def make():
        first, second = R.binop_vec(op, *_wide(name, lt, rt))
        return np.stack([first, second]) if (first != second).any() else first[None, :]
    return _memo(("want", name, lt, rt, op), make)


def _forget(lt, rt):
    for key in [k for k in _host if k[2:4] == (lt, rt)]:
        del _host[key]
    for key in [k for k in _dev if k[1:3] == (lt, rt)]:
        del _dev[key]


def _device(ec, name, lt, rt):
    if (name, lt, rt) not in _dev:
        l, r, _ = _layout(name, lt, rt)
        _dev[name, lt, rt] = (ec.CellBuffer.from_vec(l), ec.CellBuffer.from_vec(r))
    return _dev[name, lt, rt]


@functools.lru_cache(maxsize=None)
def _masks(n):
    return rand_mask(n, 7001), rand_mask(n, 7002)


_dev_masks = {}


def _device_masks(ec, n):
    if n not in _dev_masks:
        _dev_masks[n] = tuple(ec.Mask.new(m) for m in _masks(n))
    return _dev_masks[n]


def _binop_layouts(ec, lt, rt, op, offsets=(0,), masked=False, layouts="ABC"):
    """`l op r` on the layouts: A and B whole (and one cell in, for `offsets`), C window by window into one result buffer."""
    what = f"{NAMES[lt]} {'+-*/'[op]} {NAMES[rt]}"
    for name in layouts:
        dl, dr = _device(ec, name, lt, rt)
        want = _want(name, lt, rt, op)
        if name == "C":
            wins = _layout(name, lt, rt)[2]
            out = ec.CellBuffer.empty(dl.len(), ec.Float64)
            L, st = ec.lib(), ec.stream()
            for s, n in wins:
                ec._ffi.check(L.ec_binop(op, lt, dl.shard(s, n).mem.ptr, rt, dr.shard(s, n).mem.ptr, n, out.shard(s, n).mem.ptr, st))
            if wins:
                got = out.to_numpy()
                inside = np.concatenate([np.arange(s, s + n) for s, n in wins])
                _check(got[inside], want[:, inside], f"{what} layout C")
            continue
        for off in offsets:
            n = dl.len() - off
            a, b = dl.shard(off, n), dr.shard(off, n)
            if masked:
                hm, dm = _masks(dl.len()), _device_masks(ec, dl.len())
                got = ec.MaskedCellBuffer(a, dm[0].shard(off, n))._binop(op, ec.MaskedCellBuffer(b, dm[1].shard(off, n)))
                assert np.array_equal(got.mask().to_numpy(), hm[0][off:] & hm[1][off:]), (what, name, off)
                got = got.buffer()
            else:
                got = a._binop(op, b)
            _check(got.to_numpy(), want[:, off:], f"{what} layout {name} offset {off}{' masked' if masked else ''}")


# ---------------------------------------------------------------- ec_binop
@pytest.mark.parametrize("lt", range(NT), ids=NAMES)
def test_binop_every_pair_on_every_layout(ec, lt):
    """All ten right types x four ops on layouts A, B and C; the two-answer cells of the lattice are as many as the lists predict, and
    every other cell has one allowed bit pattern."""
    for rt in range(NT):
        two = 0
        n_lattice = len(sc.specials(lt)) * len(sc.specials(rt))
        for op in OPS:
            want = _want("A", lt, rt, op)
            two += int((want[0, :n_lattice] != want[-1, :n_lattice]).sum())
            _binop_layouts(ec, lt, rt, op)
        assert two == sc.predicted_two_answer_cells(lt, rt), (lt, rt, two)
        if (lt, rt) not in sc.FLOAT_PAIRS and not (lt == rt and lt in sc.BY_WIDTH.values()):
            _forget(lt, rt)   # only the eight float-bearing pairs and the formulas' same-type pairs are used again below


KNOBS = [dict(binop_variant=-1), dict(binop_variant=0), dict(binop_variant=1), dict(unaligned_vector=0), dict(peel=0), dict(peel=2)]


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_binop_float_pairs_under_every_kernel_choice(ec, knobs):
    """The eight float-bearing pairs under each binop_variant (by rule, direct, LDS-staged), with the vector path off for windows one
    cell into the buffers (the cell-wise kernels), and with the head cell never and always peeled: layouts A and B at cell offsets
    0 and 1, layout C as it is."""
    with ec.tuned(**knobs):
        for lt, rt in sc.FLOAT_PAIRS:
            for op in OPS:
                _binop_layouts(ec, lt, rt, op, offsets=(1,) if "unaligned_vector" in knobs else (0, 1))


@pytest.mark.parametrize("pair", sc.FLOAT_PAIRS, ids=lambda p: f"{NAMES[p[0]]}-{NAMES[p[1]]}")
def test_masked_binop_computes_every_cell(ec, pair):
    """ec_masked_binop computes all cells, valid or not (include/erased_cells.h): every cell is compared, and the mask."""
    for op in OPS:
        _binop_layouts(ec, *pair, op, offsets=(0, 1), masked=True, layouts="AB")
    with ec.tuned(binop_variant=1):
        _binop_layouts(ec, *pair, sc.OPS[(pair[0] + pair[1]) % 4], offsets=(0, 1), masked=True, layouts="AB")


# ---------------------------------------------------------------- ec_binop_scalar
def _scalar(bits):
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


@pytest.mark.parametrize("ct", [R.F32, R.F64, R.I16, R.U64], ids=lambda c: NAMES[c])
def test_binop_scalar_every_special_scalar(ec, ct):
    """Every special of the cell type planted alone (layout B) against every f64 special as the scalar."""
    cells, _ = sc.layout_b_single(ct)
    wide = R.widen_vec(cells)
    d = ec.CellBuffer.from_vec(cells)
    for k in sc.SCALAR_BITS:
        for op in OPS:
            first, second = R.binop_vec(op, wide, np.uint64(k))
            for off in (0, 1):
                got = d.shard(off, len(cells) - off)._binop(op, _scalar(k))
                _check(got.to_numpy(), np.stack([first, second])[:, off:], f"{NAMES[ct]} {'+-*/'[op]} scalar {k:#018x} offset {off}")


# ---------------------------------------------------------------- ec_fused, ec_masked_fused
QUADS = {"f64": [R.F64] * 4, "f32": [R.F32] * 4, "mixed": [R.F32, R.F64, R.I16, R.U8]}


@pytest.mark.parametrize("fused_mixed", [1, 0])
@pytest.mark.parametrize("kind", list(QUADS))
def test_fused_chain_lattices(ec, kind, fused_mixed):
    """(x o1 y) o2 (z o3 w) on T^4 under all 64 op triples and (x o1 y) o2 z on T^3 under all 16 op pairs, plain and masked (all cells
    compared, and the mask); once through the one-pass kernels and once through convert-then-fuse."""
    cts = QUADS[kind]
    with ec.tuned(fused_mixed=fused_mixed):
        for arity in (4, 3):
            host = sc.chain_grid(cts[:arity])
            wide = [R.widen_vec(h) for h in host]
            n = len(host[0])
            dev = [ec.CellBuffer.from_vec(h) for h in host]
            hm = [rand_mask(n, 7100 + k) for k in range(arity)]
            mdev = [ec.MaskedCellBuffer(d, ec.Mask.new(m)) for d, m in zip(dev, hm)]
            want_mask = np.bitwise_and.reduce(hm)
            for ops in (sc.OP_TRIPLES if arity == 4 else sc.OP_PAIRS):
                if arity == 4:
                    o1, o2, o3 = ops
                    steps = [(o1, 0, 1, 0), (o3, 2, 3, 1), (o2, 4, 5, 0)]
                    args = lambda b: (b[0], o1, b[1], o2, b[2], o3, b[3])  # noqa: E731
                else:
                    o1, o2 = ops
                    steps = [(o1, 0, 1, 0), (o2, 4, 2, 0)]
                    args = lambda b: (b[0], o1, b[1], o2, b[2])  # noqa: E731
                want = R.program(wide, [], steps)
                _check(ec.fused.expr(*args(dev)).to_numpy(), want, f"fused {kind} {ops}")
                got = ec.fused.expr(*args(mdev))
                _check(got.buffer().to_numpy(), want, f"masked fused {kind} {ops}")
                assert np.array_equal(got.mask().to_numpy(), want_mask), (kind, ops)


# ---------------------------------------------------------------- ec_expr, ec_masked_expr: interpreted, compiled, ahead of time
MODES = {
    "interpreter": (dict(expr_jit=0, expr_fixed=0), b"expr_interp_launches"),
    "compiled": (dict(expr_jit=2, expr_fixed=0), b"expr_jit_launches"),
    "ahead-of-time": (dict(expr_jit=0, expr_fixed=1), b"expr_fixed_launches"),
}


def _program(ec, mode, dev, scalars, steps, want, what, masks=None):
    """One launch of the program, plain, and one masked where `masks` = (host masks, device masks): each counted by the mode's
    launch counter and by no other, every cell in its allowed set."""
    _, counter = MODES[mode]
    sc_vals = [_scalar(k) for k in scalars]
    before = {c: _stat(ec, c) for _, c in MODES.values()}
    got = ec.fused.program(dev, sc_vals, steps)
    runs = 1
    _check(got.to_numpy(), want, f"{mode} {what}")
    if masks is not None:
        hm, dm = masks
        got = ec.fused.program([ec.MaskedCellBuffer(d, m) for d, m in zip(dev, dm)], sc_vals, steps)
        runs = 2
        _check(got.buffer().to_numpy(), want, f"{mode} masked {what}")
        assert np.array_equal(got.mask().to_numpy(), np.bitwise_and.reduce(hm)), (mode, what)
    after = {c: _stat(ec, c) for _, c in MODES.values()}
    assert {c: after[c] - before[c] for c in after} == {c: runs if c == counter else 0 for c in after}, (mode, what)


def _mask_pair(ec, n, k):
    hm = [rand_mask(n, 7200 + j) for j in range(k)]
    return hm, [ec.Mask.new(m) for m in hm]


@pytest.mark.parametrize("mode", ["interpreter", "compiled"])
@pytest.mark.parametrize("pair", sc.FLOAT_PAIRS, ids=lambda p: f"{NAMES[p[0]]}-{NAMES[p[1]]}")
def test_expr_single_steps_on_the_layouts(ec, pair, mode):
    """`S0 op S1` as a program on layouts A and B (masked too on A), whole and one cell in (peeled head, odd tail)."""
    lt, rt = pair
    with ec.tuned(**MODES[mode][0]):
        for name in "AB":
            dl, dr = _device(ec, name, lt, rt)
            masks = _mask_pair(ec, dl.len(), 2) if name == "A" else None
            for op in OPS:
                want = _want(name, lt, rt, op)
                _program(ec, mode, [dl, dr], [], [(op, S(0), S(1), 0)], want, f"{NAMES[lt]} {op} {NAMES[rt]} layout {name}", masks)
                n = dl.len() - 1
                _program(ec, mode, [dl.shard(1, n), dr.shard(1, n)], [], [(op, S(0), S(1), 0)], want[:, 1:],
                         f"{NAMES[lt]} {op} {NAMES[rt]} layout {name} offset 1")


_t3 = {}


def _t3_inputs(ec, ct):
    if ct not in _t3:
        host = sc.chain_grid([ct] * 3)
        _t3[ct] = ([R.widen_vec(h) for h in host], [ec.CellBuffer.from_vec(h) for h in host], _mask_pair(ec, len(host[0]), 3))
    return _t3[ct]


@pytest.mark.parametrize("mode", ["interpreter", "compiled"])
@pytest.mark.parametrize("o1,o2", sc.OP_PAIRS, ids=lambda o: "+-*/"[o])
@pytest.mark.parametrize("ct", [R.F64, R.F32], ids=["f64", "f32"])
def test_expr_two_step_chains_on_t3(ec, ct, o1, o2, mode):
    """`(S0 o1 S1) o2 S2` and `S2 o2 (S0 o1 S1)` with the first result read straight from the accumulator (the next step) and through
    a filed register (a step in between writes another register)."""
    wide, dev, masks = _t3_inputs(ec, ct)
    between = (R.MUL, S(2), S(2), 3)
    with ec.tuned(**MODES[mode][0]):
        for left in (True, False):
            last = (o2, RG(0), S(2), 1) if left else (o2, S(2), RG(0), 1)
            want = R.program(wide, [], [(o1, 0, 1, 0), last])
            for steps in ([(o1, S(0), S(1), 0), last], [(o1, S(0), S(1), 0), between, last]):
                _program(ec, mode, dev, [], steps, want, f"chain {ct} {steps}", masks if left else None)


@pytest.mark.parametrize("mode", ["interpreter", "compiled"])
@pytest.mark.parametrize("ct", [R.F64, R.F32, R.I16], ids=lambda c: NAMES[c])
def test_expr_stream_and_scalar_either_way_round(ec, ct, mode):
    """`S0 op K` and `K op S0` for every f64 special as K, on the cell type's specials planted alone."""
    cells, _ = sc.layout_b_single(ct)
    wide, d = R.widen_vec(cells), ec.CellBuffer.from_vec(cells)
    with ec.tuned(**MODES[mode][0]):
        for k in sc.SCALAR_BITS:
            kk = np.full(len(cells), k, dtype=np.uint64)
            for op in OPS:
                _program(ec, mode, [d], [k], [(op, S(0), K(0), 0)], np.stack(R.binop_vec(op, wide, kk)), f"{NAMES[ct]} {op} K {k:#x}")
                _program(ec, mode, [d], [k], [(op, K(0), S(0), 0)], np.stack(R.binop_vec(op, kk, wide)), f"K {k:#x} {op} {NAMES[ct]}")


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_expr_catalogue_formulas(ec, width, mode):
    """NDVI on layouts A and B; (a+b)*c and EVI on T^3 (EVI with ordinary and with special scalars); a*k0+k1 with special scalars,
    ordinary ones and the contraction witness — streams of one width, so that with `expr_fixed` = 1 the ahead-of-time kernel runs."""
    ct = sc.BY_WIDTH[width]
    with ec.tuned(**MODES[mode][0]):
        _, ndvi = sc.FORMULAS["NDVI"]
        for name in "AB":
            dl, dr = _device(ec, name, ct, ct)
            want = R.program(list(_wide(name, ct, ct)), [], ndvi)
            _program(ec, mode, [dl, dr], [], ndvi, want, f"NDVI width {width} layout {name}", _mask_pair(ec, dl.len(), 2) if name == "A" else None)
            n = dl.len() - 1
            _program(ec, mode, [dl.shard(1, n), dr.shard(1, n)], [], ndvi, want[:, 1:], f"NDVI width {width} layout {name} offset 1")
        host = sc.triple_streams(width)
        wide, dev = [R.widen_vec(h) for h in host], [ec.CellBuffer.from_vec(h) for h in host]
        masks = _mask_pair(ec, len(host[0]), 3)
        _, addmul = sc.FORMULAS["add-mul"]
        _program(ec, mode, dev, [], addmul, R.program(wide, [], addmul), f"(a+b)*c width {width}", masks)
        _, evi = sc.FORMULAS["EVI"]
        for ks in [sc.EVI_ORDINARY] + sc.EVI_SPECIAL:
            _program(ec, mode, dev, ks, evi, R.program(wide, ks, evi), f"EVI width {width} scalars {[hex(k) for k in ks]}", masks)
        _, affine = sc.FORMULAS["affine"]
        cells = sc.affine_stream(width)
        w1, d1 = [R.widen_vec(cells)], [ec.CellBuffer.from_vec(cells)]
        m1 = _mask_pair(ec, len(cells), 1)
        for t, (k0, k1) in enumerate(sc.AFFINE_SCALARS + [sc.AFFINE_WITNESS[width][1:], sc.AFFINE_ORDINARY]):
            _program(ec, mode, d1, [k0, k1], affine, R.program(w1, [k0, k1], affine), f"a*k0+k1 width {width} k0 {k0:#x} k1 {k1:#x}",
                     m1 if t % 8 == 0 else None)
