"""Every tuning knob across its accepted range against the oracle: a value `ec_tune_set` accepts must compute the oracle's cells in
every kernel family the knob reaches.  The occupancy caps force dynamic LDS on every launch of a family, on top of the static slabs
of the LDS-staged binop (1 KiB per wave for each staged operand of 4 bytes, 16 B for an operand that is not staged: 8 KiB for a
4-byte . 4-byte pair, the largest), so `binop_lds_kb` = 64 asks for 72 KiB per workgroup at most; the launch-shape knobs pick other
instantiations and grids.  Which values are accepted, and what they read back as, is tests/test_tuning_surface.py."""
import ctypes as C
import itertools
import threading
import time
import traceback

import numpy as np
import pytest

from oracle import eco
from test_tuning_surface import DEFAULTS
from vectors import assert_f64_bits_equal, bits_of, rand_cells, rand_mask

pytestmark = pytest.mark.gpu

NT = eco.NTYPES
N = 300_001                    # the general size: a few hundred wave tiles and a ragged tail
NBIG = (1 << 20) + 3           # the LDS rule of the binop fires from 2^20 cells on
NRED = (1 << 21) + 3           # the largest reduction
S, R, K = (lambda k: k), (lambda k: 4 + k), (lambda k: 8 + k)


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def _tune(ec):
    v, out = C.c_int64(), {}
    for k in DEFAULTS:
        assert ec.lib().ec_stat_get(b"tune." + k.encode(), C.byref(v)) == 0, k
        out[k] = v.value
    return out


@pytest.fixture(autouse=True)
def no_knob_leaks(ec):
    """A case that leaves a knob turned would change what every later test covers."""
    before = _tune(ec)
    yield
    assert _tune(ec) == before


def _stat(ec, key):
    v = C.c_int64(0)
    assert ec.lib().ec_stat_get(key, C.byref(v)) == 0, key
    return v.value


def _loose(op, l, r):
    """Cells whose NaN bits the reference does not pin: both operands NaN under a commutative op (the parity tests' rule)."""
    if op not in (eco.ADD, eco.MUL):
        return None
    with np.errstate(all="ignore"):
        return np.isnan(np.asarray(l).astype(np.float64)) & np.isnan(np.asarray(r).astype(np.float64))


def _oracle_steps(streams, scalars, steps):
    """A program evaluated step by step on the oracle's typed loops, and the cells whose NaN bits are left open (carried forward)."""
    n = min(len(s_) for s_ in streams)
    val = {k: s_[:n] for k, s_ in enumerate(streams)}
    loose = {k: np.zeros(n, bool) for k in val}
    for k, c in enumerate(scalars):
        val[8 + k], loose[8 + k] = np.full(n, float(c)), np.zeros(n, bool)
    last = None
    for op, a, b, dst in steps:
        lo = loose[a] | loose[b]
        if op in (eco.ADD, eco.MUL):
            lo = lo | _loose(op, val[a], val[b])
        val[4 + dst], loose[4 + dst] = eco.f_binop(op, val[a], val[b]), lo
        last = 4 + dst
    return val[last], loose[last]


@pytest.fixture(scope="module")
def data(ec):
    host = {ct: rand_cells(ct, NBIG + 8, 9100 + ct) for ct in range(NT)}
    dev = {ct: ec.CellBuffer.from_vec(a) for ct, a in host.items()}
    m = [rand_mask(NBIG + 8, 9200 + k) for k in range(2)]
    dm = [ec.Mask.new(x) for x in m]
    return host, dev, m, dm


@pytest.fixture(scope="module")
def oracle():
    """The oracle's answers by (pair, op, window), shared by the cases of one sweep: they do not depend on a knob."""
    return {}


def _check_binop(ec, data, lt, rt, op, off, n, masked=False, want=None):
    host, dev, m, dm = data
    hl, hr = host[lt][off:off + n], host[rt][off:off + n]
    key = (lt, rt, op, off, n)
    if want is None or key not in want:
        exp = (eco.f_binop(op, hl, hr), _loose(op, hl, hr))
        if want is not None:
            want[key] = exp
    else:
        exp = want[key]
    if masked:
        a = ec.MaskedCellBuffer(dev[lt].shard(off, n), dm[0].shard(off, n))
        b = ec.MaskedCellBuffer(dev[rt].shard(off, n), dm[1].shard(off, n))
        got = a._binop(op, b)
        assert np.array_equal(got.mask().to_numpy(), m[0][off:off + n] & m[1][off:off + n]), (lt, rt, op, off, n)
        got = got.buffer()
    else:
        got = dev[lt].shard(off, n)._binop(op, dev[rt].shard(off, n))
    try:
        assert_f64_bits_equal(got.to_numpy(), exp[0], nan_by_class_where=exp[1])
    except AssertionError as e:
        raise AssertionError(f"{eco.CT_NAMES[lt]} {op} {eco.CT_NAMES[rt]} off {off} n {n} masked {masked}: {e}") from None


# ---------------------------------------------------------------- binop_lds_kb: the direct and the LDS-staged binop, plain and masked
RULE_PAIRS = [(eco.F64, eco.U16), (eco.U16, eco.F64), (eco.F64, eco.F32)]   # an 8-byte operand against one of <= 4 bytes
# f64 . f64 is never staged (only operands of <= 4 bytes are): the direct kernel under every variant, with the 48 KiB rule at -1;
# i32 . f32 stages both operands: the largest static slabs (8 KiB), so the largest workgroup a cap can ask for
BINOP_PAIRS = [(eco.F64, eco.F64)] + RULE_PAIRS + [(eco.U8, eco.U16), (eco.I32, eco.F32)]
OPS = (eco.DIV, eco.SUB, eco.MUL, eco.ADD)


@pytest.mark.parametrize("kb", [-1, 0, 1, 16, 32, 48, 64, 65])
def test_binop_lds_kb(ec, data, oracle, kb):
    """Every binop_lds_kb value, under every binop_variant: f64 . f64 (the direct kernel — no operand of it is staged — with the
    48 KiB rule at -1 and the cap's reservation otherwise), the three rule pairs, u8 . u16, and i32 . f32 (under variant 1 the
    LDS-staged kernel with 8 KiB of static slabs plus the cap: 72 KiB at 64) — at 2^20 + 3 cells (the LDS rule must fire for the
    rule pairs when every stream is non-temporal: mall_mb = 0), at an odd cell offset, and a small ragged window; the masked binop
    under variants 0 and 1."""
    windows = [(0, NBIG), (1, NBIG), (3, 1037)]
    with ec.tuned(binop_lds_kb=kb, mall_mb=0):
        for variant in (-1, 0, 1):
            with ec.tuned(binop_variant=variant):
                for i, (lt, rt) in enumerate(BINOP_PAIRS):
                    op = OPS[i % 4]
                    for off, n in windows:
                        r0 = _stat(ec, b"binop_lds_rule_launches")
                        _check_binop(ec, data, lt, rt, op, off, n, want=oracle)
                        fired = _stat(ec, b"binop_lds_rule_launches") - r0
                        assert fired == int(variant == -1 and (lt, rt) in RULE_PAIRS and n >= (1 << 20)), (lt, rt, variant, off, n)
                    if variant >= 0:
                        _check_binop(ec, data, lt, rt, eco.DIV, 1, N, masked=True, want=oracle)
                        _check_binop(ec, data, lt, rt, eco.ADD, 0, 4099, masked=True, want=oracle)


# ---------------------------------------------------------------- scalar_lds_kb: buffer . scalar over all ten lhs types
@pytest.mark.parametrize("kb", [-1, 0, 32, 64])
def test_scalar_lds_kb(ec, data, kb):
    """Both forms of the scalar kernel: a finite scalar (integer cells take the form without the NaN rule) and NaN, +-inf and a
    zero divisor (the form with it)."""
    host, dev, _, _ = data
    cases = [(op, 2.5) for op in (eco.ADD, eco.SUB, eco.MUL, eco.DIV)] + [(eco.ADD, float("nan")), (eco.MUL, float("inf")),
                                                                         (eco.SUB, float("-inf")), (eco.DIV, 0.0)]
    with ec.tuned(scalar_lds_kb=kb):
        for ct in range(NT):
            for off, n in ((0, N), (1, 4097)):
                x = dev[ct].shard(off, n)
                hx = host[ct][off:off + n]
                for op, s in cases:
                    try:
                        assert_f64_bits_equal(x._binop(op, s).to_numpy(), eco.f_binop_scalar(op, hx, eco.Value.of(eco.F64, s)))
                    except AssertionError as e:
                        raise AssertionError(f"{eco.CT_NAMES[ct]} {op} {s} off {off}: {e}") from None


# ---------------------------------------------------------------- map_lds_kb, map_u: the map kernels
def _map_families(ec, data):
    host, dev, m, dm = data
    for off, n in ((0, N), (1, 2051)):
        hm1, hm2 = m[0][off:off + n], m[1][off:off + n]
        d1, d2 = dm[0].shard(off, n), dm[1].shard(off, n)
        assert np.array_equal((d1 & d2).to_numpy(), eco.mask_and(hm1, hm2))
        assert np.array_equal((d1 | d2).to_numpy(), eco.mask_or(hm1, hm2))
        assert np.array_equal((~d1).to_numpy(), eco.mask_not(hm1))
        for ct in range(NT):
            a, d = host[ct][off:off + n], dev[ct].shard(off, n)
            assert np.array_equal(bits_of((-d).to_numpy()), bits_of(eco.f_neg(a))), ct
            for dst in range(NT):
                if dst != ct and eco.can_fit_into(ct, dst):
                    assert np.array_equal(bits_of(d.convert(dst).to_numpy()), bits_of(eco.f_convert(a, dst))), (ct, dst)
            nd = eco.nodata_value(eco.ND_DEFAULT, ct)
            assert np.array_equal(ec.mask_from_nodata(d, ec.NoData.default()).to_numpy(), eco.f_mask_from_nodata(a, nd)), ct
            sel = ec.MaskedCellBuffer(d, d2).to_vec_with_nodata(ct, ec.NoData.default())
            assert np.array_equal(bits_of(sel), bits_of(eco.f_mask_select(a, hm2, nd))), ct


@pytest.mark.parametrize("kb", [0, 16, 64])
def test_map_lds_kb(ec, data, kb):
    with ec.tuned(map_lds_kb=kb):
        _map_families(ec, data)


@pytest.mark.parametrize("u", [1, 2, 4])
def test_map_u(ec, data, u):
    with ec.tuned(map_u=u):
        _map_families(ec, data)


def test_map_u_out_of_range_is_refused_and_changes_nothing(ec, data):
    L, E = ec.lib(), ec._ffi
    for u in (3, 0, -1, 5, 1 << 32, (1 << 32) + 2):
        assert L.ec_tune_set(b"map_u", u) == E.EC_ERR_ARG, u
    _map_families(ec, data)


# ---------------------------------------------------------------- fused_lds_kb: the one-pass kernels
FIXED = {  # the ahead-of-time catalogue (csrc/ec_expr_fixed.hpp): streams, scalars, steps
    "NDVI": (2, [], [(eco.SUB, S(0), S(1), 0), (eco.ADD, S(0), S(1), 1), (eco.DIV, R(0), R(1), 0)]),
    "add-mul": (3, [], [(eco.ADD, S(0), S(1), 0), (eco.MUL, R(0), S(2), 0)]),
    "EVI": (3, [2.5, 6.0, 7.5, 1.0], [(eco.SUB, S(0), S(1), 0), (eco.MUL, R(0), K(0), 0), (eco.MUL, S(1), K(1), 1), (eco.ADD, S(0), R(1), 1),
                                      (eco.MUL, S(2), K(2), 2), (eco.SUB, R(1), R(2), 1), (eco.ADD, R(1), K(3), 1), (eco.DIV, R(0), R(1), 0)]),
    "affine": (1, [0.0001, -273.15], [(eco.MUL, S(0), K(0), 0), (eco.ADD, R(0), K(1), 0)]),
}
BY_WIDTH = {1: [eco.U8, eco.I8], 2: [eco.U16, eco.I16], 4: [eco.F32, eco.I32, eco.U32], 8: [eco.F64, eco.I64, eco.U64]}


def _program(ec, data, cts, scalars, steps, off, n, masked):
    host, dev, m, dm = data
    bufs = [dev[ct].shard(off + k, n) for k, ct in enumerate(cts)]
    hs = [host[ct][off + k:off + k + n] for k, ct in enumerate(cts)]
    if masked:
        got = ec.fused.program([ec.MaskedCellBuffer(b, dm[k % 2].shard(off + k, n)) for k, b in enumerate(bufs)], scalars, steps)
        want_mask = np.ones(n, np.uint8)
        for k in range(len(cts)):
            want_mask &= m[k % 2][off + k:off + k + n]
        assert np.array_equal(got.mask().to_numpy(), want_mask)
        got = got.buffer()
    else:
        got = ec.fused.program(bufs, scalars, steps)
    eo, loose = _oracle_steps(hs, scalars, steps)
    assert_f64_bits_equal(got.to_numpy(), eo, nan_by_class_where=loose)


@pytest.mark.parametrize("kb", [0, 16, 64])
def test_fused_lds_kb(ec, data, kb):
    """k_fused (one cell type) and k_fused_any (a mixed pair), the interpreter (expr_fixed = 0, expr_jit = 0), and the four
    catalogue formulas at every cell width — each one launch of its built-in kernel — plain and masked."""
    host, dev, m, dm = data
    with ec.tuned(fused_lds_kb=kb, expr_jit=0):
        for lt, rt in ((eco.F32, eco.F32), (eco.U16, eco.F64), (eco.I8, eco.U32)):
            for masked in (False, True):
                for off, n in ((0, N), (1, 1031)):
                    x, y = dev[lt].shard(off, n), dev[rt].shard(off, n)
                    if masked:
                        x, y = ec.MaskedCellBuffer(x, dm[0].shard(off, n)), ec.MaskedCellBuffer(y, dm[1].shard(off, n))
                    got = ec.fused.expr(x, eco.SUB, y, eco.MUL, 2.5)
                    if masked:
                        assert np.array_equal(got.mask().to_numpy(), m[0][off:off + n] & m[1][off:off + n])
                        got = got.buffer()
                    eo, loose = _oracle_steps([host[lt][off:off + n], host[rt][off:off + n]], [2.5],
                                              [(eco.SUB, S(0), S(1), 0), (eco.MUL, R(0), K(0), 0)])
                    assert_f64_bits_equal(got.to_numpy(), eo, nan_by_class_where=loose)
        # the interpreter: a program outside the catalogue, and a catalogue one with the catalogue turned off
        with ec.tuned(expr_fixed=0):
            for masked in (False, True):
                i0 = _stat(ec, b"expr_interp_launches")
                _program(ec, data, [eco.U16, eco.I8, eco.F64], [0.5], [(eco.MUL, S(0), K(0), 0), (eco.SUB, R(0), S(1), 1),
                                                                       (eco.DIV, R(1), S(2), 0)], 1, N, masked)
                ns, scalars, steps = FIXED["EVI"]
                _program(ec, data, [eco.U16] * ns, scalars, steps, 0, 4099, masked)
                assert _stat(ec, b"expr_interp_launches") == i0 + 2
        for name, (ns, scalars, steps) in FIXED.items():
            for width, kinds in BY_WIDTH.items():
                cts = [kinds[k % len(kinds)] for k in range(ns)]
                for masked in (False, True):
                    for off, n in ((0, N), (3, 1029)):
                        f0 = _stat(ec, b"expr_fixed_launches")
                        try:
                            _program(ec, data, cts, scalars, steps, off, n, masked)
                        except AssertionError as e:
                            raise AssertionError(f"{name} width {width} masked {masked} off {off}: {e}") from None
                        assert _stat(ec, b"expr_fixed_launches") == f0 + 1, (name, width, masked)


# ---------------------------------------------------------------- reduce_bpc x reduce_shape: min_max, counts, first_difference
@pytest.fixture(scope="module")
def red(ec):
    host = {ct: rand_cells(ct, NRED + 1, 9300 + ct) for ct in range(NT)}
    dev = {ct: ec.CellBuffer.from_vec(a) for ct, a in host.items()}
    mask = rand_mask(NRED + 1, 9400)
    dmask = ec.Mask.new(mask)
    want = {}
    for ct in range(NT):
        for n in (0, 1, 255, 100_003, NRED):
            for masked in (False, True):
                want[ct, n, masked] = eco.f_min_max(host[ct][1:1 + n], mask[1:1 + n] if masked else None)
    return host, dev, mask, dmask, want


@pytest.mark.parametrize("bpc,shape", list(itertools.product([1, 2, 100], [0, 1, 2, 3, 4])))
def test_reduce_bpc_and_shape(ec, red, bpc, shape):
    """min_max plain and masked on all ten types at n in {0, 1, 255, 100003, 2^21 + 3} (at an odd offset), Mask::counts and the
    first difference of two buffers.  bpc = 100 asks for more workgroups than the finalize kernels read: the grid is capped."""
    host, dev, mask, dmask, want = red
    with ec.tuned(reduce_bpc=bpc, reduce_shape=shape):
        assert ec.lib().ec_tune_set(b"reduce_shape", 9) == ec._ffi.EC_ERR_ARG
        for ct in range(NT):
            for n in (0, 1, 255, 100_003, NRED):
                d = dev[ct].shard(1, n)
                for masked in (False, True):
                    src = ec.MaskedCellBuffer(d, dmask.shard(1, n)) if masked else d
                    got = src.min_max()
                    exp = want[ct, n, masked]
                    assert (got[0].ct, got[0].bits(), got[1].bits()) == (exp[0].ct, exp[0].bits(), exp[1].bits()), (ct, n, masked)
        for n in (1, 255, 100_003, NRED):
            assert dmask.shard(1, n).counts() == eco.mask_counts(mask[1:1 + n]), n
        a = host[eco.U16][:NRED]
        for at in (0, 7, 100_000, NRED - 1):
            b = a.copy()
            b[at] ^= 1
            db = ec.CellBuffer.from_vec(b)
            assert dev[eco.U16].shard(0, NRED).cmp(db) == eco.buffer_cmp(a, b), at
        assert dev[eco.U16].shard(0, NRED).cmp(ec.CellBuffer.from_vec(a.copy())) == 0


# ---------------------------------------------------------------- binop_variant, peel, cache_force: values the spec refuses
@pytest.mark.parametrize("knob,values", [("binop_variant", [-2, 2, 5, 1 << 32]), ("peel", [-1, 3, 7, 1 << 32]),
                                         ("cache_force", [-2, 256, 1 << 32, (1 << 63) - 1])])
def test_refused_values_leave_the_launches_alone(ec, data, knob, values):
    """Each value is refused with the knob unchanged, so the launches after it run the shipped path: a rule pair at 2^20 + 3 cells
    under mall_mb = 0 (the rule fires) and a 1-byte pair at an odd offset (the peel)."""
    L, E = ec.lib(), ec._ffi
    with ec.tuned(mall_mb=0):
        for v in values:
            before = _tune(ec)
            assert L.ec_tune_set(knob.encode(), v) == E.EC_ERR_ARG, (knob, v)
            assert _tune(ec) == before
            r0 = _stat(ec, b"binop_lds_rule_launches")
            _check_binop(ec, data, eco.F64, eco.U16, eco.DIV, 0, NBIG)
            assert _stat(ec, b"binop_lds_rule_launches") == r0 + 1
            _check_binop(ec, data, eco.U8, eco.I8, eco.SUB, 1, N)


# ---------------------------------------------------------------- ec_expr_source names the kernel the launch takes
def test_expr_source_and_the_launch_agree(ec, data):
    """The report of `ec_expr_source` and `expr_fixed_launches` agree: the plain catalogue programs, a dead stream of another width
    (fixed kernel, both sides), streams of different widths (neither); and one buffer under two names, which only the launch can
    see: the report names the formula, the launch takes the interpreter."""
    host, dev, _, _ = data
    ndvi = FIXED["NDVI"][2]
    cases = [([eco.F32, eco.F32], [], ndvi), ([eco.F32, eco.F32, eco.F64], [], ndvi), ([eco.U16, eco.F32], [], ndvi),
             ([eco.U8, eco.F32, eco.F32], [], [(eco.SUB, S(1), S(2), 0), (eco.ADD, S(1), S(2), 1), (eco.DIV, R(0), R(1), 0)]),
             ([eco.I16, eco.I16, eco.I16, eco.F64], [], FIXED["add-mul"][2])]
    cases += [([eco.U16] * ns, sc, st) for ns, sc, st in FIXED.values()]
    with ec.tuned(expr_jit=0):
        for cts, scalars, steps in cases:
            report = ec.fused.program_source(cts, len(scalars), steps).splitlines()[1]
            named = "none" not in report
            f0 = _stat(ec, b"expr_fixed_launches")
            _program(ec, data, cts, scalars, steps, 0, 4099, False)
            assert (_stat(ec, b"expr_fixed_launches") - f0 == 1) == named, (cts, report)
        # aliasing: the same buffer as both NDVI bands
        assert "NDVI" == ec.fused.program_source([eco.I16, eco.I16], 0, ndvi).splitlines()[1].split(": ", 1)[1]
        a = dev[eco.I16].shard(0, N)
        f0, i0 = _stat(ec, b"expr_fixed_launches"), _stat(ec, b"expr_interp_launches")
        got = ec.fused.program([a, a], [], ndvi)
        assert _stat(ec, b"expr_fixed_launches") == f0 and _stat(ec, b"expr_interp_launches") == i0 + 1
        eo, loose = _oracle_steps([host[eco.I16][:N]] * 2, [], ndvi)
        assert_f64_bits_equal(got.to_numpy(), eo, nan_by_class_where=loose)


# ---------------------------------------------------------------- knobs turned while other threads launch
def test_knobs_turned_while_three_threads_launch(ec, data):
    """The header's promise — each knob an atomic word that may be set while other host threads launch — once: three threads run a
    rule-pair binop, min_max and an expression program on their own streams against answers computed beforehand, while a fourth
    cycles binop_variant, binop_lds_kb, map_u, reduce_shape and fused_lds_kb through their values."""
    host, dev, _, _ = data
    L, E = ec.lib(), ec._ffi
    n = NBIG
    a, b = dev[eco.F64].shard(0, n), dev[eco.U16].shard(0, n)
    want_bin = eco.f_binop(eco.DIV, host[eco.F64][:n], host[eco.U16][:n])
    want_mm = eco.f_min_max(host[eco.F32][:N])
    ns, scalars, steps = FIXED["EVI"]
    prog_in = [dev[eco.U16].shard(k, N) for k in range(ns)]
    want_prog, loose_prog = _oracle_steps([host[eco.U16][k:k + N] for k in range(ns)], scalars, steps)
    grids = {"binop_variant": [-1, 0, 1], "binop_lds_kb": [-1, 0, 32, 64], "map_u": [1, 2, 4], "reduce_shape": [0, 1, 2, 3, 4],
             "fused_lds_kb": [0, 16, 64]}
    streams = []
    for _ in range(3):
        h = C.c_void_p()
        E.check(L.ec_stream_create(C.byref(h)))
        streams.append(h.value)
    outs = [ec.CellBuffer.empty(n, ec.Float64), ec.CellBuffer.empty(N, ec.Float64)]
    ec.synchronize()
    dt = (C.c_uint8 * ns)(*[eco.U16] * ns)
    ptrs = (C.c_void_p * ns)(*[x.mem.ptr for x in prog_in])
    sc = (ec.buffer.EcValue * len(scalars))(*[ec.CellValue.new(x).to_ec() for x in scalars])
    st = (E.EcExprStep * len(steps))(*[E.EcExprStep(*s_) for s_ in steps])
    stop = time.time() + 6.0
    errors, counts = [], [0] * 4

    def guard(k, fn):
        def run():
            try:
                while time.time() < stop and not errors:
                    fn()
                    counts[k] += 1
            except BaseException as e:  # noqa: BLE001
                errors.append((k, repr(e)))
                traceback.print_exc()
        return run

    def t_binop():
        E.check(L.ec_binop(eco.DIV, eco.F64, a.mem.ptr, eco.U16, b.mem.ptr, n, outs[0].mem.ptr, streams[0]))
        E.check(L.ec_stream_sync(streams[0]))
        assert np.array_equal(bits_of(outs[0].to_numpy()), bits_of(want_bin))

    def t_min_max():
        mn, mx = ec.buffer.EcValue(), ec.buffer.EcValue()
        E.check(L.ec_min_max(eco.F32, dev[eco.F32].mem.ptr, None, N, C.byref(mn), C.byref(mx), streams[1]))
        got = ec.CellValue.from_ec(mn), ec.CellValue.from_ec(mx)
        assert (got[0].bits(), got[1].bits()) == (want_mm[0].bits(), want_mm[1].bits())

    def t_expr():
        E.check(L.ec_expr(dt, ptrs, ns, sc, len(scalars), st, len(steps), N, outs[1].mem.ptr, streams[2]))
        E.check(L.ec_stream_sync(streams[2]))
        assert_f64_bits_equal(outs[1].to_numpy(), want_prog, nan_by_class_where=loose_prog)

    def t_knobs():
        i = counts[3]
        for key, grid in grids.items():
            E.check(L.ec_tune_set(key.encode(), grid[i % len(grid)]))
        time.sleep(0.0005)

    with ec.tuned(mall_mb=0, expr_jit=0, **{k: v[0] for k, v in grids.items()}):
        threads = [threading.Thread(target=guard(k, f)) for k, f in enumerate([t_binop, t_min_max, t_expr, t_knobs])]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=30)
        alive = [t for t in threads if t.is_alive()]
    for h in streams:
        E.check(L.ec_stream_sync(h))
        E.check(L.ec_stream_destroy(h))
    assert not alive, "a thread did not finish"
    assert not errors, errors[:3]
    assert all(c > 0 for c in counts), counts
