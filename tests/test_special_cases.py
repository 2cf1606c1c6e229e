"""The special-operand tests without a GPU: the exact reference (tests/ieee_ref.py) against the oracle and against its own array
form, what the inputs of tests/special_cases.py contain, and fault models: a cell rule changed in one of the ways a kernel can get it
wrong must change a cell of the inputs tests/test_gpu_special_cases.py runs — otherwise those inputs could not tell."""
import functools

import numpy as np
import pytest

import ieee_ref as R
import special_cases as sc
from oracle import eco
from vectors import bits_of

NT = 10
OPS = sc.OPS
FLOATS = (R.F32, R.F64)


def test_cell_type_numbers_are_the_oracles():
    assert (R.U8, R.U16, R.U32, R.U64, R.I8, R.I16, R.I32, R.I64, R.F32, R.F64) == (
        eco.U8, eco.U16, eco.U32, eco.U64, eco.I8, eco.I16, eco.I32, eco.I64, eco.F32, eco.F64)
    assert (R.ADD, R.SUB, R.MUL, R.DIV) == (eco.ADD, eco.SUB, eco.MUL, eco.DIV)
    assert [np.dtype(d) for d in R.NP_DTYPES] == [np.dtype(d) for d in eco.NP_DTYPES]


# ---------------------------------------------------------------- a. reference against reference
_exact_cache = {}


def _exact(op, a, b):
    key = (op, a, b)
    if key not in _exact_cache:
        _exact_cache[key] = R.binop_exact(op, a, b)
    return _exact_cache[key]


def _raw_bits(x: np.ndarray):
    return [int(v) for v in bits_of(x)]


@pytest.mark.parametrize("lt", range(NT), ids=eco.CT_NAMES)
def test_exact_reference_oracle_and_array_form_agree_on_the_lattice(lt):
    """Layout A's cells (the lattice; A repeats it) for every right type and op: the oracle's cell is in the exact reference's
    set, and the array form's pair is that set.  Widening is checked on the way: scalar against array form."""
    for rt in range(NT):
        l, r = sc.lattice(lt, rt)
        a, b = R.widen_vec(l), R.widen_vec(r)
        assert [R.widen_bits(lt, x) for x in _raw_bits(l)] == a.tolist(), (lt, rt)
        assert [R.widen_bits(rt, x) for x in _raw_bits(r)] == b.tolist(), (lt, rt)
        for op in OPS:
            want = [_exact(op, int(x), int(y)) for x, y in zip(a, b)]
            got = bits_of(eco.f_binop(op, l, r)).tolist()
            first, second = R.binop_vec(op, a, b)
            for i, w in enumerate(want):
                assert got[i] in w, (eco.CT_NAMES[lt], eco.CT_NAMES[rt], op, i, hex(int(a[i])), hex(int(b[i])), hex(got[i]), [hex(x) for x in w])
                assert {int(first[i]), int(second[i])} == w, (lt, rt, op, i, hex(int(a[i])), hex(int(b[i])))
            # the reference-shaped loop of the oracle: in the same sets (in a two-answer cell its compiler may pick the other operand)
            shaped = bits_of(eco.binop(op, l, r))
            assert R.allowed(np.stack([first, second]), shaped).all(), (lt, rt, op)


def _oracle_program(streams, scalars, steps):
    n = min(len(s) for s in streams)
    val = {k: s[:n] for k, s in enumerate(streams)}
    for k, c in enumerate(scalars):
        val[8 + k] = np.full(n, c, dtype=np.uint64).view(np.float64)
    last = None
    for op, a, b, dst in steps:
        val[4 + dst] = eco.f_binop(op, val[a], val[b])
        last = 4 + dst
    return bits_of(val[last])


@pytest.mark.parametrize("ct", FLOATS, ids=["f32", "f64"])
def test_program_reference_against_the_oracle_on_t3(ct):
    """Two-step chains on T^3, the first result as the left and as the right operand, all 16 op pairs: the oracle's chain is in
    the exact form's sets, and the array form's columns are those sets."""
    streams = sc.chain_grid([ct] * 3)
    wide = [R.widen_vec(s) for s in streams]
    for o1, o2 in sc.OP_PAIRS:
        for steps in ([(o1, 0, 1, 0), (o2, 4, 2, 1)], [(o1, 0, 1, 0), (o2, 2, 4, 1)]):
            got = _oracle_program(streams, [], steps)
            sets = R.program([w.tolist() for w in wide], [], steps)
            alts = R.program(wide, [], steps)
            assert R.allowed(alts, got).all(), (ct, steps)
            for i, s in enumerate(sets):
                assert int(got[i]) in s and set(alts[:, i].tolist()) == s, (ct, steps, i)


# ---------------------------------------------------------------- b. what the inputs contain
def _classes(bits64: np.ndarray):
    """Class of each f64: +0 -0 +inf -inf qnan snan subnormal normal max."""
    out = []
    for b in bits64.tolist():
        m = b & ~R.SIGN
        if m == 0:
            out.append("-0" if b & R.SIGN else "+0")
        elif m == R.INF:
            out.append("-inf" if b & R.SIGN else "+inf")
        elif m > R.INF:
            out.append("qnan" if b & R.QUIET else "snan")
        elif m < (1 << 52):
            out.append("subnormal")
        elif m == 0x7FEFFFFFFFFFFFFF:
            out.append("max")
        else:
            out.append("normal")
    return out


ALL_CLASSES = {"+0", "-0", "+inf", "-inf", "qnan", "snan", "subnormal", "normal", "max"}


def _own_classes(ct):
    """Classes of a float type's specials in their own format (an f32 subnormal, max or signalling NaN is none once widened)."""
    sp = sc.specials(ct)
    if ct == R.F64:
        return _classes(bits_of(sp))
    out = []
    for b in bits_of(sp).tolist():
        m = b & 0x7FFFFFFF
        out.append(("-0" if b >> 31 else "+0") if m == 0 else ("-inf" if b >> 31 else "+inf") if m == 0x7F800000 else
                   ("qnan" if b & 0x400000 else "snan") if m > 0x7F800000 else "subnormal" if m < 0x800000 else
                   "max" if m == 0x7F7FFFFF else "normal")
    return out


@pytest.mark.parametrize("lt", FLOATS)
@pytest.mark.parametrize("rt", FLOATS)
def test_every_pair_of_float_classes_occurs(lt, rt):
    cl, cr = _own_classes(lt), _own_classes(rt)
    assert set(cl) == ALL_CLASSES and set(cr) == ALL_CLASSES
    seen = {(x, y) for x in cl for y in cr}   # the lattice is the cross product of the two lists
    assert seen == {(x, y) for x in ALL_CLASSES for y in ALL_CLASSES}
    l, r = sc.lattice(lt, rt)
    assert len(l) == len(cl) * len(cr)


def _events(op, a, b):
    """The events of one exact cell `a op b` (f64 bits)."""
    ev = set()
    res = _exact(op, a, b)
    fin = lambda x: (x & ~R.SIGN) < R.INF  # noqa: E731
    zero = lambda x: (x & ~R.SIGN) == 0  # noqa: E731
    if R.is_nan(a) or R.is_nan(b):
        return ev
    (r,) = res
    if r == R.DEFAULT_NAN:
        ainf, azero = not fin(a), zero(a)
        ev.add({R.ADD: "inf+-inf", R.SUB: "inf-inf", R.MUL: "inf*0" if ainf else "0*inf", R.DIV: "0/0" if azero else "inf/inf"}[op])
        return ev
    if fin(a) and fin(b) and not fin(r) and not (op == R.DIV and zero(b)):
        ev.add("overflow")
    if 0 < (r & ~R.SIGN) < (1 << 52):
        ev.add("subnormal result")
    if zero(r) and not zero(a) and not zero(b) and fin(a) and fin(b) and op in (R.MUL, R.DIV):
        ev.add("underflow to zero")
    if r == R.SIGN and (zero(a) or zero(b) or (op in (R.MUL, R.DIV) and not fin(b))):
        ev.add("exact -0")
    if op == R.DIV and fin(a) and fin(b) and not zero(a) and not zero(b) and fin(r):
        with np.errstate(all="ignore"):
            x, y = np.float64(R.bits_f64(a)), np.float64(R.bits_f64(b))
            if R.f64_bits(float(x * (np.float64(1.0) / y))) != r:
                ev.add("a*(1/b) differs")
    return ev


# A sum or difference of two f64 is exact whenever it is subnormal, so it cannot underflow to zero: x - y == 0 only for x == y.
WANTED_EVENTS = {
    R.ADD: {"inf+-inf", "overflow", "subnormal result", "exact -0"},
    R.SUB: {"inf-inf", "overflow", "subnormal result", "exact -0"},
    R.MUL: {"inf*0", "0*inf", "overflow", "subnormal result", "underflow to zero", "exact -0"},
    R.DIV: {"0/0", "inf/inf", "overflow", "subnormal result", "underflow to zero", "exact -0", "a*(1/b) differs"},
}


@pytest.mark.parametrize("lt,rt", [(R.F64, R.F64), (R.F32, R.F32), (R.F32, R.F64), (R.F64, R.F32)])
def test_every_result_event_occurs_under_every_op(lt, rt):
    l, r = sc.lattice(lt, rt)
    a, b = R.widen_vec(l).tolist(), R.widen_vec(r).tolist()
    for op in OPS:
        seen = set()
        for x, y in zip(a, b):
            seen |= _events(op, x, y)
        want = set(WANTED_EVENTS[op])
        if (lt, rt) == (R.F32, R.F32):
            # two widened f32 cannot overflow or underflow an f64 sum or product: |x| in [2^-149, 2^128); only the quotient
            # max / 2^-149 stays finite too.  The events that need f64 extremes are pinned by the pairs with an f64 operand.
            want -= {"overflow", "subnormal result", "underflow to zero"}
        elif R.F32 in (lt, rt) and op in (R.ADD, R.SUB):
            want -= {"overflow"}   # a sum overflows only when both terms are near 2^1023; an f32 stays below 2^128
        assert want <= seen, (lt, rt, op, want - seen)


_predicted_two_answer_cells = sc.predicted_two_answer_cells


def test_two_answer_cells_are_what_the_lists_predict():
    assert _predicted_two_answer_cells(R.F64, R.F64) == 36
    total = {}
    for lt in range(NT):
        for rt in range(NT):
            l, r = sc.lattice(lt, rt)
            a, b = R.widen_vec(l), R.widen_vec(r)
            count = 0
            for op in OPS:
                first, second = R.binop_vec(op, a, b)
                count += int((first != second).sum())
                assert op in (R.ADD, R.MUL) or (first == second).all()
            assert count == _predicted_two_answer_cells(lt, rt), (lt, rt)
            total[lt, rt] = count
    assert all(v == 0 for (lt, rt), v in total.items() if lt not in FLOATS or rt not in FLOATS)


def test_layout_b_isolates_every_special_cell_and_layout_c_covers_head_and_tail():
    for lt, rt in sc.FLOAT_PAIRS + [(R.U8, R.I16)]:
        l, r, pos = sc.layout_b(lt, rt)
        k = len(sc.nan_pairs(lt, rt))
        assert len(pos) == 2 * k and (pos[:k] % 2 == 0).all() and (pos[k:] % 2 == 1).all()
        assert np.diff(pos).min() > 1536 and pos[0] > 1536 and len(l) - pos[-1] > 1536   # no other special cell within the widest tile
        a, b = R.widen_vec(l), R.widen_vec(r)
        special = np.zeros(len(l), bool)
        for op in OPS:
            special |= R.nan_vec(R.binop_vec(op, a, b)[0])
        assert set(np.flatnonzero(special).tolist()) == set(pos.tolist())
        ll, rr = sc.lattice(lt, rt)
        idx = sc.nan_pairs(lt, rt)
        assert np.array_equal(bits_of(l[pos[:k]]), bits_of(ll[idx])) and np.array_equal(bits_of(r[pos[k:]]), bits_of(rr[idx]))
        cl, cr, wins = sc.layout_c(lt, rt)
        assert len(wins) == 5 * k and {n for _, n in wins} == {1, 2, 3, 5, 7}
        assert all((s % 2 == 1) == (n == 7) for s, n in wins)


# ---------------------------------------------------------------- c. fault models
# A model is the cell rule as a kernel would compute it with one thing wrong.  The kernel's geometry: `head` cells peeled (a window
# that starts at an odd cell), tiles of TILE cells of which the full ones run the pairwise code (one NaN test per pair of cells, a
# repair behind a wave-wide ballot: waves of 64 lanes x 2 cells), the ragged tile and the odd tail cell the per-cell code.
TILE, WAVE = 1024, 128
Q, GPU_NAN, X86_NAN = np.uint64(R.QUIET), np.uint64(R.GPU_DEFAULT_NAN), np.uint64(R.DEFAULT_NAN)
MANT = np.uint64((1 << 52) - 1)
ABS = np.uint64(~R.SIGN & (2 ** 64 - 1))
SIGN = np.uint64(R.SIGN)


def _flush(x):
    sub = ((x & ABS) < np.uint64(1 << 52)) & ((x & ABS) != 0)
    return np.where(sub, x & SIGN, x)


def _widen(arr, m):
    if arr.dtype == np.float32 and m is not None and m.startswith("f32 nan without"):
        b = arr.view(np.uint32).astype(np.uint64)
        nan = (b & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
        sign = (b >> np.uint64(31)) << np.uint64(63)
        if m == "f32 nan without the shift":
            made = sign | np.uint64(R.EXP | R.QUIET) | (b & np.uint64(0x7FFFFF))
        else:
            made = sign | np.uint64(R.EXP) | ((b & np.uint64(0x7FFFFF)) << np.uint64(29))
        return np.where(nan, made, R.widen_vec(arr))
    return R.widen_vec(arr)


def _body(n, head):
    i = np.arange(n)
    return (i >= head) & (i < head + (n - head) // TILE * TILE)


def _cell(op, a, b, m, head=0, last=True, scalar_operand=False, narrow=False):
    """One step over arrays of f64 bits under model `m` (None: the rule itself, lhs-first)."""
    n = len(a)
    if m == "subnormal operands flushed":
        a, b = _flush(a), _flush(b)
    if m == "a * (1/b)" and op == R.DIV:
        with np.errstate(all="ignore"):
            r = (a.view(np.float64) * (1.0 / b.view(np.float64))).view(np.uint64)
    else:
        r = R.arith_vec(op, a, b)
    if m == "subnormal results flushed":
        r = _flush(r)
    na, nb, nr = R.nan_vec(a), R.nan_vec(b), R.nan_vec(r)
    q = np.uint64(0) if m is not None and m.endswith("no quieting") else Q
    dflt = GPU_NAN if m == "positive default nan" else X86_NAN
    if m == "rhs first":
        fix = np.where(nb, b | q, np.where(na, a | q, dflt))
    else:
        fix = np.where(na, a | q, np.where(nb, b | q, dflt))
    # what the GPU's instruction leaves when nobody repairs: a quieted operand (the later one when both are NaNs), its own default NaN
    raw = np.where(nb, b | Q, np.where(na, a | Q, GPU_NAN))
    i = np.arange(n)
    rep = np.ones(n, bool)
    if m == "repair at even indices only":
        rep = i % 2 == 0
    elif m == "repair at odd indices only":
        rep = i % 2 == 1
    elif m == "no repair in head and tail cells":
        rep = _body(n, head)
    elif m == "repair only with two nan lanes in a wave":
        body = _body(n, head)
        lane_nan = np.zeros((n - head + 1) // 2 + 1, bool)
        np.logical_or.at(lane_nan, (i[body] - head) // 2, nr[body])
        per_wave = np.add.reduceat(lane_nan.astype(int), np.arange(0, len(lane_nan), WAVE // 2))
        rep = ~body | (per_wave[np.clip((i - head) // WAVE, 0, len(per_wave) - 1)] >= 2)
    elif m == "repair after the last step only":
        rep = np.full(n, last)
    elif m == "small shortcut with a scalar operand" and scalar_operand and narrow:
        rep = np.zeros(n, bool)
    return np.where(nr, np.where(rep, fix, raw), r)


def _fma(a, b, c):
    """fma(a, b, c) of f64 bits arrays where all three are finite, rounded once; elsewhere None is left to the two-step form."""
    from fractions import Fraction
    out = {}
    for k, (x, y, z) in enumerate(zip(a.tolist(), b.tolist(), c.tolist())):
        if all((v & ~R.SIGN) < R.INF for v in (x, y, z)):
            e = Fraction(R.bits_f64(x)) * Fraction(R.bits_f64(y)) + Fraction(R.bits_f64(z))
            if e != 0:
                out[k] = R._round(e)
    return out


def _run(streams, scalars, steps, m, head=0):
    """A program (one step: a binop) over raw cell arrays under model `m`: the cells such a kernel would write."""
    n = min(len(s) for s in streams)
    val = {k: _widen(s[:n], m) for k, s in enumerate(streams)}
    narrow = all(s.dtype.itemsize <= 2 and s.dtype.kind in "ui" for s in streams)
    for k, c in enumerate(scalars):
        val[8 + k] = np.full(n, c, dtype=np.uint64)
    made_by, last = {}, None
    for j, (op, ra, rb, dst) in enumerate(steps):
        a, b = val[ra], val[rb]
        out = _cell(op, a, b, m, head, j == len(steps) - 1, ra >= 8 or rb >= 8, narrow)
        if m == "a*k0+k1 contracted" and op == R.ADD and made_by.get(ra, (None,))[0] == R.MUL:
            for k, v in _fma(made_by[ra][1], made_by[ra][2], b).items():
                out[k] = v
        if m == "(a+b)*c contracted" and op == R.MUL and made_by.get(ra, (None,))[0] == R.ADD:
            bc = _cell(R.MUL, made_by[ra][2], b, None)
            for k, v in _fma(made_by[ra][1], b, bc).items():
                out[k] = v
        val[4 + dst], made_by[4 + dst], last = out, (op, a, b), 4 + dst
    return val[last]


def _caught(streams, scalars, steps, m, head=0):
    """Does model `m` write a cell outside the allowed set?  (The rule itself, m = None, never does.)"""
    alts = R.program([R.widen_vec(s) for s in streams], scalars, steps)
    n = alts.shape[1]
    assert R.allowed(alts, _run(streams, scalars, steps, None, head)[:n]).all()
    return not R.allowed(alts, _run(streams, scalars, steps, m, head)[:n]).all()


@functools.lru_cache(maxsize=None)
def _binop_sets(lt, rt):
    """The binop inputs of the GPU file for one type pair, by layout: lists of (streams, head)."""
    la, lb, lc = sc.layout_a(lt, rt), sc.layout_b(lt, rt), sc.layout_c(lt, rt)
    return {"A": [((la[0], la[1]), 0), ((la[0][1:], la[1][1:]), 1)],
            "B": [((lb[0], lb[1]), 0), ((lb[0][1:], lb[1][1:]), 1)],
            "C": [((lc[0][s:s + n], lc[1][s:s + n]), s & 1) for s, n in lc[2]]}


@functools.lru_cache(maxsize=None)
def _binop_alts(lt, rt, name, k, op):
    (l, r), head = _binop_sets(lt, rt)[name][k]
    alts = np.stack(R.binop_vec(op, R.widen_vec(l), R.widen_vec(r)))
    assert R.allowed(alts, _run([l, r], [], [(op, 0, 1, 0)], None, head)).all()
    return alts


def _layouts_catching(m, lt, rt, ops=OPS):
    out = set()
    for name, runs in _binop_sets(lt, rt).items():
        for k, ((l, r), head) in enumerate(runs):
            if name not in out and any(not R.allowed(_binop_alts(lt, rt, name, k, op), _run([l, r], [], [(op, 0, 1, 0)], m, head)).all()
                                       for op in ops):
                out.add(name)
    return out


RULE_MODELS = ["rhs first", "no quieting", "positive default nan"]
ARITH_MODELS = ["subnormal results flushed", "subnormal operands flushed", "a * (1/b)"]
# "without the quiet bit" alone changes no cell: the NaN rule quiets the operand it returns, whatever the widening left.  It shows
# together with "no quieting" — which on its own shows only with an f64 operand, the one type that can hold a signalling NaN.
WIDEN_MODELS = ["f32 nan without the shift", "f32 nan without the quiet bit, no quieting"]
BOTH_FLOAT = [p for p in sc.FLOAT_PAIRS if p[0] in FLOATS and p[1] in FLOATS]


@pytest.mark.parametrize("m", RULE_MODELS)
@pytest.mark.parametrize("pair", sc.FLOAT_PAIRS, ids=lambda p: f"{eco.CT_NAMES[p[0]]}-{eco.CT_NAMES[p[1]]}")
def test_a_wrong_nan_rule_changes_a_cell_of_every_layout(m, pair):
    """rhs-first needs two NaN operands (both types floats) and a `-` or `/`: under `+` and `*` the other operand is an allowed
    answer.  No quieting needs a signalling NaN that reaches the rule: an f64 operand.  The default NaN's sign shows under every op
    that has an invalid operation for the pair: inf +- inf needs an infinity on both sides."""
    both = pair in BOTH_FLOAT
    for op in OPS:
        got = _layouts_catching(m, *pair, ops=(op,))
        if m == "rhs first":
            want = {"A", "B", "C"} if both and op in (R.SUB, R.DIV) else set()
        elif m == "no quieting":
            want = {"A", "B", "C"} if R.F64 in pair else set()
        else:
            want = {"A", "B", "C"} if both or op in (R.MUL, R.DIV) else set()
        assert got == want, (m, pair, op, got)


def test_the_quiet_bit_of_a_widened_f32_nan_alone_changes_nothing():
    for lt, rt in ((R.F32, R.F32), (R.F32, R.F64), (R.F32, R.I16)):
        assert _layouts_catching("f32 nan without the quiet bit", lt, rt) == set()


@pytest.mark.parametrize("m", ARITH_MODELS)
def test_wrong_arithmetic_changes_a_cell_of_layout_a(m):
    """Flushed subnormals change cells that are no NaNs: only the plain cross product holds them (B and C are built from the NaN
    pairs, among ordinary cells) — layout A is the only layout that catches the two flush models.  A reciprocal multiply also
    shows in the ordinary cells around B's and C's pairs: their quotients are inexact."""
    for lt, rt in ((R.F64, R.F64), (R.F32, R.F64), (R.F64, R.F32), (R.F64, R.U64), (R.U8, R.F64)):
        assert _layouts_catching(m, lt, rt) == ({"A", "B", "C"} if m == "a * (1/b)" else {"A"}), (m, lt, rt)
    if m == "a * (1/b)":
        for lt, rt in ((R.F32, R.F32), (R.F32, R.I16), (R.I64, R.F32), (R.U8, R.U16), (R.I32, R.I32)):
            assert "A" in _layouts_catching(m, lt, rt, ops=(R.DIV,)), (m, lt, rt)


@pytest.mark.parametrize("m", WIDEN_MODELS)
def test_a_wrong_f32_nan_widening_changes_a_cell_of_every_layout(m):
    for lt, rt in ((R.F32, R.F32), (R.F32, R.F64), (R.F64, R.F32), (R.F32, R.I16), (R.I64, R.F32)):
        for op in OPS:
            assert _layouts_catching(m, lt, rt, ops=(op,)) == {"A", "B", "C"}, (m, lt, rt, op)


POSITION_MODELS = {
    # model: the layouts that must tell
    "repair at even indices only": {"A", "B", "C"},
    "repair at odd indices only": {"A", "B", "C"},
    # B's pairs sit in full tiles; A's head, tail and ragged-tile cells are whatever lattice cells land there, for some type pairs
    # and ops none that shows: only C is built for it
    "no repair in head and tail cells": {"C"},
    # A's waves hold dozens of NaN lanes and C has no full tile: only B plants one NaN lane in a wave
    "repair only with two nan lanes in a wave": {"B"},
}


@pytest.mark.parametrize("m", list(POSITION_MODELS))
def test_a_repair_that_depends_on_position_is_told_by_the_layout_built_for_it(m):
    """What an unrepaired cell shows is the GPU's own default NaN or the later operand, so these show in the invalid operations
    (every op has one for two float types) and in two different NaNs under `-` and `/`."""
    a_misses = False
    for lt, rt in BOTH_FLOAT:
        for op in OPS:
            got = _layouts_catching(m, lt, rt, ops=(op,))
            assert POSITION_MODELS[m] <= got, (m, lt, rt, op, got)
            if m == "repair only with two nan lanes in a wave":
                assert got == {"B"}, (m, lt, rt, op, got)
            if m == "no repair in head and tail cells":
                assert "B" not in got, (m, lt, rt, op, got)
                a_misses |= "A" not in got
    assert a_misses == (m == "no repair in head and tail cells")


def test_scalar_inputs_tell_every_rule_model():
    """buffer . scalar: layout B of one cell type against every f64 special as the scalar."""
    for ct in (R.F32, R.F64, R.I16, R.U64):
        cells, _ = sc.layout_b_single(ct)
        for m in RULE_MODELS + ["subnormal results flushed", "a * (1/b)", "repair at even indices only", "repair at odd indices only",
                                "repair only with two nan lanes in a wave"] + (WIDEN_MODELS if ct == R.F32 else []):
            if m == "rhs first" and ct not in FLOATS:
                continue  # two NaN operands need float cells
            caught = any(_caught([cells, np.full(len(cells), k, dtype=np.uint64).view(np.float64)], [], [(op, 0, 1, 0)], m)
                         for k in sc.SCALAR_BITS for op in OPS)
            assert caught, (ct, m)


def test_chains_tell_a_repair_that_waits_for_the_last_step():
    """Two-step chains on T^3 and the two-level shapes on T^4: an intermediate NaN left unrepaired shows in the result — under
    every op pair whose second step can carry a NaN's bits on (all of them: a NaN operand propagates)."""
    m = "repair after the last step only"
    for ct in FLOATS:
        t3 = sc.chain_grid([ct] * 3)
        for o1, o2 in sc.OP_PAIRS:
            assert _caught(t3, [], [(o1, 0, 1, 0), (o2, 4, 2, 1)], m), (ct, o1, o2)
            assert _caught(t3, [], [(o1, 0, 1, 0), (o2, 2, 4, 1)], m), (ct, o1, o2)
        t4 = sc.chain_grid([ct] * 4)
        for o1, o2, o3 in sc.OP_TRIPLES:
            assert _caught(t4, [], [(o1, 0, 1, 0), (o3, 2, 3, 1), (o2, 4, 5, 0)], m), (ct, o1, o2, o3)
    for m in RULE_MODELS:
        for o1, o2, o3 in sc.OP_TRIPLES:
            sees = m != "rhs first" or R.SUB in (o1, o2, o3) or R.DIV in (o1, o2, o3)   # under + and * alone either operand is allowed
            assert _caught(sc.chain_grid([R.F64] * 4), [], [(o1, 0, 1, 0), (o3, 2, 3, 1), (o2, 4, 5, 0)], m) == sees, (m, o1, o2, o3)
    mixed = sc.chain_grid([R.F32, R.F64, R.I16, R.U8])
    for m in RULE_MODELS + WIDEN_MODELS + ["repair after the last step only"]:
        assert any(_caught(mixed, [], [(o1, 0, 1, 0), (o3, 2, 3, 1), (o2, 4, 5, 0)], m) for o1, o2, o3 in sc.OP_TRIPLES), m


def test_formula_inputs_tell_the_small_shortcut_and_contraction():
    """The catalogue formulas: a NaN test dropped for a step that has a scalar operand (the shortcut is sound only for two narrow
    integer operands) shows at widths 1 and 2 with a special scalar; a contracted a*k0+k1 shows at every width on the witness
    cell, a distributed (a+b)*c at widths 4 and 8 (integer cells have no witness: their sums and products are exact)."""
    _, affine = sc.FORMULAS["affine"]
    _, addmul = sc.FORMULAS["add-mul"]
    _, evi = sc.FORMULAS["EVI"]
    for width in (1, 2, 4, 8):
        s = [sc.affine_stream(width)]
        k0, k1 = sc.AFFINE_WITNESS[width][1:]
        assert _caught(s, [k0, k1], affine, "a*k0+k1 contracted"), width
        assert not _caught(s, list(sc.AFFINE_ORDINARY), affine, "repair after the last step only")  # ordinary scalars: nothing to see
        if width <= 2:
            m = "small shortcut with a scalar operand"
            assert any(_caught(s, [a, b], affine, m) for a, b in sc.AFFINE_SCALARS), width
            assert any(_caught(sc.triple_streams(width), ks, evi, m) for ks in sc.EVI_SPECIAL), width
            assert not _caught(sc.triple_streams(width), sc.EVI_ORDINARY, evi, m)
        if width >= 4:
            assert _caught(sc.triple_streams(width), [], addmul, "(a+b)*c contracted"), width
            assert _caught(sc.triple_streams(width), sc.EVI_ORDINARY, evi, "repair after the last step only"), width
