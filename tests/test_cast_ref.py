"""The numpy restatement of ec_cast / ec_cast_scaled (tests/cast_ref.py) against things it shares no code with, and the kernels'
own per-cell functions against the restatement — without a GPU.

1. `cast_ref.cast` is held to the oracle's `eco.convert` for the 41 fitting pairs, to `resample_ref.to_cell` for ROUND from
   Float64, to `cast_ref.cast_scalar` (one cell in Python's exact integers) for every special value of every pair, and to it
   again over the whole value space of every 8- and 16-bit source into every destination.
2. The stated examples of the header and the issue, by hand.
3. erased-cells_amd/host/test_cast_cell.cpp runs cast_as / cast_round / scaled from csrc/ec_cast_cell.hpp alone — the functions
   the kernels run — over the special values of all 100 pairs; its answers are compared with `cast_ref`.  Built plain and under
   the address and undefined-behaviour sanitizers (float-cast-overflow named).  A stand-alone program: nothing of it is loaded
   into Python.
"""
from fractions import Fraction

import numpy as np
import pytest

import cast_ref as R
import resample_ref
from host_program import run_host_program
from oracle import eco

NT, NP, NAMES = R.NT, R.NP, R.NAMES


def _bad(got, want):
    return np.flatnonzero(~R.same_cells(got, want))


def test_the_lattice_and_the_table():
    pairs = [(s, d) for s in range(NT) for d in range(NT)]
    assert all(R.can_fit_into(s, d) == eco.can_fit_into(s, d) for s, d in pairs)
    fit = [p for p in pairs if R.can_fit_into(*p)]
    narrowing_int = [p for p in pairs if not R.can_fit_into(*p) and R.is_int(p[1])]
    assert (len(fit), len(pairs) - len(fit), len(narrowing_int)) == (41, 59, 54)
    t = R.specials(R.F64)
    have = set(t[np.isfinite(t)].tolist())
    for ct in range(8):
        lo, hi = R.limits(ct)
        want = [float(lo - 1), float(lo), float(hi), float(hi + 1)]
        for mid in (Fraction(2 * lo - 1, 2), Fraction(2 * hi + 1, 2)):
            f = np.float64(float(mid))
            want += [float(f), float(np.nextafter(f, np.inf)), float(np.nextafter(f, -np.inf))]
        assert set(want) <= have, (NAMES[ct], sorted(set(want) - have))
    assert {0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999999999999994, 5e-324, 2.0**24 - 1, 2.0**24 + 1, 2.0**53 - 1, 2.0**53 + 1, 2.0**31,
            -2.0**31, 2.0**63, -2.0**63, 2.0**64, R.FLT_MAX, float(np.nextafter(np.float64(R.FLT_MAX), np.inf)), 0.1} <= have
    assert np.isinf(t).sum() == 2 and (np.signbit(t) & (t == 0)).sum() == 1
    for ct in (R.F32, R.F64):
        s = R.specials(ct)
        assert np.isnan(s).sum() == 3 and np.signbit(s[np.isnan(s)]).sum() == 1
    assert {2**24 + 1, 2**53 + 1, 2**63, 2**64 - 1} <= set(int(v) for v in R.specials(R.U64))
    assert {-2**63, 2**63 - 1, 2**53 + 1, -2**31, 2**31} <= set(int(v) for v in R.specials(R.I64))


@pytest.mark.parametrize("st", range(NT), ids=NAMES)
def test_fitting_pairs_are_the_oracles_convert(st):
    x = R.specials(st)
    for dt in range(NT):
        if R.can_fit_into(st, dt):
            want = eco.convert(x, dt)
            for mode in R.MODES:
                got = R.cast(mode, st, x, dt)
                assert got.dtype == want.dtype and _bad(got, want).size == 0, (NAMES[st], NAMES[dt], mode)


@pytest.mark.parametrize("dt", range(NT), ids=NAMES)
def test_round_from_f64_is_the_resampling_rule(dt):
    x = R.specials(R.F64)
    got = R.cast(R.ROUND, R.F64, x, dt)
    want = np.array([resample_ref.to_cell(v, NP[dt]) for v in x], dtype=NP[dt])
    assert _bad(got, want).size == 0, (NAMES[dt], x[_bad(got, want)[:3]])


@pytest.mark.parametrize("st", range(NT), ids=NAMES)
def test_special_values_against_exact_integers(st):
    x = R.specials(st)
    for dt in range(NT):
        for mode in R.MODES:
            got = R.cast(mode, st, x, dt)
            want = np.array([R.cast_scalar(mode, st, v, dt) for v in x], dtype=NP[dt])
            bad = _bad(got, want)
            assert bad.size == 0, (NAMES[st], NAMES[dt], mode, x[bad[0]], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("st", [R.U8, R.I8, R.U16, R.I16], ids=lambda c: NAMES[c])
def test_the_whole_value_space_of_the_small_types(st):
    lo, hi = R.limits(st)
    ints = range(lo, hi + 1)
    x = np.array(ints, dtype=NP[st])
    for dt in range(NT):
        dlo, dhi = (R.limits(dt) if R.is_int(dt) else (None, None))
        bits = 8 * NP[dt].itemsize
        for mode in R.MODES:
            got = R.cast(mode, st, x, dt)
            if not R.is_int(dt):
                want = [float(v) for v in ints]                   # every 16-bit integer is an f32
            elif mode == R.ROUND or R.can_fit_into(st, dt):
                want = [min(max(v, dlo), dhi) for v in ints]
            else:
                want = [(v & ((1 << bits) - 1)) - ((1 << bits) if dlo < 0 and (v >> (bits - 1)) & 1 else 0) for v in ints]
            assert got.tolist() == want, (NAMES[st], NAMES[dt], mode)


def test_the_stated_examples():
    c = R.cast
    assert c(R.ROUND, R.I64, np.int64(2**53 + 1), R.U64) == 2**53 + 1                       # no detour through f64
    assert c(R.ROUND, R.U64, np.uint64(2**64 - 1), R.I64) == 2**63 - 1 and c(R.AS, R.U64, np.uint64(2**64 - 1), R.I64) == -1
    assert c(R.ROUND, R.I16, np.int16(-3), R.U8) == 0 and c(R.AS, R.I16, np.int16(-3), R.U8) == 253
    assert c(R.ROUND, R.I16, np.int16(300), R.U8) == 255 and c(R.AS, R.I16, np.int16(300), R.U8) == 44
    f = np.float64
    assert c(R.ROUND, R.F64, f(0.49999999999999994), R.I32) == 1 and c(R.AS, R.F64, f(0.49999999999999994), R.I32) == 0   # the one-add rule
    assert 0.49999999999999994 + 0.5 == 1.0
    assert [int(c(R.ROUND, R.F64, f(v), R.I8)) for v in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5)] == [1, 2, 3, -1, -2, -3]        # half away from zero
    assert [int(c(R.AS, R.F64, f(v), R.I8)) for v in (0.5, 1.5, 2.5, -0.5, -1.5, -2.9)] == [0, 1, 2, 0, -1, -2]
    assert c(R.ROUND, R.F64, f(2.0**63), R.I64) == 2**63 - 1 and c(R.ROUND, R.F64, f(2.0**64), R.U64) == 2**64 - 1
    assert c(R.ROUND, R.F64, f(-2.0**63), R.I64) == -2**63 and c(R.ROUND, R.F32, np.float32(2.0**31), R.I32) == 2**31 - 1
    for mode in R.MODES:
        assert c(mode, R.F64, f(np.nan), R.I16) == 0 and c(mode, R.F64, f(-np.inf), R.U8) == 0 and c(mode, R.F64, f(np.inf), R.U8) == 255
        assert np.isinf(c(mode, R.F64, f(np.nextafter(f(R.FLT_MAX), np.inf) * 2), R.F32))
        assert c(mode, R.F64, f(np.nextafter(f(R.FLT_MAX), np.inf)), R.F32) == np.float32(R.FLT_MAX)
        assert c(mode, R.U32, np.uint32(2**24 + 1), R.F32) == np.float32(2.0**24) and c(mode, R.U32, np.uint32(2**24 + 3), R.F32) == np.float32(2.0**24 + 4)
        neg_nan = np.array([0xFFF8000000000000], np.uint64).view(np.float64)
        assert np.isnan(c(mode, R.F64, neg_nan, R.F32))[0] and np.signbit(c(mode, R.F64, neg_nan, R.F32))[0]
    # the scale step: two roundings, never an fma
    assert R.scaled(R.F64, f(0.1), None, 10.0, -1.0, R.F64) == 0.0
    assert float(Fraction(0.1) * 10 - 1) == 2.0**-54                                           # what a fused evaluation gives
    assert R.scaled_faulty("fma", R.F64, np.array([0.1]), None, 10.0, -1.0, R.F64)[0] == 2.0**-54
    assert R.scaled(R.F64, np.array([0.12344, np.nan, -5.0]), np.array([1, 0, 1], np.uint8), 10000.0, 0.0, R.I16, -9999).tolist() == [1234, -9999, -32768]


def _lines_and_expected():
    lines, expected = [], []
    for st in range(NT):
        x = R.specials(st)
        xb = np.ascontiguousarray(x).view(f"u{x.dtype.itemsize}").astype(np.uint64).tolist()
        for dt in range(NT):
            ut = f"u{NP[dt].itemsize}"
            a, r = (np.ascontiguousarray(R.cast(m, st, x, dt)).view(ut) for m in R.MODES)
            lines += [f"{st} {dt} {b:x}" for b in xb]
            expected += [(dt, int(p), int(q)) for p, q in zip(a.tolist(), r.tolist())]
            for scale, offset in R.SCALED_PARAMS:
                sb, ob = (int(np.float64(v).view(np.uint64)) for v in (scale, offset))
                y = np.ascontiguousarray(R.scaled(st, x, None, scale, offset, dt)).view(ut)
                lines += [f"{st} {dt} {b:x} {sb:x} {ob:x}" for b in xb]
                expected += [(dt, int(p)) for p in y.tolist()]
    return lines, expected


def _same_line(answer: str, want) -> bool:
    """bit-equal, or (a float destination) NaN against NaN of the same sign"""
    dt, bits = want[0], want[1:]
    got = [int(t, 16) for t in answer.split()]
    if len(got) != len(bits):
        return False
    for g, w in zip(got, bits):
        if g != w:
            if R.is_int(dt):
                return False
            ut = np.uint32 if dt == R.F32 else np.uint64
            pair = np.array([g, w], dtype=ut).view(NP[dt])
            if not (np.isnan(pair).all() and np.signbit(pair[0]) == np.signbit(pair[1])):
                return False
    return True


@pytest.mark.parametrize("target", ["test_cast_cell", "test_cast_cell_san"])
def test_the_cell_functions_from_the_header_alone(target):
    lines, expected = _lines_and_expected()
    assert len(lines) >= 10000
    r = run_host_program(target, stdin="\n".join(lines) + "\n", passed=f"all lines answered: {len(lines)}")
    out = r.stdout.split("\n")
    assert out[len(lines)] == f"all lines answered: {len(lines)}"
    bad = [i for i, (g, e) in enumerate(zip(out, expected)) if not _same_line(g, e)]
    assert not bad, (len(bad), lines[bad[0]], out[bad[0]], [hex(v) for v in expected[bad[0]][1:]])
