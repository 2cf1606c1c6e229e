"""The numpy restatement of the per-cell order (tests/compare_ref.py) against the oracle, and the kernels' own per-cell function
against the restatement — without a GPU.

1. `compare_ref.cmp3` is held to `eco.value_cmp` (impl Ord for CellValue, src/value.rs:248-265) cell by cell, for all 100 type
   pairs, over the cross product of the special-values table per type (signalling NaNs in the same-type float pairs only).
2. erased-cells_amd/host/test_compare_cell.cpp runs `cell_cmp` from csrc/ec_compare_cell.hpp alone — the function the kernels
   run — over the same table for all 100 pairs and 6 relations; its answers are compared with `compare_ref.relation`.  Built
   plain and under the address and undefined-behaviour sanitizers.  A stand-alone program: nothing of it is loaded into Python.
"""
import numpy as np
import pytest

import compare_ref as R
from host_program import run_host_program
from oracle import eco


def test_lattice_and_table():
    for a in range(R.NT):
        for b in range(R.NT):
            assert R.union(a, b) == eco.union(a, b), (a, b)
    assert R.NP == [np.dtype(d) for d in eco.NP_DTYPES]
    # the table holds what the issue lists, where the type holds it
    assert {2**24, 2**24 + 1, 2**53, 2**53 + 1, 2**63, 2**64 - 1, 0, 1} <= set(int(x) for x in R.specials(R.U64))
    assert {-2**63, 2**63 - 1, -1, 2**53 + 1} <= set(int(x) for x in R.specials(R.I64)) and 2**63 not in set(int(x) for x in R.specials(R.I64))
    assert set(int(x) for x in R.specials(R.I8)) == {-128, 127, 0, 1, -1}
    for ct in (R.F32, R.F64):
        t = R.specials(ct)
        assert np.isnan(t).sum() == 4 and np.signbit(t[np.isnan(t)]).sum() == 2 and np.isinf(t).sum() == 2
        assert (np.signbit(t) & (t == 0)).sum() == 1 and ((t != 0) & (np.abs(t) < np.finfo(t.dtype).tiny)).sum() == 3
        assert np.isnan(R.specials(ct, signalling=True)).sum() == 6


@pytest.mark.parametrize("lt", range(R.NT))
def test_cmp3_restates_the_oracle(lt):
    for rt in range(R.NT):
        l, r = R.cross(lt, rt)
        got = R.cmp3(lt, l, rt, r)
        exp = np.array([eco.value_cmp(eco.Value.of(lt, x), eco.Value.of(rt, y)) for x, y in zip(l, r)], dtype=np.int8)
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, (R.NAMES[lt], R.NAMES[rt], l[bad[0]], r[bad[0]], int(got[bad[0]]), int(exp[bad[0]]))
        for rel in R.RELS:   # the truth table over Ordering
            want = {R.LT: exp < 0, R.EQ: exp == 0, R.LE: exp <= 0, R.GT: exp > 0, R.NE: exp != 0, R.GE: exp >= 0}[rel]
            assert np.array_equal(R.relation(rel, lt, l, rt, r), want.astype(np.uint8)), (R.NAMES[lt], R.NAMES[rt], rel)
        # a scalar on the right broadcasts
        assert np.array_equal(R.cmp3(lt, l[:7], rt, r[3]), R.cmp3(lt, l[:7], rt, np.full(7, r[3])))


def test_the_stated_examples():
    """The cells the header names: the union decides, and floats follow the total order."""
    assert R.cmp3(R.U64, np.uint64(2**53 + 1), R.I64, np.int64(2**53)) == 0           # Equal: the union is Float64
    assert R.cmp3(R.I64, np.int64(2**53), R.I64, np.int64(2**53 + 1)) == -1           # not Equal
    f = np.float64
    assert R.cmp3(R.F64, f(-0.0), R.F64, f(0.0)) == -1
    neg_nan, pos_nan = np.array([0xFFF8000000000000, 0x7FF8000000000000], np.uint64).view(np.float64)
    assert R.cmp3(R.F64, neg_nan, R.F64, f(-np.inf)) == -1 and R.cmp3(R.F64, pos_nan, R.F64, f(np.inf)) == 1
    assert R.cmp3(R.F64, pos_nan, R.F64, pos_nan) == 0


def _lines_and_expected():
    lines, expected = [], []
    for lt in range(R.NT):
        for rt in range(R.NT):
            l, r = R.cross(lt, rt)
            lb = np.ascontiguousarray(l).view(f"u{l.dtype.itemsize}").astype(np.uint64)
            rb = np.ascontiguousarray(r).view(f"u{r.dtype.itemsize}").astype(np.uint64)
            lines += [f"{lt} {rt} {x:x} {y:x}" for x, y in zip(lb.tolist(), rb.tolist())]
            cols = np.stack([R.relation(rel, lt, l, rt, r) for rel in R.RELS], axis=1)
            expected += ["".join(map(str, row)) for row in cols.tolist()]
    return lines, expected


@pytest.mark.parametrize("target", ["test_compare_cell", "test_compare_cell_san"])
def test_cell_cmp_from_the_header_alone(target):
    lines, expected = _lines_and_expected()
    assert len(lines) >= 6000
    r = run_host_program(target, stdin="\n".join(lines) + "\n", passed=f"all lines answered: {len(lines)}")
    out = r.stdout.split("\n")
    assert out[len(lines)] == f"all lines answered: {len(lines)}"
    bad = [i for i, (g, e) in enumerate(zip(out, expected)) if g != e]
    assert not bad, (len(bad), lines[bad[0]], out[bad[0]], expected[bad[0]])
