"""The inputs of tests/test_gpu_compare.py can tell a right compare / select kernel from a wrong one — checked here without a GPU.

For each mistake a kernel of this family can make, `compare_ref` holds a numpy model of the kernel that makes it; the inputs the
GPU file uses (`gpu_inputs`, `gpu_masks`, `select_inputs`, the length `tail_len`) must contain a cell where the wrong kernel's
answer differs from the right one, for every type pair the mistake applies to.  An input set that passed a faulty model would
show nothing on the GPU either.
"""
import numpy as np
import pytest

import compare_ref as R

FLOATS = (R.F32, R.F64)
ALL_PAIRS = [(lt, rt) for lt in range(R.NT) for rt in range(R.NT)]


def _applies(kind, lt, rt):
    u = R.union(lt, rt)
    if kind == "f64_whatever_the_union":          # f64 merges neighbours beyond 2^53: both cells must be 64-bit integers of one type
        return lt == rt and u in (R.U64, R.I64)
    if kind == "signed_compare_of_u64":
        return u == R.U64
    if kind == "raw_bits_of_floats":              # raw bits order two NEGATIVE floats the wrong way round: both sides must hold negatives
        return (lt in FLOATS or rt in FLOATS) and R.NP[lt].kind != "u" and R.NP[rt].kind != "u"
    return lt in FLOATS or rt in FLOATS            # IEEE compare: a float operand brings NaNs and -0.0


@pytest.mark.parametrize("kind", R.VALUE_FAULTS)
def test_value_faults_change_an_answer(kind):
    pairs = [p for p in ALL_PAIRS if _applies(kind, *p)]
    assert pairs
    for lt, rt in pairs:
        l, r = R.gpu_inputs(lt, rt)
        changed = [rel for rel in R.RELS if not np.array_equal(R.relation(rel, lt, l, rt, r), R.relation_faulty(kind, rel, lt, l, rt, r))]
        assert changed, (kind, R.NAMES[lt], R.NAMES[rt])


@pytest.mark.parametrize("kind", R.MASK_FAULTS)
def test_mask_faults_change_an_answer(kind):
    for lt, rt in ALL_PAIRS:
        l, r = R.gpu_inputs(lt, rt)
        n = R.tail_len(l.size)
        l, r = l[:n], r[:n]
        lm, rm = R.gpu_masks(n)
        cpl = 16 // max(R.NP[lt].itemsize, R.NP[rt].itemsize)
        assert n % cpl != 0
        # the GPU file runs LT and GE on every pair's masked forms: one of the two is 0 in any tail cell
        changed = [rel for rel in (R.LT, R.GE)
                   if not np.array_equal(R.masked_relation(rel, lt, l, lm, rt, r, rm), R.masked_relation_faulty(kind, rel, lt, l, lm, rt, r, rm, cpl))]
        assert changed, (kind, R.NAMES[lt], R.NAMES[rt])


@pytest.mark.parametrize("kind", R.SELECT_FAULTS)
def test_select_faults_change_an_answer(kind):
    for ct in range(R.NT):
        sel, a, am, b, bm = R.select_inputs(ct)
        good, bad = R.masked_select(sel, a, am, b, bm), R.masked_select_faulty(kind, sel, a, am, b, bm)
        if kind == "sel_inverted":
            assert not np.array_equal(good[0].view(np.uint8), bad[0].view(np.uint8)), R.NAMES[ct]
        assert not np.array_equal(good[1], bad[1]), (kind, R.NAMES[ct])


def test_ties_are_planted():
    """Equal must be a common answer, not a rare one: LE / GE / EQ / NE differ from LT / GT only there."""
    for lt, rt in ALL_PAIRS:
        l, r = R.gpu_inputs(lt, rt)
        ties = int((R.cmp3(lt, l, rt, r) == 0).sum())
        assert ties >= 20, (R.NAMES[lt], R.NAMES[rt], ties)
        # every Ordering occurs (u16 cells are rarely below u8 cells: the special-values table provides those)
        assert (R.cmp3(lt, l, rt, r) < 0).any() and (R.cmp3(lt, l, rt, r) > 0).any()
