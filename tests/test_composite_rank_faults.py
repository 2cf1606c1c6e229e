"""The inputs of tests/test_gpu_composite_rank.py can tell a right selection kernel from a wrong one — checked here without a GPU.

For each mistake a kernel of this family can make, `composite_rank_ref` holds a numpy model of the kernel that makes it
(`rank_faulty`).  For every cell type the mistake can touch, the main GPU cases (`stack(ct, k, main_len(ct), form)` over `KS`,
`FORMS`, `QS`, both methods and `min_counts(k)`) must contain a launch with a cell where the wrong kernel's value, mask byte or aux
byte differs from the right one.  An input set that passed a faulty model would show nothing on the GPU either.
"""
import numpy as np
import pytest

import composite_ref as CR
import composite_rank_ref as R


def _differs(a, b):
    return any(not R.same_cells(x, y).all() for x, y in zip(a, b))


def _launches(ct):
    """the main GPU cases of one cell type: (k, form) with the launches made on that stack"""
    for k in R.KS:
        for form in R.FORMS:
            yield k, form, [(num, den, method, mc) for num, den in R.QS for method in R.METHODS for mc in R.min_counts(k)]


@pytest.mark.parametrize("kind", R.FAULTS)
def test_every_fault_changes_an_answer_for_every_type_it_can_touch(kind):
    seen = 0
    for ct in range(R.NT):
        n = R.main_len(ct)
        exposed = applicable = False
        for k, form, launches in _launches(ct):
            todo = [l for l in launches if R.applies(kind, ct, k, form, *l)]
            if not todo:
                continue
            applicable = True
            layers, masks = R.stack(ct, k, n, form)
            od = R.ordered(ct, layers, masks)
            for num, den, method, mc in todo:
                good = R.pick(ct, od, num, den, method, mc)
                args = [j for j, m in enumerate(masks) if m is not None] if kind == "mask_ignored" else [None]
                # a mask that is ignored must show whichever layer's it is
                exposed = all(_differs(R.rank_faulty(kind, ct, layers, masks, num, den, method, mc, arg), good) for arg in args)
                if exposed:
                    break
            if exposed:
                break
        assert exposed or not applicable, (kind, R.NAMES[ct])
        seen += exposed
    assert seen, kind


def test_what_each_fault_can_touch():
    """the table `applies` is not empty-handed: each mistake reaches the types it is about"""
    reach = {kind: {ct for ct in range(R.NT) for k, form, ls in _launches(ct) for l in ls if R.applies(kind, ct, k, form, *l)} for kind in R.FAULTS}
    every = set(range(R.NT))
    for kind in R.FAULTS:
        if kind in ("ieee_less", "raw_float_bits"):
            assert reach[kind] == set(R.FLOATS)
        elif kind == "u64_signed":
            assert reach[kind] == {R.U64}
        elif kind == "sign_bias_forgotten":
            assert reach[kind] == {R.I8, R.I16}
        else:
            assert reach[kind] == every, kind
    assert len(R.FAULTS) >= 16


@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_the_inputs_hold_what_the_faults_need(ct):
    n = R.main_len(ct)
    for k in (3, 5, 64):
        layers, masks = R.stack(ct, k, n, "all")
        order, count, bits = R.ordered(ct, layers, masks)
        key = np.stack([R.order_key(ct, a) for a in layers])
        valid = np.stack(masks) != 0
        assert (count == 0).any() and (count == 1).any() and (count == k).any() and (count % 2 == 0)[count > 0].any() and (count % 2 == 1).any()
        # ties of equal keys between valid layers, in the middle of a cell's order too
        med = np.take_along_axis(order, ((count - 1) // 2)[None, :].clip(0), axis=0)[0]
        med_key = np.take_along_axis(key, med[None, :], axis=0)[0]
        assert ((valid & (key == med_key[None, :])).sum(axis=0) >= 2)[count > 0].any()
        if ct in R.FLOATS:
            zero = np.stack([R.words(a) for a in layers])
            sign = np.uint64(1) << np.uint64(8 * R.NP[ct].itemsize - 1)
            assert ((valid & (zero == 0)).any(axis=0) & (valid & (zero.astype(np.uint64) == sign)).any(axis=0)).any()   # -0.0 and +0.0 valid in one cell
            assert (np.isnan(np.stack(layers)) & ~valid).any()                                      # a NaN under a cleared mask byte
    # the tail is ragged at every group size, behind two whole tiles of the widest group, and the last tile is guarded
    for k in R.KS:
        g, t = R.group_cells(ct, k), R.tile_cells(ct, k)
        assert n // t >= 2 and n % t != 0 and (g == 1 or n % g != 0), (k, g)
    assert len({R.group_cells(ct, k) for k in R.KS}) >= 2 and R.group_cells(ct, 1) == 16 // R.NP[ct].itemsize   # more than one group size runs
