"""The inputs of tests/test_gpu_composite.py can tell a right composite kernel from a wrong one — checked here without a GPU.

For each mistake a kernel of this family can make, `composite_ref` holds a numpy model of the kernel that makes it
(`composite_faulty`).  For every cell type and every op the mistake can touch, the main GPU cases (`stack(ct, k, main_len(ct), form)`
over `KS`, `FORMS` and `min_counts(k)`) must contain a launch with a cell where the wrong kernel's value, mask byte or aux byte
differs from the right one.  An input set that passed a faulty model would show nothing on the GPU either.

The inputs hold, planted and asserted below: cells with no valid layer, cells whose only valid layer is the last, cells where an
invalid layer holds the extreme, ties of identical bits between valid layers, for floats -0.0 and +0.0 valid in one cell, and for
f32, f64, i64 and u64 magnitudes for which the sum's order changes its bits.  For cell types of 32 bits or fewer the sum of 64 cells
is exact in f64, so the order cannot matter there (composite_ref's docstring has the arithmetic).
"""
import numpy as np
import pytest

import composite_ref as R

ORDER_SENSITIVE = (R.F32, R.F64, R.I64, R.U64)


def _differs(a, b):
    return any(not R.same_cells(x, y, nan_by_class=True).all() for x, y in zip(a, b))


def _launches(ct):
    """the main GPU cases of one cell type, short stacks first"""
    n = R.main_len(ct)
    for k in R.KS:
        for form in R.FORMS:
            yield k, form, n


@pytest.mark.parametrize("kind", R.FAULTS)
def test_every_fault_changes_an_answer_for_every_type_and_op_it_can_touch(kind):
    seen = 0
    for ct in range(R.NT):
        for op in R.OPS:
            exposed = applicable = False
            for k, form, n in _launches(ct):
                for mc in R.min_counts(k):
                    if not R.applies(kind, op, ct, k, form, mc):
                        continue
                    applicable = True
                    layers, masks = R.stack(ct, k, n, form)
                    good = R.composite(op, ct, layers, masks, mc)
                    args = [j for j, m in enumerate(masks) if m is not None] if kind == "mask_ignored" else [None]
                    # a mask that is ignored must show whichever layer's it is
                    exposed = all(_differs(R.composite_faulty(kind, op, ct, layers, masks, mc, arg), good) for arg in args)
                    if exposed:
                        break
                if exposed:
                    break
            assert exposed or not applicable, (kind, R.NAMES[ct], R.OP_NAMES[op])
            seen += exposed
    assert seen, kind


def test_what_each_fault_can_touch():
    """the table `applies` is not empty-handed: each mistake reaches the ops and types it is about"""
    reach = {kind: {(op, ct) for ct in range(R.NT) for op in R.OPS for k in R.KS for form in R.FORMS for mc in R.min_counts(k)
                    if R.applies(kind, op, ct, k, form, mc)} for kind in R.FAULTS}
    every = {(op, ct) for ct in range(R.NT) for op in R.OPS}
    for kind in ("mask_ignored", "null_mask_takes_neighbour", "count_gt", "invalid_not_zeroed", "tail_layers_skipped_2", "tail_layers_skipped_4",
                 "tail_layers_skipped_8", "tail_without_masks"):
        assert reach[kind] == every, kind
    assert reach["first_picks_last"] == {(R.FIRST, ct) for ct in range(R.NT)}
    assert reach["tie_to_higher"] == {(op, ct) for ct in range(R.NT) for op in (R.MIN, R.MAX)}
    assert reach["ieee_less"] == reach["raw_float_bits"] == {(op, ct) for ct in R.FLOATS for op in (R.MIN, R.MAX)}
    assert reach["u64_signed"] == {(R.MIN, R.U64), (R.MAX, R.U64)}
    assert reach["sum_descending"] == {(op, ct) for ct in ORDER_SENSITIVE for op in (R.SUM, R.MEAN)}
    assert reach["sum_in_f32"] == {(op, ct) for ct in range(R.NT) if R.NP[ct].itemsize >= 4 for op in (R.SUM, R.MEAN)}
    assert reach["int64_truncated"] == {(op, ct) for ct in (R.I64, R.U64) for op in (R.SUM, R.MEAN)}
    assert reach["sum_adds_invalid"] == {(op, ct) for ct in range(R.NT) for op in (R.SUM, R.MEAN)}
    assert reach["mean_divides_by_k"] == {(R.MEAN, ct) for ct in range(R.NT)}
    assert reach["invalid_aux_not_255"] == reach["aux_index_in_batch"] == {(op, ct) for ct in range(R.NT) for op in (R.FIRST, R.LAST, R.MIN, R.MAX)}


@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_the_planted_cells_are_there(ct):
    n = R.main_len(ct)
    for k in (3, 5, 64):
        layers, masks = R.stack(ct, k, n, "all")
        v, m = np.stack(layers), np.stack(masks)
        key = np.stack([R.order_key(ct, a) for a in layers])
        p = R.planted(ct, k)[0].shape[1]
        tail = n - n % 16                                      # the planted cells of the tail lie behind the last 16-cell group
        assert n - p >= tail - 4, "the planted tail cells reach into the ragged tail"
        for base in (0, n - p):
            at = lambda i: base + i
            count = m.sum(axis=0)
            assert count[at(0)] == 0                                                        # no valid layer
            assert count[at(1)] == 1 and m[k - 1, at(1)] == 1                               # only the last
            for cell, best in ((at(2), key[:, at(2)].argmax()), (at(3), key[:, at(3)].argmin())):
                assert m[best, cell] == 0 and count[cell] > 0                              # an invalid layer holds the extreme
                valid_keys = key[m[:, cell] != 0, cell]
                assert (valid_keys < key[best, cell]).all() or (valid_keys > key[best, cell]).all()
            for cell, pick in ((at(4), np.max), (at(5), np.min)):                           # ties of identical bits between valid layers
                valid = m[:, cell] != 0
                ext = pick(key[valid, cell])
                tied = np.flatnonzero(valid & (key[:, cell] == ext))
                assert tied.size >= 2 and len({int(R.words(v[j:j + 1, cell])[0]) for j in tied}) == 1
            if ct in R.FLOATS:
                for cell in (at(6), at(7)):
                    bits = {int(R.words(v[j:j + 1, cell])[0]) for j in range(k) if m[j, cell]}
                    assert {0, 1 << (8 * R.NP[ct].itemsize - 1)} <= bits                    # -0.0 and +0.0 valid in one cell
                assert (np.isnan(v) & (m == 0)).any()                                       # a NaN under a cleared mask byte
                valid_nan = np.isnan(v) & (m != 0)
                assert not valid_nan.any()
            if ct in ORDER_SENSITIVE:
                col, val = [a[at(8):at(8) + 1] for a in layers], [mk[at(8):at(8) + 1] for mk in masks]
                up = R.composite(R.SUM, ct, col, val, 1)[0]
                down = R.composite_faulty("sum_descending", R.SUM, ct, col, val, 1)[0]
                assert not R.same_cells(up, down).all()                                     # the sum's order changes its bits
            else:                                                                           # and cannot, where 64 cells sum exactly
                assert 64 * 2 ** (8 * R.NP[ct].itemsize) < 2 ** 53
    # the tail is ragged at every CPL, behind two whole tiles of every op, and the last tile is guarded
    for op in R.OPS:
        c, t = R.cpl(op, ct), R.tile_cells(op, ct)
        assert n % c != 0 and n // t >= 2 and 0 < (n // c) % (t // c)


def test_the_stack_heights_lie_on_both_sides_of_every_batch_size():
    for b in (2, 4, 8, 16):
        assert {b - 1, b, b + 1} & set(R.KS) >= {b, b + 1} and any(k % b for k in R.KS) and any(k % b == 0 for k in R.KS)
    assert max(R.KS) == R.MAX_LAYERS and 1 in R.KS and R.MAX_LAYERS - 1 in R.KS
