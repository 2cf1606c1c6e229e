"""The inputs of tests/test_gpu_reclass.py expose the mistakes a reclass kernel, or the table it reads, can make: for each
modelled mistake (tests/reclass_ref.py) and every cell type it applies to, the cells that file classifies contain one where the
faulty model differs from the right answer.  The order mistakes are models of the predicate; the kernel mistakes are models of a
kernel reading the record the library's own builder wrote (host only: no device is needed).  A GPU test that passes on inputs
which could not tell a faulty kernel from a right one would show nothing."""
import numpy as np
import pytest

import reclass_ref as Q
from test_gpu_reclass import CROSS, bits, class_values, every_type_cases, some_valid


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    return ec


@pytest.mark.parametrize("kind", Q.ORDER_FAULTS)
def test_the_inputs_expose_a_mistake_in_the_order(kind):
    seen = set()
    for t in range(Q.NT):
        for bt, breaks, x, _ in every_type_cases(t):
            if not Q.applies(kind, t, bt):
                continue
            for right in (False, True):
                if kind == "right_ignored" and not right:
                    continue
                right_answer, faulty = Q.classes(t, x, bt, breaks, right), Q.classes_faulty(kind, t, x, bt, breaks, right)
                differ = int(np.count_nonzero(right_answer != faulty))
                if kind == "right_ignored":   # only ties tell: at least 20 cells equal to a break wherever t holds one of them
                    ties = int(np.count_nonzero(Q.classes(t, x, bt, breaks, False) != Q.classes(t, x, bt, breaks, True)))
                    with np.errstate(all="ignore"):
                        holds_one = np.any(Q.R.cmp3(t, np.asarray(breaks, Q.NP[bt]).astype(Q.NP[t]), bt, breaks) == 0)
                    assert ties >= 20 or not holds_one, (Q.NAMES[t], Q.NAMES[bt], ties)
                if differ:
                    seen.add(t)
    want = {t for t in range(Q.NT) if any(Q.applies(kind, t, bt) for bt in (t, Q.F64, CROSS[t]))}
    assert seen == want, (kind, "not exposed for", [Q.NAMES[t] for t in want - seen])


@pytest.mark.parametrize("kind", Q.TABLE_FAULTS)
def test_the_inputs_expose_a_mistake_in_the_kernel(ec, kind):
    seen, want = set(), set()
    for t in range(Q.NT):
        for k, (bt, breaks, x, mask) in enumerate(every_type_cases(t)):
            dt = Q.I16 if kind == "value_slot_at_the_wrong_width" else Q.U8
            if not Q.applies(kind, t, bt, dt):
                continue
            if kind == "searches_n_breaks_not_n_reached" and (Q.size_of(t) > 2 or bt == t):
                continue   # it shows where a break is out of the raster type's reach: the narrow types against wider breaks
            want.add(t)
            values, nodata = class_values(dt, len(breaks) + 1, k)
            valid = some_valid(len(breaks) + 1, k)
            table = ec.ReclassTable(t, breaks, values, right=bool(k % 2), valid=valid, nodata=nodata)
            tab = Q.parse(table.bytes())
            good, good_ok = Q.kernel_model(None, tab, t, x, mask, dt)
            ref, ref_ok = Q.reclass(t, x, mask, bt, breaks, bool(k % 2), dt, values, valid, nodata)
            assert np.array_equal(bits(good), bits(ref)) and np.array_equal(good_ok, ref_ok), "the model without a mistake is the reference"
            bad, bad_ok = Q.kernel_model(kind, tab, t, x, mask, dt)
            if not (np.array_equal(bits(bad), bits(ref)) and np.array_equal(bad_ok, ref_ok)):
                seen.add(t)
    assert want and seen == want, (kind, "not exposed for", [Q.NAMES[t] for t in want - seen])
