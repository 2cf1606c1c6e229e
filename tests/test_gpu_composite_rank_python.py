"""ec.composite_rank and ec.composite_median, the public functions: plain, masked and mixed stacks, `aux=True`, the return types, the
empty stack and what Python refuses itself — against tests/composite_rank_ref.py, bit for bit."""
import numpy as np
import pytest

import composite_ref as CR
import composite_rank_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def test_plain_masked_and_mixed_stacks(ec):
    n, ct = 1000, CR.I16
    layers, masks = R.stack(ct, 5, n, "all", seed=6)
    plain = [ec.CellBuffer.from_vec(a) for a in layers]
    out = ec.composite_rank(plain)
    assert isinstance(out, ec.CellBuffer) and out.cell_type() == ec.Int16
    assert np.array_equal(out.to_numpy(), R.composite_rank(ct, layers, None, 1, 2, R.LOWER, 1)[0])
    assert np.array_equal(out.to_numpy(), np.sort(np.stack(layers), axis=0)[2])            # five layers, all valid: the median
    out, aux = ec.composite_rank(plain, q=(9, 10), method="upper", aux=True)
    assert isinstance(out, ec.CellBuffer) and isinstance(aux, ec.CellBuffer) and aux.cell_type() == ec.UInt8
    wc, _, wa = R.composite_rank(ct, layers, None, 9, 10, R.UPPER, 1)
    assert np.array_equal(out.to_numpy(), wc) and np.array_equal(aux.to_numpy(), wa)
    assert np.array_equal(np.stack(layers)[aux.to_numpy(), np.arange(n)], wc)               # aux names the layer the cell came from
    masked = [ec.MaskedCellBuffer(b, ec.Mask.new(m)) for b, m in zip(plain, masks)]
    for q, method, mc in (((1, 2), "lower", 1), ((1, 2), "upper", 3), ((1, 4), "lower", 5), (0, "lower", 2), (1, "upper", 1)):
        out, aux = ec.composite_rank(masked, q, method, min_count=mc, aux=True)
        assert isinstance(out, ec.MaskedCellBuffer) and isinstance(aux, ec.CellBuffer)
        num, den = (q, 1) if isinstance(q, int) else q
        wc, wm, wa = R.composite_rank(ct, layers, masks, num, den, R.METHOD_NAMES.index(method), mc)
        assert R.same_cells(out.buffer().to_numpy(), wc).all() and np.array_equal(out.mask().to_numpy(), wm) and np.array_equal(aux.to_numpy(), wa)
    mixed = [plain[0], masked[1], plain[2]]
    m3 = [None, masks[1], None]
    out = ec.composite_rank(mixed, min_count=3)
    assert isinstance(out, ec.MaskedCellBuffer)
    wc, wm, _ = R.composite_rank(ct, layers[:3], m3, 1, 2, R.LOWER, 3)
    assert R.same_cells(out.buffer().to_numpy(), wc).all() and np.array_equal(out.mask().to_numpy(), wm)


@pytest.mark.parametrize("ct", (CR.U8, CR.F32, CR.F64, CR.U64), ids=lambda t: CR.NAMES[t])
def test_the_median_functions(ec, ct):
    n = 777
    layers, masks = R.stack(ct, 8, n, "some", seed=8)
    stack = [ec.CellBuffer.from_vec(a) if m is None else ec.MaskedCellBuffer(ec.CellBuffer.from_vec(a), ec.Mask.new(m)) for a, m in zip(layers, masks)]
    lo, hi = ec.composite_median(stack), ec.composite_median(stack, method="upper")
    wl, wh = R.composite_rank(ct, layers, masks, 1, 2, R.LOWER, 1), R.composite_rank(ct, layers, masks, 1, 2, R.UPPER, 1)
    assert R.same_cells(lo.buffer().to_numpy(), wl[0]).all() and R.same_cells(hi.buffer().to_numpy(), wh[0]).all()
    assert np.array_equal(lo.mask().to_numpy(), wl[1]) and np.array_equal(hi.mask().to_numpy(), wh[1])
    res, aux = ec.composite_median(stack, "upper", min_count=4, aux=True)
    want = R.composite_rank(ct, layers, masks, 1, 2, R.UPPER, 4)
    assert R.same_cells(res.buffer().to_numpy(), want[0]).all() and np.array_equal(res.mask().to_numpy(), want[1]) and np.array_equal(aux.to_numpy(), want[2])
    # the ends are composite's min and max (the bits; the aux of the minimum too)
    low, low_aux = ec.composite_rank(stack, 0, aux=True)
    cmin, cmin_aux = ec.composite(stack, "min", aux=True)
    assert R.same_cells(low.buffer().to_numpy(), cmin.buffer().to_numpy()).all() and np.array_equal(low_aux.to_numpy(), cmin_aux.to_numpy())
    assert R.same_cells(ec.composite_rank(stack, 1).buffer().to_numpy(), ec.composite(stack, "max").buffer().to_numpy()).all()


def test_the_empty_stack_and_what_python_refuses(ec):
    n, ct = 100, CR.I16
    layers, masks = R.stack(ct, 3, n, "all", seed=9)
    plain = [ec.CellBuffer.from_vec(a) for a in layers]
    empty = ec.composite_rank([ec.CellBuffer.from_vec(np.zeros(0, np.int16))] * 2, aux=True)
    assert empty[0].len() == 0 and empty[0].cell_type() == ec.Int16 and empty[1].len() == 0
    for bad, text in (([], "layers"), (plain * 22, "EC_COMPOSITE_MAX_LAYERS"), ([plain[0], ec.CellBuffer.from_vec(layers[0].astype(np.int32))], "cell type"),
                      ([plain[0], ec.CellBuffer.from_vec(layers[0][:5])], "cells"), ([plain[0], masks[0]], "not a CellBuffer")):
        with pytest.raises(ec.EcError, match=text):
            ec.composite_rank(bad)
    for mc in (0, 4, True, 1.0):
        with pytest.raises(ec.EcError, match="min_count"):
            ec.composite_rank(plain, min_count=mc)
    for q in (0.5, (2, 1), (1, 0), (1, 65536), "1/2"):
        with pytest.raises(ec.EcError, match="q "):
            ec.composite_rank(plain, q)
    for method in ("median", 2, None):
        with pytest.raises(ec.EcError, match="method"):
            ec.composite_rank(plain, (1, 2), method)
    with pytest.raises(ec.EcError, match="operation"):
        ec.composite(plain, "median")                    # ec.composite stays as it was
