"""tests/composite_ref.py, the numpy restatement of ec_composite, held to four things — no GPU:

1. a scalar, cell-by-cell transcription of the rule in include/erased_cells.h (`rule_cell` below: Python loops, numpy scalars);
2. cells worked out by hand: the -0.0 sum, a tie, count < min_count, u64 above 2^53;
3. the oracle's order (eco.value_cmp, impl Ord for CellValue, src/value.rs:248-265) for MIN / MAX;
4. the oracle's Add for SUM: a chain of oracle Adds from a zero f64 buffer over unmasked layers is the rule exactly.
"""
import numpy as np
import pytest

import composite_ref as R
from oracle import eco


def rule_cell(op, ct, cells, valid, min_count):
    """one cell of the header's rule: `cells` the K cells (numpy scalars), `valid` K bools -> (value bits as an int, mask, aux)"""
    dt = R.NP[ct]
    count = sum(1 for v in valid if v)
    ok = count >= min_count
    if R.sums(op):
        acc = np.float64(0.0)
        for c, v in zip(cells, valid):
            if v:
                with np.errstate(over="ignore", invalid="ignore"):
                    acc = acc + np.float64(c)
        with np.errstate(over="ignore", invalid="ignore"):
            r = acc / np.float64(count) if (op == R.MEAN and ok) else acc
        return (int(np.array([r]).view(np.uint64)[0]) if ok else 0), int(ok), count
    picked = None
    for k, (c, v) in enumerate(zip(cells, valid)):
        if not v:
            continue
        if picked is None:
            picked = k
        elif op == R.LAST:
            picked = k
        elif op in (R.MIN, R.MAX):
            order = eco.value_cmp(eco.Value.of(ct, c), eco.Value.of(ct, cells[picked]))   # the oracle's Ord
            if (op == R.MAX and order > 0) or (op == R.MIN and order < 0):
                picked = k
    if not ok:
        return 0, 0, R.NONE
    return int(R.words(np.array([cells[picked]], dt))[0]), 1, picked


def _bits(a):
    return [int(x) for x in R.words(a)]


@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_the_restatement_is_the_scalar_rule_with_the_oracles_order(ct):
    """items 1 and 3: every op, K on both sides of the batch, every mask form, on the head of the GPU inputs (the planted cells and
    palette cells behind them)"""
    n = 40
    for k in (1, 2, 3, 5, 9):
        for form in R.FORMS:
            layers, masks = R.stack(ct, k, n, form)
            valid = R._valid(layers, masks)
            for op in R.OPS:
                for mc in R.min_counts(k):
                    cells, mask, aux = R.composite(op, ct, layers, masks, mc)
                    assert cells.dtype == R.NP[R.result_type(op, ct)] and mask.dtype == aux.dtype == np.uint8
                    for i in range(n):
                        want = rule_cell(op, ct, [a[i] for a in layers], [bool(v[i]) for v in valid], mc)
                        got = (_bits(cells[i:i + 1])[0], int(mask[i]), int(aux[i]))
                        assert got == want, (R.NAMES[ct], R.OP_NAMES[op], k, form, mc, i)


def test_order_key_restates_the_oracles_order():
    for ct in range(R.NT):
        pal = R.palette(ct)
        if ct in R.FLOATS:
            pal = np.concatenate([pal, [R.nan_of(ct), -R.nan_of(ct), np.inf, -np.inf]]).astype(R.NP[ct])
        keys = R.order_key(ct, pal)
        for i, x in enumerate(pal):
            for j, y in enumerate(pal):
                want = eco.value_cmp(eco.Value.of(ct, x), eco.Value.of(ct, y))
                assert int(np.sign(int(keys[i]) - int(keys[j]))) == want, (R.NAMES[ct], x, y)


def _one(op, ct, columns, valid_columns=None, min_count=1):
    """cells given as columns: columns[i] = the K cells of cell i"""
    k = len(columns[0])
    layers = [np.array([c[j] for c in columns], R.NP[ct]) for j in range(k)]
    masks = None if valid_columns is None else [np.array([v[j] for v in valid_columns], np.uint8) for j in range(k)]
    return R.composite(op, ct, layers, masks, min_count)


def test_cells_worked_out_by_hand():
    # the sum of a single -0.0 is 0.0 + -0.0 = +0.0; MIN copies its bits
    cells, mask, aux = _one(R.SUM, R.F64, [[-0.0]])
    assert _bits(cells) == [0] and list(mask) == [1] and list(aux) == [1]
    cells, _, _ = _one(R.MIN, R.F64, [[-0.0]])
    assert _bits(cells) == [1 << 63]
    # -0.0 < +0.0 in the total order, whichever comes first; a NaN is the greatest, -NaN the least
    for col, mn, mx in (([0.0, -0.0], 1, 0), ([-0.0, 0.0], 0, 1)):
        assert list(_one(R.MIN, R.F32, [col])[2]) == [mn] and list(_one(R.MAX, R.F32, [col])[2]) == [mx]
    nan = R.nan_of(R.F64)
    assert list(_one(R.MAX, R.F64, [[1.0, nan, np.inf]])[2]) == [1] and list(_one(R.MIN, R.F64, [[1.0, -nan, -np.inf]])[2]) == [1]
    # a tie: the least k wins, for MIN and MAX; LAST and FIRST by position
    col = [7, 9, 9, 7, 8]
    assert [int(_one(op, R.U16, [col])[2][0]) for op in (R.FIRST, R.LAST, R.MIN, R.MAX)] == [0, 4, 0, 1]
    # masks: the invalid extreme is not seen; count < min_count stores zero bits, mask 0, aux 255 (SUM: the count)
    col, val = [200, 3, 100, 5], [0, 1, 0, 1]
    cells, mask, aux = _one(R.MAX, R.U8, [col], [val])
    assert (int(cells[0]), int(mask[0]), int(aux[0])) == (5, 1, 3)
    cells, mask, aux = _one(R.MAX, R.U8, [col], [val], min_count=3)
    assert (int(cells[0]), int(mask[0]), int(aux[0])) == (0, 0, 255)
    cells, mask, aux = _one(R.SUM, R.U8, [col], [val], min_count=3)
    assert (float(cells[0]), int(mask[0]), int(aux[0])) == (0.0, 0, 2)
    cells, mask, aux = _one(R.MEAN, R.U8, [col], [val], min_count=2)
    assert (float(cells[0]), int(mask[0]), int(aux[0])) == (4.0, 1, 2)
    # u64 above 2^53: double() rounds to even, then each addition rounds: (2^53 + 1 -> 2^53) + 1 -> 2^53, + 3 -> 2^53 + 4
    cells, _, _ = _one(R.SUM, R.U64, [[(1 << 53) + 1, 1, 3]])
    assert float(cells[0]) == float((1 << 53) + 4)
    cells, _, _ = _one(R.SUM, R.U64, [[3, 1, (1 << 53) + 1]])
    assert float(cells[0]) == float((1 << 53) + 4) and float(_one(R.SUM, R.U64, [[1, 1, 1 << 53]])[0][0]) == float((1 << 53) + 2)
    assert float(_one(R.SUM, R.U64, [[1 << 53, 1, 1]])[0][0]) == float(1 << 53)
    # u64 is unsigned: 2^63 is the maximum, not the minimum
    assert list(_one(R.MAX, R.U64, [[5, 1 << 63, 7]])[2]) == [1] and list(_one(R.MIN, R.I64, [[5, -(1 << 63), 7]])[2]) == [1]
    # MEAN of i64 goes through the rounded sum
    assert float(_one(R.MEAN, R.I64, [[(1 << 53) + 1, 1]])[0][0]) == float(1 << 53) / 2.0


@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_sum_is_a_chain_of_the_oracles_adds(ct):
    """item 4: acc = 0.0 (f64); acc = acc + layer_k through the oracle's Add (cv_bin_op!, src/value.rs:199-217: (l as f64) + (r as f64))"""
    n = 257
    for k in (1, 3, 8):
        layers, _ = R.stack(ct, k, n, "none")
        acc = np.zeros(n, np.float64)
        for a in layers:
            acc = eco.f_binop(eco.ADD, acc, a)
        cells, mask, aux = R.composite(R.SUM, ct, layers, None, 1)
        assert R.same_cells(cells, acc).all() and mask.all() and (aux == k).all(), (R.NAMES[ct], k)
        mean, _, _ = R.composite(R.MEAN, ct, layers, None, 1)
        assert R.same_cells(mean, eco.f_binop(eco.DIV, acc, np.full(n, float(k)))).all()
