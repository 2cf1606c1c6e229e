"""tests/composite_rank_ref.py, the numpy statement of ec_composite_rank, held to: a scalar transcription of the header's rule (Python's
`sorted` on (key, k)), numpy.sort along the stack for every position, numpy.median for odd heights, composite_ref's MIN (bits and aux)
and MAX (bits) at num = 0 and num = den, and cells worked out by hand.  No GPU."""
import numpy as np
import pytest

import composite_ref as CR
import composite_rank_ref as R


def scalar_rank(ct, layers, masks, num, den, method, min_count):
    """the header, one cell at a time"""
    k_layers, n = len(layers), layers[0].size
    keys = [R.order_key(ct, a) for a in layers]
    bits = [R.words(a) for a in layers]
    cells, mask, aux = np.zeros(n, bits[0].dtype), np.zeros(n, np.uint8), np.full(n, R.NONE, np.uint8)
    for i in range(n):
        valid = sorted((int(keys[k][i]), k) for k in range(k_layers) if masks is None or masks[k] is None or masks[k][i] != 0)
        c = len(valid)
        if c >= min_count:
            r = (num * (c - 1)) // den if method == R.LOWER else (num * (c - 1) + den - 1) // den
            cells[i], mask[i], aux[i] = bits[valid[r][1]][i], 1, valid[r][1]
    return cells.view(R.NP[ct]), mask, aux


def same(a, b):
    return R.same_cells(a[0], b[0]).all() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_against_the_scalar_transcription(ct):
    n = 61
    for k in (1, 2, 3, 5, 9, 64):
        for form in R.FORMS:
            layers, masks = R.stack(ct, k, n, form, seed=11)
            if ct in R.FLOATS and form == "all":           # NaNs of both signs among the valid cells
                layers[0][7], layers[k - 1][8], masks[0][7], masks[k - 1][8] = CR.nan_of(ct), -CR.nan_of(ct, 0x77), 1, 1
            od = R.ordered(ct, layers, masks)
            for num, den, method in R.TRIPLES:
                for mc in R.min_counts(k):
                    assert same(R.pick(ct, od, num, den, method, mc), scalar_rank(ct, layers, masks, num, den, method, mc)), (k, form, num, den, method, mc)


@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_against_numpy_sort_for_every_position(ct):
    """all valid, no NaNs: position r of numpy's sort along the stack holds the same value (floats: equal as numbers — numpy's sort
    does not order the signed zeros — and of equal keys once both are taken through order_key)"""
    for k in (1, 4, 7, 16, 33):
        layers, _ = R.stack(ct, k, 200, "none", seed=12)
        want = np.sort(np.stack(layers), axis=0)
        for r in range(k):
            den = max(k - 1, 1)
            for method in R.METHODS:                      # r / (k - 1) is exact: both methods keep position r
                cells, mask, aux = R.composite_rank(ct, layers, None, r, den, method, 1)
                assert mask.all() and np.array_equal(cells, want[r]), (k, r)
                assert np.array_equal(np.stack(layers)[aux, np.arange(200)].view(R.words(cells).dtype), R.words(cells))
        assert np.array_equal(R.composite_rank(ct, layers, None, 1, 2, R.LOWER, 1)[0], want[(k - 1) // 2])
        assert np.array_equal(R.composite_rank(ct, layers, None, 1, 2, R.UPPER, 1)[0], want[k // 2])


@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_against_numpy_median_for_odd_heights(ct):
    for k in (1, 3, 5, 9, 63):
        layers, _ = R.stack(ct, k, 300, "none", seed=13)
        want = np.median(np.stack(layers).astype(np.longdouble if R.NP[ct].itemsize == 8 else np.float64), axis=0)
        for method in R.METHODS:
            got = R.composite_rank(ct, layers, None, 1, 2, method, 1)[0]
            assert np.array_equal(got.astype(want.dtype), want), (k, method)


@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_the_ends_are_composite_min_and_max(ct):
    for k in (1, 2, 5, 17):
        for form in R.FORMS:
            layers, masks = R.stack(ct, k, 500, form, seed=14)
            for mc in R.min_counts(k):
                lo, hi = CR.composite(CR.MIN, ct, layers, masks, mc), CR.composite(CR.MAX, ct, layers, masks, mc)
                for method in R.METHODS:
                    assert same(R.composite_rank(ct, layers, masks, 0, 7, method, mc), lo)
                    top = R.composite_rank(ct, layers, masks, 7, 7, method, mc)
                    assert R.same_cells(top[0], hi[0]).all() and np.array_equal(top[1], hi[1])
                    assert (top[2] >= hi[2]).all()        # the GREATEST k among equal keys, where MAX reports the least
    layers = [np.array([5, 5, 5], R.NP[ct])] * 3
    assert R.composite_rank(ct, layers, None, 1, 1, R.LOWER, 1)[2].tolist() == [2, 2, 2]
    assert CR.composite(CR.MAX, ct, layers, None, 1)[2].tolist() == [0, 0, 0]


def cell(ct, values, valid, num, den, method, min_count=1):
    """one hand-made cell -> (bits as an int, mask byte, aux byte)"""
    layers = [np.array([v], R.NP[ct]) if not isinstance(v, np.ndarray) else v for v in values]
    masks = [np.array([m], np.uint8) for m in valid]
    c, m, a = R.composite_rank(ct, layers, masks, num, den, method, min_count)
    return int(R.words(c)[0]), int(m[0]), int(a[0])


def bits(ct, v):
    return int(R.words(np.array([v], R.NP[ct]))[0])


def test_cells_worked_out_by_hand():
    U8, I8, F32 = CR.U8, CR.I8, CR.F32
    # an even count: 4 valid of 5, sorted 10(k0) 20(k3) 30(k1) 40(k4); the invalid 0 (k2) takes no part
    v, ok = [10, 30, 0, 20, 40], [1, 1, 0, 1, 1]
    assert cell(U8, v, ok, 1, 2, R.LOWER) == (20, 1, 3)      # r = 3 // 2 = 1
    assert cell(U8, v, ok, 1, 2, R.UPPER) == (30, 1, 1)      # r = (3 + 1) // 2 = 2
    assert cell(U8, v, ok, 1, 4, R.LOWER) == (10, 1, 0)      # r = 3 // 4 = 0
    assert cell(U8, v, ok, 1, 4, R.UPPER) == (20, 1, 3)      # r = (3 + 3) // 4 = 1
    assert cell(U8, v, ok, 9, 10, R.LOWER) == (30, 1, 1)     # r = 27 // 10 = 2
    assert cell(U8, v, ok, 9, 10, R.UPPER) == (40, 1, 4)     # r = 36 // 10 = 3
    assert cell(U8, v, ok, 0, 1, R.UPPER) == (10, 1, 0) and cell(U8, v, ok, 1, 1, R.LOWER) == (40, 1, 4)
    # ties across layers: 7 7 7 9, equal keys in layer order
    v, ok = [7, 9, 7, 7], [1, 1, 1, 1]
    assert [cell(U8, v, ok, r, 3, R.LOWER)[2] for r in range(4)] == [0, 2, 3, 1]
    assert cell(U8, v, ok, 1, 2, R.LOWER) == (7, 1, 2) and cell(U8, v, ok, 1, 2, R.UPPER) == (7, 1, 3)
    # -0.0 against +0.0: the total order puts -0.0 first, whatever the layers' order
    v, ok = [0.0, -0.0], [1, 1]
    assert cell(F32, v, ok, 0, 1, R.LOWER) == (0x80000000, 1, 1) and cell(F32, v, ok, 1, 1, R.LOWER) == (0, 1, 0)
    assert cell(F32, v, ok, 1, 2, R.LOWER) == (0x80000000, 1, 1) and cell(F32, v, ok, 1, 2, R.UPPER) == (0, 1, 0)
    # both NaN signs: the negative NaN is the least cell, the positive one the greatest, payloads come through
    pos, neg = CR.nan_of(F32, 0x1234), np.array([0xffc00077], np.uint32).view(np.float32)[0]
    v, ok = [pos, 1.0, neg, -np.inf, np.inf], [1, 1, 1, 1, 1]
    assert [cell(F32, v, ok, r, 4, R.LOWER)[2] for r in range(5)] == [2, 3, 1, 4, 0]
    assert cell(F32, v, ok, 0, 1, R.LOWER)[0] == 0xffc00077 and cell(F32, v, ok, 1, 1, R.LOWER)[0] == 0x7fc01234
    assert cell(F32, v, ok, 1, 2, R.LOWER) == (bits(F32, 1.0), 1, 1)
    for ct, ones in ((CR.F32, 0x7fffffff), (CR.F64, 0x7fffffffffffffff)):      # the all-ones positive NaN: no key is greater
        top = np.array([ones], R.words(np.zeros(1, R.NP[ct])).dtype).view(R.NP[ct])
        assert cell(ct, [top, 3.0, top], [1, 1, 1], 1, 1, R.LOWER) == (ones, 1, 2)
        assert cell(ct, [top, 3.0, top], [1, 1, 0], 1, 2, R.UPPER) == (ones, 1, 0)
    # the u64 maximum is the greatest cell and 2^63 lies above 2^63 - 1 (no signed reading)
    big = 2 ** 64 - 1
    v, ok = [big, 2 ** 63, 2 ** 63 - 1, 0, big], [1, 1, 1, 1, 1]
    assert [cell(CR.U64, v, ok, r, 4, R.LOWER)[:3:2] for r in range(5)] == [(0, 3), (2 ** 63 - 1, 2), (2 ** 63, 1), (big, 0), (big, 4)]
    # i8 -128 is the least cell; 127 the greatest; as bits 0x80 and 0x7f
    v, ok = [127, -128, 0, -1], [1, 1, 1, 1]
    assert [cell(I8, v, ok, r, 3, R.LOWER)[:3:2] for r in range(4)] == [(0x80, 1), (0xff, 3), (0, 2), (0x7f, 0)]
    assert cell(CR.I16, [32767, -32768, -1], [1, 1, 1], 1, 2, R.LOWER) == (0xffff, 1, 2)
    # a NaN under a cleared mask byte does not reach the result
    v, ok = [CR.nan_of(F32), 2.0, 1.0, -CR.nan_of(F32)], [0, 1, 1, 0]
    assert cell(F32, v, ok, 1, 1, R.LOWER) == (bits(F32, 2.0), 1, 1) and cell(F32, v, ok, 0, 1, R.LOWER) == (bits(F32, 1.0), 1, 2)
    # count < min_count: zero bits, mask 0, aux 255 — and at count == min_count the cell is back
    v, ok = [5, 6, 7], [1, 0, 1]
    assert cell(U8, v, ok, 1, 2, R.UPPER, min_count=3) == (0, 0, 255) and cell(U8, v, ok, 1, 2, R.UPPER, min_count=2) == (7, 1, 2)
    assert cell(U8, v, [0, 0, 0], 1, 2, R.LOWER) == (0, 0, 255)


def test_lower_and_upper_agree_at_odd_counts_and_bracket_the_rest():
    for ct in (CR.U16, CR.F64):
        layers, masks = R.stack(ct, 9, 2000, "all", seed=15)
        od = R.ordered(ct, layers, masks)
        lo, hi = R.pick(ct, od, 1, 2, R.LOWER, 1), R.pick(ct, od, 1, 2, R.UPPER, 1)
        odd = od[1] % 2 == 1
        assert odd.any() and (~odd & (od[1] > 0)).any()
        assert R.same_cells(lo[0], hi[0])[odd].all() and np.array_equal(lo[2][odd], hi[2][odd])
        even = ~odd & (od[1] > 0)
        assert (lo[2][even] != hi[2][even]).all() and (R.order_key(ct, lo[0]) <= R.order_key(ct, hi[0])).all()


def test_the_position_formula():
    for num, den, method in R.TRIPLES:
        for c in range(1, 65):
            r = R.position(num, den, method, c)
            assert 0 <= r <= c - 1 and den * r <= num * (c - 1) + (den - 1 if method == R.UPPER else 0)
            if method == R.LOWER:
                assert den * r <= num * (c - 1) < den * (r + 1)
            else:
                assert den * (r - 1) < num * (c - 1) <= den * r
