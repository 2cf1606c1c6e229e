"""Would the GPU tests of ec_focal / ec_focal_convolve notice a wrong kernel?  Each mistake a tiled moving-window kernel can make is
modelled here in numpy (`model`, the rule with one switch thrown) and run over the inputs, shapes and radii that
tests/test_gpu_focal.py runs (tests/focal_cases.py): for every model at least one of them must give an answer that differs from
tests/focal_ref.py, bit for bit as the GPU file compares — otherwise that file is blind to the fault.  A store that never happens is
the exception: it shows only in the pre-filled arenas of tests/test_gpu_focal_bounds.py, so those two models run over that file's kinds
and shapes.  No GPU."""
import numpy as np
import pytest

import focal_cases as K
import focal_ref as R

WHOLE, NORMALIZE = 1, 2


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(K.UINT[a.dtype.itemsize])


def differs(got, exp, by_class=False):
    (g, gv), (e, ev) = got, exp
    same = bits(g) == bits(e)
    if by_class:
        same |= np.isnan(g) & np.isnan(e)
    return not (same.all() and np.array_equal(gv, ev))


def model(what, a, mask, rx, ry, flags=0, w=None, fault=None):
    """the rule cell by cell in index arrays, with `fault` thrown; what: an operation number or "convolve" """
    rows, cols = a.shape
    n = rows * cols
    if fault == "radii-swapped":
        rx, ry = ry, rx
    nx, ny = 2 * rx + 1, 2 * ry + 1
    if w is not None:
        if fault == "weights-transposed":
            w = w.T
        elif fault == "weights-flipped":
            w = w[::-1, ::-1]
        assert w.shape == (ny, nx), (w.shape, fault)
    I, J = np.mgrid[0:rows, 0:cols]
    x0, y0 = (J // K.TW) * K.TW, (I // K.TH) * K.TH          # the output cell's tile
    flat_a = a.ravel()
    flat_m = None if mask is None else mask.ravel()
    if fault == "mask-off-by-one" and flat_m is not None:
        flat_m = np.roll(flat_m, 1)
    sums = what == "convolve" or what in (R.SUM, R.MEAN)
    acc = np.zeros((rows, cols))
    wsum = np.zeros((rows, cols))
    count = np.zeros((rows, cols), dtype=np.int64)
    keys = None
    if not sums:
        if fault == "order-raw-bits":
            keys = bits(a).astype(np.uint64).ravel()
        elif fault == "order-less-than":
            keys = flat_a   # compared with < and >: a NaN never wins, -0.0 and +0.0 tie
        else:
            keys = R.order_keys(a).ravel()
    best = np.zeros((rows, cols), dtype=np.int64)      # index of the winning cell
    have = np.zeros((rows, cols), dtype=bool)
    outer, inner = (range(nx), range(ny)) if fault == "column-major" else (range(ny), range(nx))
    with np.errstate(all="ignore"):
        for o in outer:
            racc, rw = np.zeros((rows, cols)), np.zeros((rows, cols))
            for i in inner:
                dy, dx = (i, o) if fault == "column-major" else (o, i)
                y, x = I - ry + dy, J - rx + dx
                if fault == "wrap":
                    at = y * cols + x
                    inside = (at >= 0) & (at < n)
                else:
                    inside = (y >= 0) & (y < rows) & (x >= 0) & (x < cols)
                    at = np.where(inside, y * cols + x, 0)
                at = np.where(inside, at, 0)
                if fault == "halo-left":
                    inside &= ~(x == x0 - rx) | (rx == 0)
                elif fault == "halo-right":
                    inside &= ~(x == x0 + K.TW - 1 + rx) | (rx == 0)
                elif fault == "halo-top":
                    inside &= ~(y == y0 - ry) | (ry == 0)
                elif fault == "halo-bottom":
                    inside &= ~(y == y0 + K.TH - 1 + ry) | (ry == 0)
                on = inside if flat_m is None else inside & (flat_m[at] != 0)
                tap = on
                counted = inside if fault == "masked-counted" else on
                if sums:
                    v = flat_a[at].astype(np.float64)
                    if what == "convolve":
                        term = w[dy, dx] * v
                        wt = np.full((rows, cols), w[dy, dx])
                    else:
                        term, wt = v, np.zeros((rows, cols))
                    if fault == "masked-times-zero":   # the cell is multiplied by its mask byte and added anyway
                        term = np.where(on, term, term * 0.0)
                        tap = inside
                        wt = np.where(on, wt, 0.0)
                    if fault == "no-racc":
                        acc = np.where(tap, acc + term, acc)
                        wsum = np.where(tap, wsum + wt, wsum)
                    else:
                        racc = np.where(tap, racc + term, racc)
                        rw = np.where(tap, rw + wt, rw)
                else:
                    k = keys[at]
                    if what == R.MIN:
                        better = k < keys[best]
                    else:
                        better = k > keys[best]
                    take = tap & (~have | better)
                    best = np.where(take, at, best)
                    have |= tap
                count += counted
            if fault != "no-racc":
                acc = acc + racc
                wsum = wsum + rw
        full = nx * ny
        if fault == "whole-ignores-edges":
            xs = np.minimum(J + rx, cols - 1) - np.maximum(J - rx, 0) + 1
            ys = np.minimum(I + ry, rows - 1) - np.maximum(I - ry, 0) + 1
            full = xs * ys
        whole = bool(flags & WHOLE)
        if fault == "whole-ignores-holes" and whole:
            inside_count = (np.minimum(J + rx, cols - 1) - np.maximum(J - rx, 0) + 1) * (np.minimum(I + ry, rows - 1) - np.maximum(I - ry, 0) + 1)
            valid = inside_count == full
        else:
            valid = (count == full) if whole else (count > 0)
        if what == "convolve":
            r = acc
            if flags & NORMALIZE:
                den = np.full((rows, cols), w.sum()) if fault == "normalize-by-all-weights" else wsum
                valid = valid & (den != 0.0)
                r = acc / den
        elif what == R.SUM:
            r = acc
        elif what == R.MEAN:
            r = acc / (np.float64(nx * ny) if fault == "mean-by-full-footprint" else count.astype(np.float64))
        else:
            r = flat_a[best]
    out = np.zeros((rows, cols), dtype=np.float64 if sums else a.dtype)
    out[valid] = r[valid]
    vm = valid.astype(np.uint8)
    if fault == "last-column-skipped":      # never written: the arena's complement of the expected bytes stays (tests/arena.py)
        skip = J % K.TW == K.TW - 1
        out[skip] = (~bits(out))[skip].view(out.dtype)
        vm[skip] ^= 0xff
    elif fault == "last-row-skipped":
        skip = I % K.TH == K.TH - 1
        out[skip] = (~bits(out))[skip].view(out.dtype)
        vm[skip] ^= 0xff
    return out, vm


def gpu_cases(types, raw=False):
    """(ct, a, mask, radius, what, flags) as test_gpu_focal.sweep and its sources run them, smallest rasters first"""
    import test_gpu_focal as G
    for radius in K.RADII:
        for cols, rows in sorted(K.shapes(*radius), key=lambda s: s[0] * s[1]):
            for ct in types:
                for masked in (False, True):
                    a, m = G.source(ct, cols, rows, masked, raw)
                    for what, flags in G.FOCAL_CALLS + [("convolve", f) for f in G.CONV_FLAGS]:
                        yield ct, a, m, radius, what, flags


def reference(a, m, radius, what, flags):
    if what == "convolve":
        return R.convolve(a, m, K.weights(*radius), bool(flags & NORMALIZE), bool(flags & WHOLE))
    return R.focal(what, a, m, radius[0], radius[1], bool(flags & WHOLE))


def first_exposure(fault, types, raw=False, want=None, limit=600):
    tried = 0
    for ct, a, m, radius, what, flags in gpu_cases(types, raw):
        if want is not None and not want(ct, a, m, radius, what, flags):
            continue
        tried += 1
        if tried > limit:
            break
        w = K.weights(*radius) if what == "convolve" else None
        got = model(what, a, m, radius[0], radius[1], flags, w, fault)
        by_class = raw and what not in (R.MIN, R.MAX)
        if differs(got, reference(a, m, radius, what, flags), by_class):
            return ct, a.shape, radius, what, flags, m is not None
    return None


def test_the_model_without_a_fault_is_the_rule():
    tried = 0
    for ct, a, m, radius, what, flags in gpu_cases((1, 9)):
        if a.size > 700 or radius == (7, 7):
            continue
        w = K.weights(*radius) if what == "convolve" else None
        assert not differs(model(what, a, m, radius[0], radius[1], flags, w), reference(a, m, radius, what, flags)), (ct, a.shape, radius, what, flags)
        tried += 1
    assert tried > 300


SUMS = lambda ct, a, m, radius, what, flags: what == "convolve" or what in (R.SUM, R.MEAN)
FAULTS = {
    # fault: (cell types tried, which of the GPU file's cases can show it)
    "halo-left": ((0, 9), lambda ct, a, m, r, what, f: a.shape[1] > K.TW and r[0] > 0),
    "halo-right": ((0, 9), lambda ct, a, m, r, what, f: a.shape[1] > K.TW and r[0] > 0),
    "halo-top": ((0, 9), lambda ct, a, m, r, what, f: a.shape[0] > K.TH and r[1] > 0),
    "halo-bottom": ((0, 9), lambda ct, a, m, r, what, f: a.shape[0] > K.TH and r[1] > 0),
    "wrap": ((0, 5), lambda ct, a, m, r, what, f: r[0] > 0 and a.shape[0] > 1),
    "radii-swapped": ((1,), lambda ct, a, m, r, what, f: r[0] != r[1] and what != "convolve"),
    "column-major": ((8, 9), SUMS),
    "no-racc": ((8, 9), SUMS),
    "masked-counted": ((2,), lambda ct, a, m, r, what, f: m is not None),
    "mean-by-full-footprint": ((0,), lambda ct, a, m, r, what, f: what == R.MEAN and r != (0, 0)),
    "whole-ignores-edges": ((0,), lambda ct, a, m, r, what, f: bool(f & WHOLE) and m is None and r != (0, 0)),
    "whole-ignores-holes": ((0,), lambda ct, a, m, r, what, f: bool(f & WHOLE) and m is not None),
    "weights-transposed": ((4,), lambda ct, a, m, r, what, f: what == "convolve" and r[0] == r[1] and r[0] > 0),
    "weights-flipped": ((4,), lambda ct, a, m, r, what, f: what == "convolve" and r != (0, 0)),
    "normalize-by-all-weights": ((6,), lambda ct, a, m, r, what, f: what == "convolve" and bool(f & NORMALIZE) and r != (0, 0)),
    "mask-off-by-one": ((3,), lambda ct, a, m, r, what, f: m is not None),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_the_gpu_inputs_expose(fault):
    types, want = FAULTS[fault]
    assert first_exposure(fault, types, want=want) is not None, fault


def arena_cases():
    """(kind id, a, mask, radius, what, flags) as tests/test_gpu_focal_bounds.py runs them: its kinds, its shapes, its seeds"""
    import test_gpu_focal_bounds as B
    for kind, name in zip(B.KINDS, B.KIND_IDS):
        ct, what, flags, masked, _, radius = kind
        for k, (cols, rows) in enumerate(B.SHAPES):
            a = K.raster_cells(ct, cols, rows, 0xB0 + ct + k)
            m = K.mask_bytes("hashed", cols, rows, 0xB1 + k) if masked else None
            yield name, a, m, radius, what, flags


@pytest.mark.parametrize("fault", ["last-column-skipped", "last-row-skipped"])
def test_a_skipped_store_shows_in_the_arenas(fault):
    """A store that never happens shows only where the output was pre-filled with something else: the arenas of
    tests/test_gpu_focal_bounds.py hold the complement of the expected bytes (test_gpu_focal.py writes into fresh blocks that may
    still hold an earlier right answer).  Every kind of that file has a shape in which the tile's last column and last row exist."""
    seen = set()
    for name, a, m, radius, what, flags in arena_cases():
        w = K.weights(*radius) if what == "convolve" else None
        if differs(model(what, a, m, radius[0], radius[1], flags, w, fault), reference(a, m, radius, what, flags)):
            seen.add(name)
    import test_gpu_focal_bounds as B
    assert seen == set(B.KIND_IDS), (fault, sorted(set(B.KIND_IDS) - seen))


def test_every_separate_halo_fault_shows_in_every_kind():
    """a halo that is not loaded must show for the sums, for min / max and for the convolution alike: three kernels stage it"""
    for fault in ("halo-left", "halo-right", "halo-top", "halo-bottom"):
        for kind in ((R.SUM, R.MEAN), (R.MIN, R.MAX), ("convolve",)):
            want = lambda ct, a, m, r, what, f: what in kind and FAULTS[fault][1](ct, a, m, r, what, f)
            assert first_exposure(fault, (0, 9), want=want) is not None, (fault, kind)


def test_a_nan_under_a_cleared_mask_byte_shows_when_it_is_multiplied_by_zero():
    """NaN * 0 = NaN: only the raw hashed floats of test_raw_hashed_floats_nan_by_class hold NaNs, masked ones among them"""
    want = lambda ct, a, m, r, what, f: m is not None and (what == "convolve" or what in (R.SUM, R.MEAN))
    assert first_exposure("masked-times-zero", (9, 8), raw=True, want=want) is not None
    assert first_exposure("masked-times-zero", (9,), raw=False, want=want, limit=60) is None   # finite cells times zero add nothing: blind


def test_min_max_by_raw_bits_or_by_less_than_show():
    """negative floats order the other way by raw bits; by < a NaN never wins and -0.0 ties with +0.0"""
    want = lambda ct, a, m, r, what, f: what in (R.MIN, R.MAX)
    assert first_exposure("order-raw-bits", (8, 9), want=want) is not None
    assert first_exposure("order-raw-bits", (4, 7), want=want) is not None        # signed integers by raw bits
    assert first_exposure("order-less-than", (8, 9), raw=True, want=want) is not None
    for dt in (np.float32, np.float64):
        a = K.order_edge_raster(dt)
        for op in (R.MIN, R.MAX):
            for fault in ("order-raw-bits", "order-less-than"):
                assert differs(model(op, a, None, 1, 0, 0, None, fault), R.focal(op, a, None, 1, 0)), (dt, op, fault)
    zeros = np.array([[0.0, -0.0, 0.0, -0.0]])
    got, _ = R.focal(R.MIN, zeros, None, 1, 0)
    assert np.signbit(got).all()
    assert differs(model(R.MIN, zeros, None, 1, 0, 0, None, "order-less-than"), R.focal(R.MIN, zeros, None, 1, 0))
