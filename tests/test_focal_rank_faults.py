"""Would the GPU tests of ec_focal_rank / ec_focal_majority notice a wrong kernel?  Each mistake the kernel can make is modelled here in
numpy (`model`, the rule with one switch thrown: a gather of the footprint in index arrays, a sort, a pick) and run over the inputs,
shapes and radii that tests/test_gpu_focal_rank.py runs (tests/focal_rank_cases.py): for every model at least one of them must give an
answer that differs from tests/focal_rank_ref.py, bit for bit as the GPU file compares — otherwise that file is blind to the fault.
A store that never happens is the exception: it shows only in the pre-filled arenas of tests/test_gpu_focal_rank_bounds.py.  No GPU."""
import numpy as np
import pytest

import focal_rank_cases as K
import focal_rank_ref as R

MAJORITY = None


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(K.UINT[a.dtype.itemsize])


def differs(got, exp):
    return not (np.array_equal(bits(got[0]), bits(exp[0])) and np.array_equal(got[1], exp[1]))


def key_to_words(key, dtype):
    """the inverse of focal_rank_ref.order_key, on uint64 words"""
    width = 8 * dtype.itemsize
    top, ones = np.uint64(1 << (width - 1)), np.uint64((1 << width) - 1)
    if dtype.kind == "f":
        return np.where(key & top != 0, key ^ top, ~key & ones)
    return key ^ top if dtype.kind == "i" else key


def model(a, mask, rx, ry, q, whole, fault=None):
    """what a kernel with the mistake `fault` stores; q = (num, den, method), or MAJORITY"""
    rows, cols = a.shape
    n = rows * cols
    dt = a.dtype
    width = 8 * dt.itemsize
    top, ones = np.uint64(1 << (width - 1)), np.uint64((1 << width) - 1)
    nx, ny = 2 * rx + 1, 2 * ry + 1
    taps, kb = nx * ny, K.bucket((rx, ry))
    I, J = np.mgrid[0:rows, 0:cols]
    x0, y0 = (J // K.TW) * K.TW, (I // K.TH) * K.TH          # the output cell's tile
    flat_w, flat_m = R.words(a).ravel(), (None if mask is None else np.asarray(mask).ravel())
    if fault == "ieee-less" and dt.kind == "f":              # `<` cannot tell -0.0 from +0.0: they tie, and the tap's position decides
        flat_k = R.order_key(np.where(a == 0, np.zeros(1, dt), a)).ravel()
    elif fault == "signedness-confused":                      # signed cells by their raw bits, unsigned ones as if they were signed
        flat_k = flat_w if dt.kind == "i" else flat_w ^ top if dt.kind == "u" else R.order_key(a).ravel()
    else:
        flat_k = R.order_key(a).ravel()
    word, key, on = [], [], []
    for b in range(kb if fault == "bucket-read" else taps):   # "bucket-read": positions past the footprint go on in row-major order
        dy, dx = divmod(b, nx)
        y, x = I - ry + dy, J - rx + dx
        if fault == "seam-off-by-one":                        # every tile but the first of its row reads one column to the left
            x = np.where(x0 > 0, x - 1, x)
        if fault == "wrap":
            at = y * cols + x
            inside = (at >= 0) & (at < n)
        else:
            inside = (y >= 0) & (y < rows) & (x >= 0) & (x < cols)
            at = y * cols + x
        at = np.where(inside, at, 0)
        real = inside
        if fault == "halo-column" and rx > 0:
            real = real & ~(x == x0 + K.TW - 1 + rx)
        elif fault == "halo-row" and ry > 0:
            real = real & ~(y == y0 - ry)
        tap = real if flat_m is None or fault == "mask-ignored" else real & (flat_m[at] != 0)
        w, k = flat_w[at], flat_k[at]
        if fault == "off-raster-counted":                     # a cell off the raster takes part as a zero
            zero_key = R.order_key(np.zeros(1, dt))[0]
            w, k, tap = np.where(inside, w, np.uint64(0)), np.where(inside, k, zero_key), tap | ~inside
        word.append(w), key.append(k), on.append(tap)
    word, key, on = np.stack(word), np.stack(key), np.stack(on)
    count = on.sum(axis=0)
    if fault == "sentinel-low":                               # the sentinel one below the greatest key, in one sort with the taps
        sent = ones - np.uint64(1)
        key = np.where(on, key, sent)
        word = np.where(on, word, key_to_words(np.full(1, sent, np.uint64), dt)[0])
        order = np.argsort(key, axis=0, kind="stable")
    else:
        first = np.argsort(key, axis=0, kind="stable")
        order = np.take_along_axis(first, np.argsort(~np.take_along_axis(on, first, axis=0), axis=0, kind="stable"), axis=0)
    word, key = np.take_along_axis(word, order, axis=0), np.take_along_axis(key, order, axis=0)
    p = word.shape[0]
    if q is MAJORITY:
        is_tap = np.arange(p).reshape(p, 1, 1) < count[None]
        freq = np.zeros(key.shape, np.int64)
        for j in range(p):
            freq += (key == key[j][None]) & is_tap[j][None]
        if fault == "run-into-sentinels" and dt.itemsize == 8:   # the sentinels of an 8-byte cell hold the greatest key: they lengthen its run
            freq += np.where(key == ones, kb - count[None], 0)
        freq = np.where(is_tap, freq, 0)
        if fault == "ties-to-greatest":
            best = p - 1 - np.argmax(freq[::-1], axis=0)
        else:
            best = np.argmax(freq, axis=0)
        picked = np.take_along_axis(word, best[None], axis=0)[0]
    else:
        num, den, method = q
        if fault == "lower-upper-swapped":
            method = 1 - method
        c = np.full(count.shape, taps) if fault == "rank-from-footprint" else count
        table = np.array([0] + [R.position(num, den, method, x) for x in range(1, R.MAX_TAPS + 1)], np.int64)
        picked = np.take_along_axis(word, np.minimum(table[c], p - 1)[None], axis=0)[0]
    valid = (count == taps) if whole else (count > 0)
    out = np.where(valid, picked, np.uint64(0)).astype(K.UINT[dt.itemsize]).view(dt)
    vm = valid.astype(np.uint8)
    if fault == "last-column-skipped":      # never written: the arena's complement of the expected bytes stays (tests/arena.py)
        skip = J % K.TW == K.TW - 1
        out[skip] = (~bits(out))[skip].view(dt)
        vm[skip] ^= 0xff
    elif fault == "last-row-skipped":
        skip = I % K.TH == K.TH - 1
        out[skip] = (~bits(out))[skip].view(dt)
        vm[skip] ^= 0xff
    return out, vm


def reference(a, m, radius, q, whole):
    if q is MAJORITY:
        return R.focal_majority(a, m, radius[0], radius[1], whole)
    return R.focal_rank(a, m, radius[0], radius[1], q[0], q[1], q[2], whole)


def gpu_cases(types, kinds=(None, "hashed")):
    """(ct, a, mask, radius, q, whole) as test_gpu_focal_rank.test_every_radius_shape_and_mask_kind runs them (one_shape: the rank
    raster under every q, the class raster under the majority), smallest rasters first"""
    for radius in K.RADII:
        for cols, rows in sorted(K.shapes(*radius), key=lambda s: s[0] * s[1]):
            for ct in types:
                for kind in kinds:
                    a, c, m = K.sources(ct, kind, cols, rows)
                    for whole in (False, True):
                        for q in K.QS:
                            yield ct, a, m, radius, q, whole
                        yield ct, c, m, radius, MAJORITY, whole


def first_exposure(fault, types, want, kinds=(None, "hashed"), limit=400):
    tried = 0
    for ct, a, m, radius, q, whole in gpu_cases(types, kinds):
        if not want(a, m, radius, q, whole):
            continue
        tried += 1
        if tried > limit:
            break
        if differs(model(a, m, radius[0], radius[1], q, whole, fault), reference(a, m, radius, q, whole)):
            return ct, a.shape, radius, q, whole, m is not None
    return None


def test_the_model_without_a_fault_is_the_rule():
    tried = 0
    for ct, a, m, radius, q, whole in gpu_cases((0, 3, 9)):
        if a.size > 500 or K.taps(radius) > 30:
            continue
        assert not differs(model(a, m, radius[0], radius[1], q, whole), reference(a, m, radius, q, whole)), (ct, a.shape, radius, q, whole)
        tried += 1
    assert tried > 300


RANK = lambda q: q is not MAJORITY
INNER = lambda q: q is not MAJORITY and 0 < q[0] < q[1]
FAULTS = {
    # fault: (cell types tried — all of them among the GPU file's — and which of its cases can show the fault)
    "halo-column": (K.WORD_FORM_TYPES, lambda a, m, r, q, w: a.shape[1] > K.TW and r[0] > 0),
    "halo-row": (K.WORD_FORM_TYPES, lambda a, m, r, q, w: a.shape[0] > K.TH and r[1] > 0),
    "wrap": ((0, 5), lambda a, m, r, q, w: r[0] > 0 and a.shape[0] > 1),
    "mask-ignored": ((0, 8), lambda a, m, r, q, w: m is not None),
    "off-raster-counted": ((5, 9), lambda a, m, r, q, w: r != (0, 0)),
    "rank-from-footprint": ((5, 8), lambda a, m, r, q, w: INNER(q) and r != (0, 0)),
    "lower-upper-swapped": ((5, 9), lambda a, m, r, q, w: INNER(q) and r != (0, 0)),
    "ieee-less": ((8, 9), lambda a, m, r, q, w: r != (0, 0)),
    "signedness-confused": ((0, 5), lambda a, m, r, q, w: r != (0, 0)),
    "sentinel-low": ((9,), lambda a, m, r, q, w: r != (0, 0)),
    "ties-to-greatest": ((0, 9), lambda a, m, r, q, w: q is MAJORITY and r != (0, 0)),
    "run-into-sentinels": ((9,), lambda a, m, r, q, w: q is MAJORITY and r != (0, 0)),
    "bucket-read": ((0, 9), lambda a, m, r, q, w: K.bucket(r) != K.taps(r) and a.shape[0] > r[1] + 1),
    "seam-off-by-one": (K.WORD_FORM_TYPES, lambda a, m, r, q, w: a.shape[1] > K.TW),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_the_gpu_inputs_expose(fault):
    types, want = FAULTS[fault]
    assert first_exposure(fault, types, want) is not None, fault


@pytest.mark.parametrize("fault", ["halo-column", "halo-row", "seam-off-by-one", "bucket-read", "mask-ignored"])
def test_the_gather_faults_show_for_the_rank_and_for_the_majority(fault):
    """one gather feeds both picks, but a test of one pick alone would do: both must notice"""
    types, want = FAULTS[fault]
    for pick in (RANK, lambda q: q is MAJORITY):
        assert first_exposure(fault, types, lambda a, m, r, q, w: pick(q) and want(a, m, r, q, w), limit=1500) is not None, fault


def test_the_sentinel_faults_need_the_greatest_key_and_the_inputs_hold_it():
    """a sentinel below the greatest key, and a majority run that goes on into the sentinels, show only where a tap holds the greatest
    key of an 8-byte cell — a u64 maximum or the all-ones NaN — next to a cell that is no tap: the rank rasters and the palettes of the
    class rasters plant them"""
    for ct in (K.U64, K.F64):
        assert first_exposure("sentinel-low", (ct,), lambda a, m, r, q, w: r != (0, 0), kinds=("hashed",)) is not None, ct
        assert first_exposure("sentinel-low", (ct,), lambda a, m, r, q, w: r != (0, 0), kinds=(None,)) is not None, ct   # the raster's edge
        assert first_exposure("run-into-sentinels", (ct,), lambda a, m, r, q, w: q is MAJORITY and r != (0, 0)) is not None, ct
    # without the planted extremes the rank raster of a u64 would not tell: the fault needs them
    plain = K.K.raster_cells(K.U64, 9, 4, 3)
    assert not differs(model(plain, None, 1, 1, (1, 1, K.LOWER), False, "sentinel-low"), R.focal_rank(plain, None, 1, 1, 1, 1, K.LOWER))


def test_the_order_faults_on_the_order_edge_raster():
    """both zeros side by side, NaNs of both signs, negative values, an infinity: `<` and the total order disagree"""
    for dt in (np.float32, np.float64):
        a = K.K.order_edge_raster(dt)
        shown = [differs(model(a, None, 1, 0, q, False, "ieee-less"), reference(a, None, (1, 0), q, False)) for q in K.QS + [MAJORITY]]
        assert any(shown[:5]) and shown[5], dt


def arena_cases():
    """(kind id, a, mask, radius, q, whole) as tests/test_gpu_focal_rank_bounds.py runs them: its kinds, its shapes, its seeds"""
    import test_gpu_focal_rank_bounds as B
    for kind, name in zip(B.KINDS, B.KIND_IDS):
        ct, q, flags, masked, _, radius = kind
        for k, (cols, rows) in enumerate(B.SHAPES):
            a = K.class_raster(ct, cols, rows, 0xB0 + ct + k) if q is None else K.rank_raster(ct, cols, rows, 0xB0 + ct + k)
            m = K.mask_bytes("hashed", cols, rows, 0xB1 + k) if masked else None
            yield name, a, m, radius, q, bool(flags)


@pytest.mark.parametrize("fault", ["last-column-skipped", "last-row-skipped"])
def test_a_skipped_store_shows_in_the_arenas(fault):
    """A store that never happens shows only where the output was pre-filled with something else: the arenas of
    tests/test_gpu_focal_rank_bounds.py hold the complement of the expected bytes.  Every kind of that file has a shape in which the
    tile's last column and last row exist."""
    import test_gpu_focal_rank_bounds as B
    seen = set()
    for name, a, m, radius, q, whole in arena_cases():
        if differs(model(a, m, radius[0], radius[1], q, whole, fault), reference(a, m, radius, q, whole)):
            seen.add(name)
    assert seen == set(B.KIND_IDS), (fault, sorted(set(B.KIND_IDS) - seen))
