"""The inputs of tests/distance_cases.py expose each modelled mistake of the kernels of ec_distance — shown without a GPU.

`model` below is the two-phase algorithm as the kernels run it (csrc/ec_distance_line.hpp, ec_distance_kernels.hpp), in numpy and
plain Python: column sweeps down and up in chunks of CHUNK rows, a forward and a backward scan of every row over tiles of T columns
with 32-bit parabola values and u16 stack entries, the stacks of a wave's W rows side by side, the result tile stored row by row with
the limit, the square root and the mask byte applied there.  One mistake can be switched on at a time.  The fault-free model equals
tests/distance_ref.py on every case (the largest rasters: on every case whose rows are scanned here within a second or two, named
below); every mistake changes at least one cell or mask byte of at least one case and form that the GPU tests run."""
import numpy as np
import pytest

import distance_cases as K
import distance_ref as R

W, T, CHUNK, INF = K.W, K.T, K.CHUNK, K.INF
M32 = 0xFFFFFFFF
UNWRITTEN = -2      # a cell no store reached (the GPU tests pre-fill their outputs, so such a cell differs)


def columns(m, fault):
    """g of every column at once: the sweeps run over rows, the carry is a row of the raster"""
    rows, cols = m.shape
    target = m != 0
    g = np.full((rows, cols), INF, np.int64)
    if fault != "up-sweep-only":
        d = np.full(cols, INF, np.int64)
        for y in range(rows):
            if fault == "carry-dropped-at-a-chunk-edge" and y % CHUNK == 0:
                d[:] = INF
            d = np.where(target[y], 0, np.where(d == INF, INF, d + 1))
            g[y] = d
    if fault != "down-sweep-only":
        d = np.full(cols, INF, np.int64)
        for k, y in enumerate(range(rows - 1, -1, -1)):
            if fault == "carry-dropped-at-a-chunk-edge" and k % CHUNK == 0:
                d[:] = INF
            d = np.where(target[y], 0, np.where(d == INF, INF, d + 1))
            g[y] = np.minimum(g[y], d)
    return g


def f32(x, i, g2):
    return ((x - i) * (x - i) + g2) & M32


def forward(g, x0, cols, stack, fault):
    """the forward scan over the columns x0 .. x0 + len(g) - 1; stack: lists (s, t, g2), the last entry is the top"""
    S, Tt, G2 = stack
    for k, gu in enumerate(g):
        u = x0 + k
        if gu == INF:
            if fault == "inf-pushed-as-zero":
                gu2 = 0
            elif fault == "inf-pushed-as-inf-squared":
                gu2 = (INF * INF) & M32
            else:
                continue
        else:
            gu2 = gu * gu
        while S:
            a, b = f32(Tt[-1], S[-1], G2[-1]), f32(Tt[-1], u, gu2)
            if not (a >= b if fault == "pop-on-equal" else a > b):
                break
            S.pop(), Tt.pop(), G2.pop()
        w = 0
        if S:
            num, den = u * u - S[-1] * S[-1] + gu2 - G2[-1], 2 * (u - S[-1])
            if fault == "sep-rounded-up":
                w = 1 + -(-num // den)
            elif fault == "sep-without-plus-one":
                w = num // den
            else:
                w = 1 + num // den
            if w >= cols and fault != "push-unguarded":
                continue
        S.append(u), Tt.append(w & 0xFFFF), G2.append(gu2)


def backward(x0, n, stack, q, read=None):
    """the backward scan over x0 + n - 1 .. x0 from stack depth q (entries 0 .. q - 1) -> (d2 of the n columns, the new q); read: the
    stack whose entries a pop loads (the lane's own, unless a mistake says otherwise)"""
    S, Tt, G2 = stack
    rS, rT, rG2 = stack if read is None else read
    out = [0] * n
    top = (S[q - 1], Tt[q - 1], G2[q - 1]) if q > 0 else None
    for k in range(n - 1, -1, -1):
        u = x0 + k
        if top is None:
            out[k] = -1
            continue
        out[k] = f32(u, top[0], top[2])
        if u == top[1]:
            q -= 1
            top = (rS[q - 1], rT[q - 1], rG2[q - 1]) if 0 < q <= len(rS) else None
    return out, q


def rows_phase(g, fault):
    """d2 of every cell (-1: no parabola, UNWRITTEN: no store reached it), by waves of W rows and tiles of T columns"""
    rows, cols = g.shape
    flat = g.ravel()
    d2 = np.full((rows, cols), UNWRITTEN, np.int64)
    tiles = [(x0, min(T, cols - x0)) for x0 in range(0, cols, T)]
    for y0 in range(0, rows, W):
        lanes = range(y0, min(y0 + W, rows))
        if fault == "last-partial-tile-skipped-in-y" and len(lanes) < W:
            continue
        stacks = {}
        for y in lanes:
            stack = ([], [], [])
            for x0, n in tiles:
                if fault == "envelope-rebuilt-per-tile":
                    continue
                if fault == "row-scan-wraps-into-the-next-row":   # a whole tile is read where the row ends inside it
                    piece = flat[y * cols + x0:y * cols + x0 + T]
                else:
                    piece = g[y, x0:x0 + n]
                forward(piece.tolist(), x0, cols, stack, fault)
            stacks[y] = stack
        for y in lanes:
            if fault == "envelope-rebuilt-per-tile":
                for x0, n in tiles:
                    stack = ([], [], [])
                    forward(g[y, x0:x0 + n].tolist(), x0, cols, stack, fault)
                    stack[1][0:1] = [x0] * min(1, len(stack[1]))   # its first parabola starts with the tile
                    d2[y, x0:x0 + n] = backward(x0, n, stack, len(stack[0]))[0]
                continue
            read = stacks.get(y + 1, stacks[y]) if fault == "stack-of-the-next-lane" else None
            q = len(stacks[y][0])
            for x0, n in reversed(tiles):
                out, q = backward(x0, n, stacks[y], q, read)
                if fault == "last-partial-tile-skipped-in-x" and n < T:
                    continue
                d2[y, x0:x0 + n] = out
    if fault == "tile-stored-transposed":   # rows and columns swapped where the result is stored
        swapped = np.full(rows * cols, UNWRITTEN, np.int64)
        y, x = np.mgrid[0:rows, 0:cols]
        swapped[(x * rows + y).ravel()] = d2.ravel()
        d2 = swapped.reshape(rows, cols)
    return d2


STRUCTURAL = ["down-sweep-only", "up-sweep-only", "carry-dropped-at-a-chunk-edge", "inf-pushed-as-zero", "inf-pushed-as-inf-squared", "sep-rounded-up",
              "sep-without-plus-one", "push-unguarded", "envelope-rebuilt-per-tile", "stack-of-the-next-lane", "row-scan-wraps-into-the-next-row",
              "tile-stored-transposed", "last-partial-tile-skipped-in-x", "last-partial-tile-skipped-in-y"]
STORING = ["limit-exclusive", "square-root-in-f32", "mask-byte-set-without-a-target", "values-stored-in-invalid-cells"]
EQUIVALENT = ["pop-on-equal"]


def finish(d2, max_sq, out_type, fault):
    """(cell bits as u64, mask bytes; UNWRITTEN cells as all-ones / 0xFF) of the model's d2 under the storing rules"""
    none = d2 == -1
    unwritten = d2 == UNWRITTEN
    valid = ~none & ~unwritten & ((d2 < max_sq) if fault == "limit-exclusive" else (d2 <= max_sq))
    kept = np.where(valid | ((fault == "values-stored-in-invalid-cells") & ~unwritten), d2 & M32, 0)
    if out_type == R.U32:
        bits = kept.astype(np.uint64)
    elif fault == "square-root-in-f32":
        bits = np.sqrt(kept.astype(np.float32)).astype(np.float64).view(np.uint64)
    else:
        bits = np.sqrt(kept.astype(np.float64)).view(np.uint64)
    mask = valid.astype(np.uint8)
    if fault == "mask-byte-set-without-a-target":
        mask = (valid | none).astype(np.uint8)
    return np.where(unwritten, np.uint64(0xFFFFFFFFFFFFFFFF), bits), np.where(unwritten, 0xFF, mask).astype(np.uint8)


def model_d2(case, fault=None):
    return rows_phase(columns(K.mask(*case), fault), fault)


def expected(case, max_sq, out_type):
    cells, valid = K.expected(*case, max_sq, out_type)
    return (cells.astype(np.uint64) if out_type == R.U32 else cells.view(np.uint64)), valid


def differs(d2, case, fault):
    """does the model's answer differ from the reference in a form the GPU tests run?  (u32 and f64 without a limit, every limit)"""
    for out_type in (R.U32, R.F64):
        for max_sq in K.limits(*case):
            bits, mask = finish(d2, max_sq, out_type, fault)
            eb, ev = expected(case, max_sq, out_type)
            if not (np.array_equal(bits, eb) and np.array_equal(mask, ev)):
                return True
    return False


# the cases a mistake is looked for in, small ones first: every shape up to 2T + 1 with every pattern
SEARCH = sorted(K.cases(K.SMALL), key=lambda c: c[0] * c[1])
# the fault-free model is run on all of those, on the long lines, and on the 257 x 300 patterns below
MODEL_CASES = K.cases(K.SMALL) + K.cases(K.LONG) + [(257, 300, p) for p in ("none", "centre", "random1", "diagonal", "decreasing-g", "last-column-one")]


def test_the_fault_free_model_is_the_reference():
    for case in MODEL_CASES:
        d2 = model_d2(case)
        want, any_target = K.squared(*case)
        assert np.array_equal(d2, want), case
        assert any_target == bool((d2 >= 0).any())
    for case in ((K.T + 1, 2 * K.W + 3, "random1"), (K.T, 3, "none"), (2 * K.T + 1, K.W - 1, "diagonal")):
        assert not differs(model_d2(case), case, None)


@pytest.mark.parametrize("fault", STRUCTURAL + STORING)
def test_every_mistake_changes_an_answer(fault):
    found = None
    for case in SEARCH:
        d2 = model_d2(case, fault if fault in STRUCTURAL else None)
        if differs(d2, case, fault):
            found = case
            break
    assert found is not None, f"no input of distance_cases.py exposes {fault}"


def test_popping_on_equal_values_is_no_mistake():
    """`>=` instead of `>` in the pop test cannot change an answer, and the inputs agree: f(t, s) == f(t, u) with u right of s means u is
    nowhere above s from t on, where s starts — s is redundant, and u's start against the entry below is computed as for any push.  The
    kernels keep Meijster's strict test; this model shows the inputs do not tell the two apart, as reasoning says none can."""
    for case in SEARCH[::7]:
        assert not differs(model_d2(case, "pop-on-equal"), case, "pop-on-equal"), case
