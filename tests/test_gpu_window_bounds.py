"""The window kernels write all of their output and nothing else — wherever the contiguous side sits — and leave their inputs alone.

tests/test_gpu_window.py and tests/test_gpu_resample.py are strict about values and about the raster side of a paste, but every
contiguous-side buffer there (the output of a cut, the tile of a paste, their mask streams) is a fresh 256-byte-aligned block of
which only [0, n) is read back.  Here every call goes through the C ABI with pointers into guarded arenas (tests/arena.py):

  * the output of a cut or of a resampling and its mask stream each sit in an arena of their own, pre-filled with the complement
    of the expected result between random guards, the values at cell offsets {0, 1, 16 / W - 1} and the mask at byte offsets
    (0, 1, 3, 8, 15) behind a 256-byte boundary, the two chosen independently;
  * the source raster, the source mask, the tile and the tile mask sit in operand arenas at cell offsets 0 and 1 and are compared
    byte for byte, guards included, after every test;
  * the destination of a paste is an arena that holds a whole raster (its window pre-filled with the complement of the tile) and
    is compared, guards included, with numpy's slice assignment; its mask likewise.

Expected values are numpy slices, the integer nearest-neighbour rule of test_gpu_window.py and resample_ref.resample; the
resampling sources are the folded-exponent floats of test_gpu_resample.py, so every comparison is bit for bit.  Each family runs
under dict() and dict(unaligned_vector=0); the pointer residues that decide between the vector and the cell-wise kernels
(`rows_aligned` in ec_window.hip, `cellwise_stores` in ec_window_resample.hip) are asserted from the pointers themselves, and each
sweep asserts which combinations it has made.  tests/test_window_arena_faults.py shows (without a GPU) that these arenas, offsets
and shapes notice the faults this file is for.

Sizes of the contiguous side come from the kernels' constants, restated here: a lane owns 16-byte slots of CPL = 16 / W cells, a
workgroup of 256 lanes a tile of 4 slots per lane, T = 256 * 4 * CPL cells; the mask stream of the copying kernels has 16-byte
slots of its own over the same cells (1024 / W of them per tile), that of the resampling kernel CPL bytes per value slot.
"""
import numpy as np
import pytest

import resample_ref as R
import test_gpu_resample as TR
import test_gpu_window as TW
from arena import Arena, noise, operand, output
from oracle import eco

pytestmark = pytest.mark.gpu

EC_OK, EC_ERR_ARG = 0, 6
WIDTHS = (1, 2, 4, 8)
MASK_OFFS = (0, 1, 3, 8, 15)   # bytes
IN_OFFS = (0, 1)               # cells
COPY_TYPES = {1: eco.I8, 2: eco.U16, 4: eco.F32, 8: eco.I64}    # the copying kernels are typed by width only
RESAMPLE_TYPES = (eco.U8, eco.I16, eco.F32, eco.F64, eco.U64)   # the typed kernel: both floats and a 64-bit integer
ARMS = [dict(), dict(unaligned_vector=0)]
ARM_IDS = ["default", "cellwise-when-unaligned"]
X0, Y0 = 3, 1                  # where the windows of the resampling sweeps start
MAX_REDUCTION = 64             # EC_WINDOW_MAX_REDUCTION


def cpl(W):
    return 16 // W


def tile(W):
    return 256 * 4 * cpl(W)


def width_of(ct):
    return np.dtype(eco.NP_DTYPES[ct]).itemsize


def value_offs(W):
    return sorted({0, 1, cpl(W) - 1})


def offset_pairs(W, masked):
    """(cell offset of the values, byte offset of the mask): every pair, so that each is misaligned alone and with the other"""
    return [(vo, mo) for vo in value_offs(W) for mo in (MASK_OFFS if masked else (0,))]


def _odd_rows(lo, hi):
    """(w, h) with w odd, the fewest h >= 3 rows and lo < w * h < hi"""
    for h in range(3, 64):
        for n in range(lo + 1, hi):
            if n % h == 0 and (n // h) % 2 == 1:
                return n // h, h
    raise AssertionError((lo, hi))


def single_rows(W):
    c, t = cpl(W), tile(W)
    return sorted({1, c - 1, c, c + 1, t - 1, t, t + 1, t + 2, 2 * t + c + 3})


def shapes(W):
    """(w, h) of the contiguous side: the single rows, odd-width blocks below a tile, above one and above two, narrow windows
    whose slots span several rows, one block whose rows all start on 16-byte boundaries at every width, and three rows one cell
    wider than a tile: the lane map's wide branch (the window at least a tile wide) with slots that wrap into the next row"""
    c, t = cpl(W), tile(W)
    multi = [_odd_rows(t - c, t), _odd_rows(t, t + c), _odd_rows(2 * t, 2 * t + 64)]
    narrow = [(1, c + 3), (3, c // 3 + 2)]
    return [(n, 1) for n in single_rows(W)] + multi + narrow + [(t + 1, 3), (48, 5)]


def put_x0s(W):
    """the first column of a paste: destination row starts at 0 mod 16 for values and mask (16), for the values (CPL), CPL - 1
    cells behind a boundary and at an odd cell (5, which is no CPL - 1)"""
    return sorted({16, cpl(W), cpl(W) - 1, 5})


def put_cols(x0, w):
    """cells per row of a paste's destination: at least one spare column right of the window; a multiple of 16 (every row start
    has the residue of x0) except for the odd x0 = 5, where the pitch is odd and the row starts take every residue"""
    return (x0 + w + 2) | 1 if x0 == 5 else x0 + w + 1 - (x0 + w + 1) % -16


def cut_placements(W):
    """(cell offset of the source arenas, x0): all aligned, an odd column, an odd pointer, and an odd pointer whose row starts
    are aligned again"""
    return [(0, 0), (0, 3), (1, 0), (1, cpl(W) - 1)]


def window_for(kind, ow, oh):
    """the window that is read at ow x oh: `same`, a fractional reduction (3 : 2), a fractional enlargement (2 : 3), a whole
    factor (2 : 1).  A single output row is a single window row (the column axis alone resamples)."""
    scale = {"same": lambda k: k, "down": lambda k: (3 * k + 1) // 2, "up": lambda k: (2 * k + 2) // 3, "whole": lambda k: 2 * k}[kind]
    return scale(ow), oh if oh == 1 else scale(oh)


NEAREST_KINDS = ("down", "up", "whole")


def nearest_kind(k, ow):
    """the window kind of shape number k of a nearest-neighbour cut: 3 : 2 and 2 : 3 in turn; an output row of a multiple of 16
    cells is read from twice as many, so that the rows of the WINDOW can start on 16-byte boundaries as well"""
    return "whole" if ow % 16 == 0 else NEAREST_KINDS[k % 2]
RESAMPLE_KINDS = {R.AVERAGE: ("down", "up", "whole"), R.BILINEAR: ("down", "up")}


def resample_kind(alg, ct, k):
    """the window kind of shape number k: the kinds rotate over the shapes, from another start for every cell type"""
    kinds = RESAMPLE_KINDS[alg]
    return kinds[(k + RESAMPLE_TYPES.index(ct)) % len(kinds)]


def _assert_the_lists_are_what_the_kernels_need():
    for W in WIDTHS:
        c, t, sh = cpl(W), tile(W), shapes(W)
        assert t == 256 * 4 * (16 // W) and c == 16 // W
        ns = [w * h for w, h in sh]
        assert {1, c - 1, c, c + 1, t - 1, t, t + 1, t + 2, 2 * t + c + 3} <= {w for w, h in sh if h == 1}
        blocks = [(w, h) for w, h in sh if w % 2 == 1 and h >= 3 and w > 3]
        assert any(t - c < w * h < t for w, h in blocks) and any(t < w * h < t + c for w, h in blocks) and any(w * h > 2 * t for w, h in blocks)
        assert all(any(w == nw and h > 1 and w * h > c for w, h in sh) for nw in (1, 3))
        assert {0, 1, c % 16, 15} <= {n % 16 for n in ns}, W
        assert any(h > 1 and w * W % 16 == 0 and w % 16 == 0 for w, h in sh)
        assert {vo * W % 16 for vo in value_offs(W)} == {0, W % 16, 16 - W} and set(MASK_OFFS) == {0, 1, 3, 8, 15}
        # a paste: spare cells on every side, and the row starts of the destination (y0 = 1) at 0, at CPL - 1 cells and at an odd cell
        for w, h in sh:
            assert all(x0 >= 1 and put_cols(x0, w) >= x0 + w + 1 for x0 in put_x0s(W))
        starts = {x0: {((1 + r) * put_cols(x0, 48) + x0) * W % 16 for r in range(5)} for x0 in put_x0s(W)}
        assert starts[16] == {0} and starts[c] == {0} and starts[c - 1] == {(c - 1) * W} 
        assert len(starts[5]) > 1 and any(x // W % 2 == 1 for x in starts[5])
        # the resampling windows: a fractional reduction, a fractional enlargement and (the average) a whole factor, below the cap
        for alg, kinds in RESAMPLE_KINDS.items():
            assert set(kinds) >= {"down", "up"} and ("whole" in kinds) == (alg == R.AVERAGE)
        for ow, oh in sh:
            for kind in ("down", "up", "whole"):
                w, h = window_for(kind, ow, oh)
                assert 1 <= w <= MAX_REDUCTION * ow and 1 <= h <= MAX_REDUCTION * oh
        ow, oh = sh[-1]
        assert window_for("down", ow, oh) == (72, 8) and window_for("up", ow, oh) == (32, 4) and window_for("whole", ow, oh) == (96, 10)
    assert MAX_REDUCTION == R.MAX_REDUCTION


_assert_the_lists_are_what_the_kernels_need()


def source_dims(W, kinds):
    """(cols, rows) of the raster that holds every window of a sweep at every placement; cols a multiple of 16"""
    wins = [window_for(kind, ow, oh) for ow, oh in shapes(W) for kind in kinds]
    cols = max(w for w, h in wins) + max(cpl(W), X0) + 1
    return cols - cols % -16, max(h for w, h in wins) + Y0 + 1


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def _seed(*parts):
    return hash(parts) & 0xFFFF


class Sources:
    """The inputs: per (family, cell type, cell offset) one raster and its mask, each in a guarded arena of its own, uploaded once;
    per (cell type, cell offset) the cells that tiles are prefixes of, and their mask bytes.  A sweep reads windows of them."""

    def __init__(self, ec):
        self.ec, self.hosts, self.arenas = ec, {}, {}

    def host(self, family, ct):
        key = (family, ct)
        if key not in self.hosts:
            W = width_of(ct)
            if family == "cut":        # hashed bytes, mask bytes 0 / 1
                cols, rows = source_dims(W, ("same",) + NEAREST_KINDS)
                a = TW.raster_cells(self.ec, ct, cols, rows, 0xB0D5 + ct)
                m = eco.fill_u8(cols * rows, 0xB0D6 + ct, lo=0, hi=1).reshape(rows, cols)
            elif family == "resample":  # folded-exponent floats, 60 % of the cells valid
                cols, rows = source_dims(W, ("down", "up", "whole"))
                a = TR.raster_cells(self.ec, ct, cols, rows, 0xB0D7 + ct)
                m = (eco.fill_u8(cols * rows, 0xB0D8 + ct, lo=0, hi=99).reshape(rows, cols) < 60).astype(np.uint8)
            else:                       # the tiles of a paste: prefixes of one row of hashed cells
                n = max(w * h for w, h in shapes(W))
                a = TW.raster_cells(self.ec, ct, n, 1, 0xB0D9 + ct)
                m = eco.fill_u8(n, 0xB0DA + ct, lo=0, hi=1).reshape(1, n)
            self.hosts[key] = (a, m)
        return self.hosts[key]

    def get(self, family, ct, off, mask_off=None):
        """(pointer to the first cell, pointer to the first mask byte, host cells, host mask) with the cells `off` cells and the
        mask `mask_off` bytes (default: `off`) behind a 256-byte boundary"""
        a, m = self.host(family, ct)
        mask_off = off if mask_off is None else mask_off
        for key, what, o in (((family, ct, "cells", off), a, off), ((family, ct, "mask", mask_off), m, mask_off)):
            if key not in self.arenas:
                self.arenas[key] = operand(self.ec, what, o, seed=len(self.arenas) + 1)
        pa, pm = self.arenas[family, ct, "cells", off].ptr, self.arenas[family, ct, "mask", mask_off].ptr
        assert pa % 16 == off * width_of(ct) % 16 and pm % 16 == mask_off
        return pa, pm, a, m

    def recheck(self):
        for key, a in self.arenas.items():
            a.check_unchanged(f"input {key}")


@pytest.fixture(scope="module")
def sources(ec):
    return Sources(ec)


@pytest.fixture(autouse=True)
def inputs_stay_as_they_were(sources):
    yield
    sources.recheck()


_memo = {}   # expected results, shared between the knob arms: they do not depend on a knob


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _outputs(ec, W, exp, em, vo, mo, masked, seed):
    out = output(ec, exp, vo, seed)
    om = output(ec, em, mo, seed + 1) if masked else None
    assert out.ptr % 16 == vo * W % 16 and (om is None or om.ptr % 16 == mo)
    return out, om


# ================================================================ ec_window: the copy and the nearest-neighbour cut
def _cut_expected(a, m, x0, w, h, ow, oh):
    if (w, h) == (ow, oh):
        return a[Y0:Y0 + h, x0:x0 + w].ravel().copy(), m[Y0:Y0 + h, x0:x0 + w].ravel().copy()
    return TW.resampled(a, x0, Y0, w, h, ow, oh).ravel(), TW.resampled(m, x0, Y0, w, h, ow, oh).ravel()


@pytest.mark.parametrize("arm", ARMS, ids=ARM_IDS)
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("family", ["copy", "nearest"])
def test_cut(ec, sources, family, W, masked, arm):
    """`dst` holds out_cols * out_rows cells and `dst_mask` as many bytes afterwards, nothing around them has changed.  With
    unaligned_vector = 0 the vector kernel runs where the source's row starts and both output pointers are 16-byte aligned
    and the cell-wise kernel everywhere else: the launches where the raster side is aligned and only `dst`, only `dst_mask`
    or neither is misaligned are all made (asserted below)."""
    L, chk, ct = ec.lib(), ec._ffi.check, COPY_TYPES[W]
    seen = set()
    with ec.tuned(**arm):
        for io, x0 in cut_placements(W):
            src, smask, a, m = sources.get("cut", ct, io)
            rows, cols = a.shape
            for k, (ow, oh) in enumerate(shapes(W)):
                w, h = window_for("same" if family == "copy" else nearest_kind(k, ow), ow, oh)
                exp, em = memo(("cut", ct, x0, w, h, ow, oh), lambda: _cut_expected(a, m, x0, w, h, ow, oh))
                origin = Y0 * cols + x0
                raster_aligned = ((src + origin * W) | (cols * W) | (w * W)) % 16 == 0
                mask_raster_aligned = ((smask + origin) | cols | w) % 16 == 0
                for vo, mo in offset_pairs(W, masked):
                    what = f"ec_window {family} {eco.CT_NAMES[ct]} {'masked ' if masked else ''}{w} x {h} at ({x0}, {Y0}) -> {ow} x {oh}, source +{io} cells, out +{vo} cells, mask +{mo} bytes, {arm}"
                    out, om = _outputs(ec, W, exp, em, vo, mo, masked, _seed(ow, oh, vo, mo))
                    chk(L.ec_window(ct, src, smask if masked else None, cols, rows, x0, Y0, w, h, ow, oh, out.ptr, om.ptr if masked else None, ec.stream()))
                    out.check(exp, what + ": values")
                    if masked:
                        om.check(em, what + ": mask")
                    seen.add((raster_aligned and (mask_raster_aligned or not masked), out.ptr % 16 != 0, masked and om.ptr % 16 != 0))
    # every outcome of rows_aligned that the contiguous side decides, and the raster side's own
    want = {(True, False, False), (True, True, False), (False, False, False), (False, True, False)}
    if masked:
        want |= {(True, False, True), (True, True, True), (False, False, True), (False, True, True)}
    assert seen == want, sorted(want - seen)


# ================================================================ ec_window_put
def _put_destination(ec, ct, cols, rows, x0, w, h, tile_cells, tile_mask):
    """The raster a tile is pasted into and its mask: hashed cells, mask bytes 2 .. 255 (no stray mask byte equals them), and the
    window itself the complement of the tile (mask: the other of 0 / 1): a byte of the window that is not written cannot pass."""
    base = TW.raster_cells(ec, ct, cols, rows, 0x9A57 + x0 + 7 * w)
    bm = eco.fill_u8(cols * rows, 0x9A58 + x0 + 7 * w, lo=2, hi=255).reshape(rows, cols)
    TW.bits(base)[1:1 + h, x0:x0 + w] = ~TW.bits(tile_cells)
    bm[1:1 + h, x0:x0 + w] = tile_mask ^ 1
    return base, bm


@pytest.mark.parametrize("arm", ARMS, ids=ARM_IDS)
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("W", WIDTHS)
def test_put(ec, sources, W, masked, arm):
    """The whole destination arena — raster and guards — equals numpy's slice assignment, and so does its mask; the tile and
    its mask sit at cell / byte offsets 0 and 1, each on its own."""
    L, chk, ct = ec.lib(), ec._ffi.check, COPY_TYPES[W]
    seen = set()
    with ec.tuned(**arm):
        for w, h in shapes(W):
            n, rows = w * h, h + 2
            for x0 in put_x0s(W):
                cols = put_cols(x0, w)
                _, _, cells, mask = sources.get("tile", ct, 0)
                t_cells, t_mask = cells[0, :n].reshape(h, w), mask[0, :n].reshape(h, w)
                base, bm = _put_destination(ec, ct, cols, rows, x0, w, h, t_cells, t_mask)
                exp, expm = base.copy(), bm.copy()
                exp[1:1 + h, x0:x0 + w], expm[1:1 + h, x0:x0 + w] = t_cells, t_mask
                for to, tmo in ([(0, 0), (1, 0), (0, 1), (1, 1)] if masked else [(0, 0), (1, 0)]):
                    what = f"ec_window_put {eco.CT_NAMES[ct]} {'masked ' if masked else ''}{w} x {h} at ({x0}, 1) of {cols} x {rows}, tile +{to} cells, tile mask +{tmo} bytes, {arm}"
                    tp, tmp, _, _ = sources.get("tile", ct, to, tmo)
                    dst = Arena(base.nbytes, seed=_seed(w, h, x0, to), ec=ec).hold(base)
                    dm = Arena(bm.nbytes, seed=_seed(w, h, x0, tmo, 1), ec=ec).hold(bm) if masked else None
                    origin = cols + x0
                    raster_aligned = ((dst.ptr + origin * W) | (cols * W) | (w * W)) % 16 == 0
                    mask_raster_aligned = not masked or ((dm.ptr + origin) | cols | w) % 16 == 0
                    chk(L.ec_window_put(ct, tp, tmp if masked else None, w, h, dst.ptr, dm.ptr if masked else None, cols, rows, x0, 1, ec.stream()))
                    dst.check(exp, what + ": values")
                    if masked:
                        dm.check(expm, what + ": mask")
                    seen.add((raster_aligned and mask_raster_aligned, tp % 16 != 0, masked and tmp % 16 != 0))
    want = {(True, False, False), (True, True, False), (False, False, False), (False, True, False)}
    if masked:
        want |= {(True, False, True), (True, True, True), (False, False, True), (False, True, True)}
    assert seen == want, sorted(want - seen)


# ================================================================ ec_window_resample: average and bilinear
def _resample_expected(alg, a, m, w, h, ow, oh):
    exp, em = R.resample(alg, a, m, X0, Y0, w, h, ow, oh)
    return exp.ravel(), em.ravel()


@pytest.mark.parametrize("arm", ARMS, ids=ARM_IDS)
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("ct", RESAMPLE_TYPES, ids=[eco.CT_NAMES[ct] for ct in RESAMPLE_TYPES])
@pytest.mark.parametrize("name", ["Average", "Bilinear"])
def test_resample(ec, sources, name, ct, masked, arm):
    """The shapes are the OUTPUT's.  With unaligned_vector = 0 a misaligned `dst` or `dst_mask` sets ResampleArgs::cellwise_stores
    (the `!whole` arm of k_window_resample for every slot): values aligned and mask not, the reverse, both and neither are all
    run (asserted below), and each writes the same cells and the same mask bytes between untouched guards."""
    L, chk, W, alg = ec.lib(), ec._ffi.check, width_of(ct), TR.ALGS[name]
    seen = set()
    with ec.tuned(**arm):
        for io in IN_OFFS:
            src, smask, a, m = sources.get("resample", ct, io)
            rows, cols = a.shape
            for k, (ow, oh) in enumerate(shapes(W)):
                w, h = window_for(resample_kind(alg, ct, k), ow, oh)
                exp, em = memo(("resample", alg, ct, masked, w, h, ow, oh), lambda: _resample_expected(alg, a, m if masked else None, w, h, ow, oh))
                for vo, mo in offset_pairs(W, masked):
                    what = f"ec_window_resample {name} {eco.CT_NAMES[ct]} {'masked ' if masked else ''}{w} x {h} at ({X0}, {Y0}) -> {ow} x {oh}, source +{io} cells, out +{vo} cells, mask +{mo} bytes, {arm}"
                    out, om = _outputs(ec, W, exp, em, vo, mo, masked, _seed(ow, oh, vo, mo, 2))
                    chk(L.ec_window_resample(alg, ct, src, smask if masked else None, cols, rows, X0, Y0, w, h, ow, oh, out.ptr, om.ptr if masked else None, ec.stream()))
                    out.check(exp, what + ": values")
                    if masked:
                        om.check(em, what + ": mask")
                    if (w, h) != (ow, oh):   # (equal sizes are the copy: ec_window, covered by test_cut)
                        seen.add((out.ptr % 16 != 0, masked and om.ptr % 16 != 0))
    assert seen == ({(False, False), (True, False), (False, True), (True, True)} if masked else {(False, False), (True, False)})


# ================================================================ calls that must write nothing
def test_refused_and_empty_calls_write_nothing(ec):
    """An empty window with an empty output is EC_OK; everything the header lists as refused is EC_ERR_ARG; either way every
    arena — inputs, outputs, their guards — is as it was."""
    L, s, ct = ec.lib(), ec.stream(), eco.U16
    cols, rows = 140, 70
    a = TW.raster_cells(ec, ct, cols, rows, 0xE3F7)
    m = eco.fill_u8(cols * rows, 0xE3F8, lo=0, hi=1)
    src, smask = operand(ec, a, 1, seed=1), operand(ec, m, 1, seed=2)
    dst = Arena(2 * cols * rows, offset=2, seed=3, ec=ec).hold(noise(2 * cols * rows, 4))
    dmask = Arena(cols * rows, offset=3, seed=5, ec=ec).hold(noise(cols * rows, 6))
    arenas = {"src": src, "src_mask": smask, "dst": dst, "dst_mask": dmask}
    S, SM, D, DM = src.ptr, smask.ptr, dst.ptr, dmask.ptr

    def window(x0, y0, w, h, ow, oh, sm=None, dm=None):
        return lambda: L.ec_window(ct, S, sm, cols, rows, x0, y0, w, h, ow, oh, D, dm, s)

    def resample(alg, x0, y0, w, h, ow, oh, sm=None, dm=None):
        return lambda: L.ec_window_resample(alg, ct, S, sm, cols, rows, x0, y0, w, h, ow, oh, D, dm, s)

    def put(x0, y0, w, h, tm=None, dm=None):   # the tile is `src`, the raster `dst`
        return lambda: L.ec_window_put(ct, S, tm, w, h, D, dm, cols, rows, x0, y0, s)

    calls = [
        ("an empty window, an empty output", EC_OK, window(3, 1, 0, 0, 0, 0)),
        ("an empty window of one empty axis", EC_OK, window(3, 1, 5, 0, 0, 7, SM, DM)),
        ("an empty average", EC_OK, resample(R.AVERAGE, 3, 1, 0, 0, 0, 0, SM, DM)),
        ("an empty bilinear read", EC_OK, resample(R.BILINEAR, 3, 1, 0, 4, 2, 0)),
        ("an empty paste", EC_OK, put(3, 1, 0, 0, SM, DM)),
        ("an empty paste of one empty axis", EC_OK, put(3, 1, 7, 0)),
        ("a window past the right edge", EC_ERR_ARG, window(cols - 4, 1, 5, 3, 5, 3)),
        ("a window past the bottom", EC_ERR_ARG, window(3, rows - 2, 5, 3, 5, 3, SM, DM)),
        ("a window that starts outside", EC_ERR_ARG, window(cols + 1, 0, 1, 1, 1, 1)),
        ("a resampled window past the right edge", EC_ERR_ARG, window(cols - 4, 1, 5, 3, 9, 2)),
        ("an average of a window past the bottom", EC_ERR_ARG, resample(R.AVERAGE, 3, rows - 2, 6, 3, 3, 1, SM, DM)),
        ("a bilinear read of a window past the right edge", EC_ERR_ARG, resample(R.BILINEAR, cols - 4, 1, 5, 3, 9, 2)),
        ("a paste past the right edge", EC_ERR_ARG, put(cols - 4, 1, 5, 3)),
        ("a paste past the bottom", EC_ERR_ARG, put(3, rows - 2, 5, 3, SM, DM)),
        ("a source mask alone", EC_ERR_ARG, window(3, 1, 5, 3, 5, 3, SM, None)),
        ("an output mask alone", EC_ERR_ARG, window(3, 1, 5, 3, 5, 3, None, DM)),
        ("a source mask alone, resampled", EC_ERR_ARG, window(3, 1, 6, 4, 3, 2, SM, None)),
        ("a source mask alone, averaged", EC_ERR_ARG, resample(R.AVERAGE, 3, 1, 6, 4, 3, 2, SM, None)),
        ("an output mask alone, bilinear", EC_ERR_ARG, resample(R.BILINEAR, 3, 1, 6, 4, 9, 5, None, DM)),
        ("a tile mask alone", EC_ERR_ARG, put(3, 1, 5, 3, SM, None)),
        ("a destination mask alone", EC_ERR_ARG, put(3, 1, 5, 3, None, DM)),
        ("an average of columns beyond the cap", EC_ERR_ARG, resample(R.AVERAGE, 3, 1, 2 * MAX_REDUCTION + 1, 4, 2, 2)),
        ("an average of rows beyond the cap", EC_ERR_ARG, resample(R.AVERAGE, 3, 1, 4, MAX_REDUCTION + 1, 4, 1, SM, DM)),
        ("an empty window with an output", EC_ERR_ARG, window(3, 1, 0, 0, 4, 4)),
        ("a window with an empty output", EC_ERR_ARG, window(3, 1, 4, 4, 0, 0, SM, DM)),
        ("an empty window with an averaged output", EC_ERR_ARG, resample(R.AVERAGE, 3, 1, 0, 3, 2, 2)),
        ("a window with an empty bilinear output", EC_ERR_ARG, resample(R.BILINEAR, 3, 1, 4, 4, 3, 0)),
    ] + [(f"algorithm number {alg}", EC_ERR_ARG, resample(alg, 3, 1, 6, 4, 3, 2, SM, DM)) for alg in (2, 3, 4, 6, 7, -1, 255)]
    # at the cap itself the average is accepted — the refusals above are the cap's, not the shape's — and writes 2 x 2 cells
    exp, em = R.resample(R.AVERAGE, a, m.reshape(rows, cols), 3, 1, 2 * MAX_REDUCTION, 4, 2, 2)
    out, om = output(ec, exp.ravel(), 1, seed=7), output(ec, em.ravel(), 3, seed=8)
    assert L.ec_window_resample(R.AVERAGE, ct, S, SM, cols, rows, 3, 1, 2 * MAX_REDUCTION, 4, 2, 2, out.ptr, om.ptr, s) == EC_OK
    out.check(exp.ravel(), "an average at the cap: values")
    om.check(em.ravel(), "an average at the cap: mask")
    for what, status, call in calls:
        assert call() == status, what
        for name, arena in arenas.items():
            arena.check_unchanged(f"{what}: {name}")
