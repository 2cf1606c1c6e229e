"""ec_regions on the device, bit for bit against tests/regions_ref.py (a flood fill in raster order): labels, mask bytes and K for
every shape, pattern and mask of tests/regions_cases.py — lines, squares and oblongs around the tile sides TW and TH, one 257 x 300,
the long rasters 32768 x 1, 1 x 32768 and 32768 x 2 — under both connectivities, both numberings and every sieve of interest; the four
cell widths; the mask form and the sieve-only form; odd byte offsets of both masks; outputs pre-filled with 0xA5; the same bytes from
two calls and from the caller's and the pooled workspace.  No case is skipped or sampled: every cell of every case is compared."""
import ctypes as C

import numpy as np
import pytest

import regions_cases as K
import regions_ref as R

pytestmark = pytest.mark.gpu

DTYPE = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.uint32): 2, np.dtype(np.uint64): 3, np.dtype(np.float32): 8, np.dtype(np.float64): 9}


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


class Dev:
    """a device block with `nbytes` behind `offset` bytes: the pointer the entry point gets sits at any residue"""

    def __init__(self, ec, nbytes, offset=0):
        self.ec, self.nbytes = ec, nbytes
        self.mem = ec.DeviceMem(nbytes + offset + 16)
        self.ptr = self.mem.ptr + offset

    def put(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes == self.nbytes
        self.ec._ffi.check(self.ec.lib().ec_upload(self.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, self.ec.stream()))
        return self

    def get(self, dtype):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype)
        self.ec._ffi.check(self.ec.lib().ec_download(out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes, self.ec.stream()))
        return out


class Inputs:
    """the cells (or None: the mask form) and validity bytes (or None) of one raster on the device, uploaded once for all its calls"""

    def __init__(self, ec, cells, valid, smask_offset=0):
        self.ec, self.cells, self.valid = ec, cells, valid
        self.rows, self.cols = (cells if cells is not None else valid).shape
        self.src = Dev(ec, cells.nbytes).put(cells) if cells is not None else None
        self.smask = Dev(ec, valid.size, smask_offset).put(valid) if valid is not None else None

    def unchanged(self):
        if self.src is not None:
            assert np.array_equal(self.src.get(np.uint8), np.ascontiguousarray(self.cells).view(np.uint8).ravel()), "the input cells changed"
        if self.smask is not None:
            assert np.array_equal(self.smask.get(np.uint8), self.valid.ravel()), "the input mask changed"


def run(ec, inp, connectivity, numbering, min_cells, labels=True, want_mask=True, want_k=True, workspace=False, dmask_offset=0):
    """one call -> (labels or None, mask bytes or None, K or None); the outputs are pre-filled with 0xA5 so that a cell never written shows"""
    n = inp.cols * inp.rows
    L = ec.lib()
    dst = Dev(ec, 4 * n).put(np.full(4 * n, R.UNWRITTEN, np.uint8)) if labels else None
    dmask = Dev(ec, n, dmask_offset).put(np.full(n, R.UNWRITTEN, np.uint8)) if want_mask else None
    k = Dev(ec, 8).put(np.full(8, R.UNWRITTEN, np.uint8)) if want_k else None
    ws = Dev(ec, L.ec_regions_workspace_bytes(inp.cols, inp.rows)) if workspace else None
    st = L.ec_regions(DTYPE[inp.cells.dtype] if inp.cells is not None else 0, inp.src.ptr if inp.src else None, inp.smask.ptr if inp.smask else None,
                      inp.cols, inp.rows, connectivity, numbering, min_cells, dst.ptr if dst else None, dmask.ptr if dmask else None,
                      k.ptr if k else None, ws.ptr if ws else None, ec.stream())
    assert st == 0, L.ec_last_error_string()
    return (dst.get(np.int32) if dst else None, dmask.get(np.uint8) if dmask else None, int(k.get(np.uint64)[0]) if k else None)


def compare(got, exp, cols, what):
    (labels, mask, k), (el, em, ek) = got, exp
    if labels is not None:
        bad = np.flatnonzero(labels != el.ravel())
        assert bad.size == 0, (what, f"{bad.size} labels differ, first (y, x) = {divmod(int(bad[0]), cols)}: got {labels[bad[0]]}, expected {el.ravel()[bad[0]]}")
    if mask is not None:
        bad = np.flatnonzero(mask != em.ravel())
        assert bad.size == 0, (what, f"{bad.size} mask bytes differ, first (y, x) = {divmod(int(bad[0]), cols)}: got {mask[bad[0]]}")
    if k is not None:
        assert k == ek, (what, f"K is {k}, expected {ek}")


def inputs_of(ec, case, form="cells", **kw):
    cols, rows, pattern, mask = case
    if form == "mask":
        return Inputs(ec, None, K.mask_form(case), **kw)
    return Inputs(ec, K.cells(cols, rows, pattern), K.valid(cols, rows, mask), **kw)


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_case_connectivity_numbering_and_sieve(ec, shape):
    for case in K.cases([shape]):
        inp = inputs_of(ec, case)
        for c in (4, 8):
            for numbering in (K.ROOT, K.DENSE):
                for min_cells in K.sieves(case):
                    compare(run(ec, inp, c, numbering, min_cells), K.expected(case, c, numbering, min_cells), case[0], (case, c, numbering, min_cells))
        inp.unchanged()


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_mask_form_and_the_sieve_only_form(ec, shape):
    """src NULL: the regions of the mask itself; dst NULL: only the validity bytes; and the labels without validity bytes — zero bits
    wherever no kept region is, although nothing says so beside them"""
    for case in K.cases([shape]):
        c = 4 if len(case[2]) % 2 else 8
        if case[2] in K.BINARY:
            inp = inputs_of(ec, case, "mask")
            for numbering in (K.ROOT, K.DENSE):
                for min_cells in (0, 5):
                    compare(run(ec, inp, c, numbering, min_cells), K.expected(case, c, numbering, min_cells, "mask"), case[0], (case, c, numbering, min_cells, "mask form"))
            compare(run(ec, inp, 12 - c, K.ROOT, 2, labels=False, want_k=False), K.expected(case, 12 - c, K.ROOT, 2, "mask"), case[0], (case, "mask form, sieve only"))
            inp.unchanged()
        inp = inputs_of(ec, case)
        for min_cells in (0, 2, 5):
            compare(run(ec, inp, c, K.DENSE, min_cells, labels=False, want_k=False), K.expected(case, c, K.DENSE, min_cells), case[0], (case, c, min_cells, "sieve only"))
            compare(run(ec, inp, c, K.DENSE, min_cells, want_mask=False), K.expected(case, c, K.DENSE, min_cells), case[0], (case, c, min_cells, "no dst_mask"))
        compare(run(ec, inp, c, K.ROOT, 2, labels=False, want_mask=False), K.expected(case, c, K.ROOT, 2), case[0], (case, c, "K alone"))
        compare(run(ec, inp, c, K.ROOT, 2, want_mask=False, want_k=False), K.expected(case, c, K.ROOT, 2), case[0], (case, c, "labels alone"))
        inp.unchanged()


def test_the_four_cell_widths(ec):
    """the same three classes as 1-, 2-, 4- and 8-byte cells give the same regions; the wide ones differ only in their top byte"""
    for shape in ((K.TW + 1, K.TH + 1), (2 * K.TW + 1, K.TH - 1), (257, 300)):
        classes = (K.hashed(shape[0] * shape[1], 0x70B0) % np.uint64(3)).astype(np.uint8).reshape(shape[1], shape[0])
        for c in (4, 8):
            want = R.regions(classes, None, c, K.DENSE, 3)
            for pattern in ("wide2", "wide4", "wide8"):
                cells = K.cells(shape[0], shape[1], pattern)
                compare(run(ec, Inputs(ec, cells, None), c, K.DENSE, 3), want, shape[0], (shape, pattern, c))
            compare(run(ec, Inputs(ec, classes, None), c, K.DENSE, 3), want, shape[0], (shape, "one byte", c))
            # f64 and i16 go the way of u64 and u16: only the width matters
            compare(run(ec, Inputs(ec, K.cells(shape[0], shape[1], "wide8").view(np.float64), None), c, K.DENSE, 3), want, shape[0], (shape, "f64", c))


def test_odd_byte_offsets_of_both_masks(ec):
    for shape in ((K.TW + 1, 5), (7, K.TH + 1), (2 * K.TW + 1, 3)):
        for k, (so, do) in enumerate(((1, 0), (0, 1), (3, 7), (15, 9), (5, 5))):
            case = shape + (("random59", "checkerboard", "random3", "serpentine", "wide4")[k], ("random10", "seam")[k % 2])
            inp = inputs_of(ec, case, smask_offset=so)
            for c, numbering, min_cells in ((4, K.DENSE, 0), (8, K.ROOT, 2)):
                compare(run(ec, inp, c, numbering, min_cells, dmask_offset=do), K.expected(case, c, numbering, min_cells), case[0], (case, so, do))
                compare(run(ec, inp, c, numbering, min_cells, labels=False, want_k=False, dmask_offset=do), K.expected(case, c, numbering, min_cells), case[0], (case, so, do))
            inp.unchanged()


def test_the_same_bytes_twice_and_from_either_workspace(ec):
    for case in ((2 * K.TW + 1, K.TH + 1, "random59", "random10"), (K.TW - 1, 2 * K.TH + 1, "spiral", "none"), (257, 300, "random59", "none"),
                 (32768, 2, "serpentine", "none")):
        inp = inputs_of(ec, case)
        for c, numbering, min_cells in ((4, K.DENSE, 0), (8, K.DENSE, 5), (8, K.ROOT, 2)):
            first = run(ec, inp, c, numbering, min_cells)
            again = run(ec, inp, c, numbering, min_cells)
            own = run(ec, inp, c, numbering, min_cells, workspace=True)
            for other in (again, own):
                assert np.array_equal(first[0], other[0]) and np.array_equal(first[1], other[1]) and first[2] == other[2], (case, c, numbering, min_cells)
            compare(own, K.expected(case, c, numbering, min_cells), case[0], (case, "the caller's workspace"))


def test_k_is_the_greatest_dense_label(ec):
    """a cross-check that needs no reference: under DENSE without a sieve the labels of a mask's regions are exactly 1 .. K"""
    for case in ((2 * K.TW + 1, 2 * K.TH + 1, "random59", "none"), (257, 300, "random59", "none"), (K.TW + 1, K.TH + 1, "checkerboard", "seam")):
        for c in (4, 8):
            labels, mask, k = run(ec, inputs_of(ec, case, "mask"), c, K.DENSE, 0)
            assert k == labels.max() and np.array_equal(np.unique(labels[labels > 0]), np.arange(1, k + 1)) and np.array_equal(mask != 0, labels > 0)
