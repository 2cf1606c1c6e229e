"""ec_distance on the device, bit for bit against tests/distance_ref.py (brute force over all targets, exact integers): both output
types, with and without dst_mask, and the mask-only form (dst NULL); every shape and pattern of tests/distance_cases.py — lines,
squares and oblongs around the lines per wave W and the staging tile side T, one 257 x 300, the long lines 1 x 32768, 32768 x 1 and
2 x 32768 — every max_sq of interest, odd byte offsets of mask and dst_mask, the same bytes from two calls and from the caller's and the
pooled workspace, and two cross-checks against an existing kernel (Mask.dilate).  No case is skipped or sampled: every cell of every
case is compared."""
import ctypes as C

import numpy as np
import pytest

import distance_cases as K
import distance_ref as R

pytestmark = pytest.mark.gpu

U32, F64 = R.U32, R.F64
NP = {U32: np.uint32, F64: np.float64}
BITS = {U32: np.uint32, F64: np.uint64}


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


def run(ec, m, max_sq, out_type, values=True, want_mask=True, workspace=False, mask_offset=0, dmask_offset=0):
    """one call -> (cell bits or None, mask bytes or None); the outputs are pre-filled with 0xA5 so that a cell never written shows"""
    rows, cols = m.shape
    n = cols * rows
    L = ec.lib()
    src = Dev(ec, n, mask_offset).put(m)
    dst = Dev(ec, n * np.dtype(NP[out_type]).itemsize).put(np.full(n * np.dtype(NP[out_type]).itemsize, 0xA5, np.uint8)) if values else None
    dmask = Dev(ec, n, dmask_offset).put(np.full(n, 0xA5, np.uint8)) if want_mask else None
    ws = Dev(ec, L.ec_distance_workspace_bytes(cols, rows)) if workspace else None
    st = L.ec_distance(src.ptr, cols, rows, max_sq, out_type, dst.ptr if dst else None, dmask.ptr if dmask else None, ws.ptr if ws else None, ec.stream())
    assert st == 0, L.ec_last_error_string()
    got = (dst.get(BITS[out_type]) if dst else None, dmask.get(np.uint8) if dmask else None)
    assert np.array_equal(src.get(np.uint8), m.ravel()), "the input mask changed"
    return got


def check(ec, case, max_sq, out_type, **form):
    cols, rows, pattern = case
    exp, ev = K.expected(cols, rows, pattern, max_sq, out_type)
    got, gv = run(ec, K.mask(cols, rows, pattern), max_sq, out_type, **form)
    what = (case, max_sq, out_type, form)
    if got is not None:
        bad = np.flatnonzero(got != exp.ravel().view(BITS[out_type]))
        assert bad.size == 0, (what, f"{bad.size} cells differ, first (y, x) = {divmod(int(bad[0]), cols)}: got {got[bad[0]]:#x}, expected {exp.ravel().view(BITS[out_type])[bad[0]]:#x}")
    if gv is not None:
        bad = np.flatnonzero(gv != ev.ravel())
        assert bad.size == 0, (what, f"{bad.size} mask bytes differ, first (y, x) = {divmod(int(bad[0]), cols)}: got {gv[bad[0]]}")


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_pattern_in_every_form(ec, shape):
    """u32 with its mask bytes, f64 without them, and the mask-only form under a limit that occurs"""
    for pattern in K.patterns_of(shape):
        case = shape + (pattern,)
        check(ec, case, K.UNLIMITED, U32)
        check(ec, case, K.UNLIMITED, F64, want_mask=False)
        check(ec, case, K.limits(*case)[3], U32, values=False)


LIMIT_SHAPES = [(1, 1), (K.T + 1, 1), (1, K.W + 1), (K.T + 1, 2 * K.W + 3), (2 * K.W + 3, K.T + 1), (2 * K.T + 1, 2 * K.T + 1)]


@pytest.mark.parametrize("shape", LIMIT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_limit(ec, shape):
    """max_sq in {0, 1, 2, a value that occurs, that value - 1, no limit}: values with zero bits outside it, with and without mask bytes"""
    for pattern in ("none", "all", "centre", "corner11", "diagonal", "random1", "random50"):
        case = shape + (pattern,)
        for max_sq in K.limits(*case):
            check(ec, case, max_sq, U32)
            check(ec, case, max_sq, F64)
            check(ec, case, max_sq, F64, want_mask=False)
            check(ec, case, max_sq, F64, values=False)


def test_odd_byte_offsets_of_mask_and_dst_mask(ec):
    for shape in ((K.T + 1, 5), (7, K.W + 1), (2 * K.T + 1, 3)):
        for k, (mo, do) in enumerate(((1, 0), (0, 1), (3, 7), (15, 9), (5, 5))):
            case = shape + (("random1", "checkerboard", "centre", "random50", "full-column")[k],)
            check(ec, case, K.UNLIMITED, F64, mask_offset=mo, dmask_offset=do)
            check(ec, case, 2, U32, mask_offset=mo, dmask_offset=do)
            check(ec, case, 5, U32, values=False, mask_offset=mo, dmask_offset=do)


def test_the_same_bytes_twice_and_from_either_workspace(ec):
    for case in ((2 * K.T + 1, K.W + 1, "random1"), (K.T - 1, 2 * K.W + 3, "random50"), (257, 300, "random001"), (32768, 2, "corner11")):
        m = K.mask(*case)
        for out_type in (U32, F64):
            first = run(ec, m, K.UNLIMITED, out_type)
            again = run(ec, m, K.UNLIMITED, out_type)
            own = run(ec, m, K.UNLIMITED, out_type, workspace=True)
            for other in (again, own):
                assert np.array_equal(first[0], other[0]) and np.array_equal(first[1], other[1]), (case, out_type)
            check(ec, case, K.UNLIMITED, out_type, workspace=True)


def test_against_dilate_and_the_mask_itself(ec):
    """an existing kernel as the witness: within d2 <= 2 is the 3 x 3 dilation (ec_focal MAX over the bytes), d2 <= 0 the mask as 0 / 1"""
    for case in ((K.T + 1, 2 * K.W + 3, "random1"), (2 * K.T + 1, K.W - 1, "diagonal"), (257, 300, "random001"), (K.T, 3, "checkerboard"), (1, K.W + 1, "centre"),
                 (K.T + 1, 1, "corner00")):
        cols, rows, _ = case
        m = K.mask(*case)
        mask = ec.Mask(m.size, ec.buffer._upload(m.ravel()))
        dilated = mask.dilate(cols, (1, 1)).to_numpy()
        assert np.array_equal(run(ec, m, 2, U32, values=False)[1], (dilated != 0).astype(np.uint8)), case
        assert np.array_equal(run(ec, m, 0, U32, values=False)[1], (m.ravel() != 0).astype(np.uint8)), case
