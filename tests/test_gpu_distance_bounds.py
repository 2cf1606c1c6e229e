"""ec_distance writes all of its output and nothing else — wherever it sits — keeps inside its workspace and leaves its input alone.

tests/test_gpu_distance.py is strict about values, but its outputs are fresh blocks of which only the payload is read back.  Here every
call goes through the C ABI with pointers into guarded arenas (tests/arena.py):

  * `dst`, `dst_mask` and the caller's workspace each sit in an arena of their own; the two outputs are pre-filled with the complement
    of the expected result between random guards, `dst` at every residue mod 16 its cell type allows and `dst_mask` at EVERY byte offset
    0 .. 15 behind a 256-byte boundary: exactly cols * rows cells and mask bytes are written;
  * the workspace arena's payload is exactly ec_distance_workspace_bytes(cols, rows) bytes: its guards, compared byte for byte, show any
    g cell or stack entry outside it (the payload itself is scrap);
  * the input mask sits in an operand arena (at an odd byte offset) that is compared byte for byte, guards included, at the end;
  * every shape of tests/distance_cases.py up to 2T + 1 a side;
  * a refused call writes nothing: the arenas still hold their before-image.

The guards are the default 32 KiB: a whole result tile's stores, W x T x 8 bytes of f64 and W x T mask bytes, cannot jump over them
unseen (asserted below)."""
import numpy as np
import pytest

import distance_cases as K
import distance_ref as R
from arena import GUARD, Arena, operand

pytestmark = pytest.mark.gpu

OK, UNSUPPORTED, ARG = 0, 2, 6
U32, F64 = R.U32, R.F64

assert GUARD >= K.W * K.T * 8 and GUARD > K.W * K.T   # one tile's f64 results, one tile's mask bytes


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


# (out_type, dst?, dst_mask?, max_sq or None for a value that occurs)
FORMS = [(U32, True, True, K.UNLIMITED), (F64, True, True, None), (F64, True, False, 2), (U32, True, False, None), (F64, False, True, None)]
FORM_IDS = ["u32-masked", "f64-masked-limited", "f64-within-2", "u32-limited", "mask-only"]


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_outputs_and_workspace_at_every_residue(ec, form):
    out_type, values, want_mask, limit = form
    L = ec.lib()
    cell = 4 if out_type == U32 else 8
    patterns = ("random1", "checkerboard", "centre", "none", "corner11", "random50", "diagonal")
    for k, (cols, rows) in enumerate(K.SMALL):
        pattern = patterns[k % len(patterns)]
        max_sq = K.limits(cols, rows, pattern)[3] if limit is None else limit
        exp, ev = K.expected(cols, rows, pattern, max_sq, out_type)
        src = operand(ec, K.mask(cols, rows, pattern), offset_cells=1 + 2 * (k % 8), seed=k)
        ws_bytes = L.ec_distance_workspace_bytes(cols, rows)
        ws = Arena(ws_bytes, GUARD, 0, 900 + k, ec).hold(np.zeros(ws_bytes, np.uint8))
        for off in range(16):
            dst = Arena(exp.nbytes, GUARD, off // cell * cell, 7 * off + k, ec).expect(exp) if values else None
            dmask = Arena(ev.nbytes, GUARD, (5 * off + 3) % 16, 11 * off + k, ec).expect(ev) if want_mask else None
            st = L.ec_distance(src.ptr, cols, rows, max_sq, out_type, dst.ptr if values else None, dmask.ptr if want_mask else None, ws.ptr, ec.stream())
            assert st == OK, L.ec_last_error_string()
            case = (FORM_IDS[FORMS.index(form)], cols, rows, pattern, off)
            if values:
                dst.check(exp, f"dst {case}")
            if want_mask:
                dmask.check(ev, f"dst_mask {case}")
        image = ws.image()
        lo, hi = ws.lo, ws.lo + ws_bytes
        assert np.array_equal(image[:lo], ws.before[:lo]) and np.array_equal(image[hi:], ws.before[hi:]), f"a byte outside the workspace's {ws_bytes} changed {(cols, rows, pattern)}"
        src.check_unchanged(f"mask {cols} x {rows}")


def test_a_refused_call_writes_nothing(ec):
    cols, rows = K.T + 1, 3
    n = cols * rows
    m = K.mask(cols, rows, "random50")
    L, s = ec.lib(), ec.stream()
    src = operand(ec, m, offset_cells=1)
    zeros, zmask = np.zeros(n, np.float64), np.zeros(n, np.uint8)
    dst, dmask = Arena(zeros.nbytes, GUARD, 8, 1, ec).expect(zeros), Arena(n, GUARD, 3, 2, ec).expect(zmask)
    ws_bytes = L.ec_distance_workspace_bytes(cols, rows)
    ws = Arena(ws_bytes, GUARD, 0, 3, ec).hold(np.zeros(ws_bytes, np.uint8))

    def call(mask=src.ptr, cols=cols, rows=rows, out_type=F64, dst=dst.ptr, dm=dmask.ptr, w=ws.ptr):
        return L.ec_distance(mask, cols, rows, 5, out_type, dst, dm, w, s)

    refused = [call(cols=0), call(rows=0), call(cols=32769), call(rows=1 << 40), call(out_type=0), call(out_type=8), call(mask=None),
               call(dst=None, dm=None), call(dst=dst.ptr + 4), call(out_type=U32, dst=dst.ptr + 2), call(mask=dst.ptr), call(dm=src.ptr),
               call(mask=dmask.ptr), call(dm=dst.ptr + 8), call(w=dst.ptr + 16), call(w=dmask.ptr - 16), call(mask=ws.ptr + 32)]
    assert refused == [ARG] * len(refused)
    assert call(out_type=10) == UNSUPPORTED and call(out_type=255) == UNSUPPORTED
    for arena in (dst, dmask, ws, src):
        arena.check_unchanged("a refused call")
