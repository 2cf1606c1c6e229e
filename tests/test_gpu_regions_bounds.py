"""ec_regions writes all of its output and nothing else — wherever it sits — keeps inside its workspace and leaves its inputs alone.

tests/test_gpu_regions.py is strict about values, but its outputs are fresh blocks of which only the payload is read back.  Here every
call goes through the C ABI with pointers into guarded arenas (tests/arena.py):

  * `dst`, `dst_mask`, the K word and the caller's workspace each sit in an arena of their own; the outputs are pre-filled with the
    complement of the expected result between random guards, `dst` at every residue mod 16 an int32 allows, `dst_mask` at EVERY byte
    offset 0 .. 15 behind a 256-byte boundary and K at both residues mod 16 a uint64 allows: exactly cols * rows labels, cols * rows
    mask bytes and eight bytes of K are written;
  * the workspace arena's payload is exactly ec_regions_workspace_bytes(cols, rows) bytes: its guards, compared byte for byte, show any
    parent, size or block sum outside it (the payload itself is scrap);
  * the cells and the source mask sit in operand arenas (the mask at an odd byte offset) that are compared byte for byte, guards
    included, at the end;
  * every shape of tests/regions_cases.py up to 2 TW + 1 by 2 TH + 1;
  * a refused call writes nothing: the arenas still hold their before-image.

The guards are the default 32 KiB: a whole tile's stores, TW x TH x 4 bytes of labels, cannot jump over them unseen (asserted below)."""
import numpy as np
import pytest

import regions_cases as K
from arena import GUARD, Arena, operand

pytestmark = pytest.mark.gpu

OK, UNSUPPORTED, ARG = 0, 2, 6
DTYPE = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.uint32): 2, np.dtype(np.uint64): 3, np.dtype(np.float32): 8}

assert GUARD >= K.TW * K.TH * 4 and GUARD >= 4 * 256 * 4    # one tile's labels; one workgroup's quads of the store kernel


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


# (connectivity, numbering, min_cells, dst?, dst_mask?, K?)
FORMS = [(4, K.DENSE, 0, True, True, True), (8, K.DENSE, 5, True, True, True), (8, K.ROOT, 2, True, False, False), (4, K.ROOT, 2, False, True, False),
         (4, K.DENSE, 2, False, False, True)]
FORM_IDS = ["dense-4", "dense-8-sieved", "root-8-labels-alone", "sieve-only", "k-alone"]


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_outputs_and_workspace_at_every_residue(ec, form):
    c, numbering, min_cells, values, want_mask, want_k = form
    L = ec.lib()
    patterns = ("random59", "checkerboard", "random3", "serpentine", "wide4", "none", "spiral", "wide8", "float-specials")
    for k, (cols, rows) in enumerate(K.SMALL):
        case = (cols, rows, patterns[k % len(patterns)], K.MASKS[k % 3])
        labels, mask, kept = K.expected(case, c, numbering, min_cells)
        kept = np.array([kept], np.uint64)
        cells, valid = K.cells(*case[:3]), K.valid(cols, rows, case[3])
        src = operand(ec, cells, offset_cells=k % 4, seed=k)
        smask = operand(ec, valid, offset_cells=1 + 2 * (k % 8), seed=50 + k) if valid is not None else None
        ws_bytes = L.ec_regions_workspace_bytes(cols, rows)
        ws = Arena(ws_bytes, GUARD, 0, 900 + k, ec).hold(np.zeros(ws_bytes, np.uint8))
        for off in range(16):
            dst = Arena(labels.nbytes, GUARD, off // 4 * 4, 7 * off + k, ec).expect(labels) if values else None
            dmask = Arena(mask.nbytes, GUARD, (5 * off + 3) % 16, 11 * off + k, ec).expect(mask) if want_mask else None
            kdev = Arena(8, GUARD, off // 8 * 8, 13 * off + k, ec).expect(kept) if want_k else None
            st = L.ec_regions(DTYPE[cells.dtype], src.ptr, smask.ptr if smask else None, cols, rows, c, numbering, min_cells, dst.ptr if values else None,
                              dmask.ptr if want_mask else None, kdev.ptr if want_k else None, ws.ptr, ec.stream())
            assert st == OK, L.ec_last_error_string()
            what = (FORM_IDS[FORMS.index(form)], case, off)
            if values:
                dst.check(labels, f"dst {what}")
            if want_mask:
                dmask.check(mask, f"dst_mask {what}")
            if want_k:
                kdev.check(kept, f"K {what}")
        image = ws.image()
        lo, hi = ws.lo, ws.lo + ws_bytes
        assert np.array_equal(image[:lo], ws.before[:lo]) and np.array_equal(image[hi:], ws.before[hi:]), f"a byte outside the workspace's {ws_bytes} changed {case}"
        src.check_unchanged(f"cells {case}")
        if smask is not None:
            smask.check_unchanged(f"src_mask {case}")


def test_a_refused_call_writes_nothing(ec):
    cols, rows = K.TW + 1, 3
    n = cols * rows
    L, s = ec.lib(), ec.stream()
    src = operand(ec, K.cells(cols, rows, "wide2"), offset_cells=1)
    smask = operand(ec, K.valid(cols, rows, "random10"), offset_cells=3)
    dst, dmask = Arena(4 * n, GUARD, 4, 1, ec).expect(np.zeros(n, np.int32)), Arena(n, GUARD, 3, 2, ec).expect(np.zeros(n, np.uint8))
    kdev = Arena(8, GUARD, 8, 4, ec).expect(np.zeros(1, np.uint64))
    ws_bytes = L.ec_regions_workspace_bytes(cols, rows)
    ws = Arena(ws_bytes, GUARD, 0, 3, ec).hold(np.zeros(ws_bytes, np.uint8))

    def call(t=1, src=src.ptr, sm=smask.ptr, cols=cols, rows=rows, c=4, numbering=K.DENSE, dst=dst.ptr, dm=dmask.ptr, k=kdev.ptr, w=ws.ptr):
        return L.ec_regions(t, src, sm, cols, rows, c, numbering, 2, dst, dm, k, w, s)

    refused = [call(cols=0), call(rows=0), call(cols=32769), call(rows=1 << 40), call(c=0), call(c=6), call(numbering=2), call(src=None, sm=None),
               call(dst=None, dm=None, k=None), call(src=src.ptr + 1), call(dst=dst.ptr + 2), call(k=kdev.ptr + 4), call(w=ws.ptr + 8), call(src=dst.ptr),
               call(dm=smask.ptr), call(sm=dmask.ptr), call(k=src.ptr + 6), call(dm=dst.ptr + 8), call(k=dst.ptr + 4), call(w=dst.ptr + 12),
               call(w=dmask.ptr - 19), call(sm=ws.ptr + 32), call(k=ws.ptr + 64)]
    assert refused == [ARG] * len(refused)
    assert call(t=10) == UNSUPPORTED and call(t=255) == UNSUPPORTED
    for arena in (dst, dmask, kdev, ws, src, smask):
        arena.check_unchanged("a refused call")
