"""ec_focal / ec_focal_convolve write all of their output and nothing else — wherever it sits — and leave their inputs alone.

tests/test_gpu_focal.py is strict about values, but its outputs are fresh 256-byte-aligned blocks of which only [0, n) is read back.
Here every call goes through the C ABI with pointers into guarded arenas (tests/arena.py):

  * `dst` and `dst_mask` each sit in an arena of their own, pre-filled with the complement of the expected result between random
    guards, at EVERY byte offset 0 .. 15 behind a 256-byte boundary (the mask at another one: offset 5 k mod 16 beside k), so the
    16-byte slot stores and the 16 / W-byte mask stores start on every residue;
  * `src` and `src_mask` sit in operand arenas (at cell offsets 0 and 1) that are compared byte for byte, guards included, at the end;
  * both settings of "unaligned_vector" run: with 0 a slot that can start off a 16-byte boundary is stored cell by cell
    (`cellwise_stores`, ec_focal.hip), and the sweep asserts from the pointers that it has made both kinds of launch;
  * shapes around one tile (TW x TH) and around one 16-byte slot;
  * a refused call writes nothing: the arenas still hold their before-image.

The guards are the default 32 KiB: more than a whole tile's stores, TW * TH * 8 = 8 KiB of f64 results and 1 KiB of mask bytes, so a
workgroup that stores its tile at a wrong place cannot jump over them unseen (asserted below)."""
import ctypes as C

import numpy as np
import pytest

import focal_cases as K
import focal_ref as R
from arena import GUARD, Arena, operand

pytestmark = pytest.mark.gpu

OK, ARG = 0, 6
WHOLE, NORMALIZE = 1, 2
ARMS = [dict(), dict(unaligned_vector=0)]
ARM_IDS = ["default", "cellwise-when-unaligned"]
SHAPES = [(K.TW, K.TH), (K.TW + 1, K.TH + 1), (K.TW - 1, 3), (17, 2), (16, 1), (15, 2), (1, 1), (2 * K.TW + 3, 2), (32, 3)]
# (cell type number, what, flags, source mask?, dst_mask?, radius)
KINDS = [(0, R.MAX, 0, True, True, (1, 1)), (5, R.SUM, 0, True, True, (2, 1)), (8, R.MIN, WHOLE, False, True, (1, 3)),
         (9, "convolve", NORMALIZE, True, True, (1, 1)), (3, R.MEAN, 0, False, False, (7, 7)), (7, "convolve", 0, False, False, (2, 1)),
         (5, R.MIN, 0, True, True, (2, 1))]   # 2-byte results: 8 cells per slot and the 8-byte mask store beside it
KIND_IDS = ["u8-max-masked", "i16-sum-masked", "f32-min-whole", "f64-convolve-normalize-masked", "u64-mean", "i64-convolve", "i16-min-masked"]

assert GUARD > K.TW * K.TH * 8 and GUARD > K.TW * K.TH   # one tile's f64 results, one tile's mask bytes


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def call(ec, ct, what, flags, radius, src, smask, cols, rows, dst, dmask):
    L = ec.lib()
    if what == "convolve":
        w = np.ascontiguousarray(K.weights(*radius))
        return L.ec_focal_convolve(ct, src, smask, cols, rows, w.ctypes.data_as(C.POINTER(C.c_double)), radius[0], radius[1], flags, dst, dmask, ec.stream())
    return L.ec_focal(what, ct, src, smask, cols, rows, radius[0], radius[1], flags, dst, dmask, ec.stream())


@pytest.mark.parametrize("arm", ARMS, ids=ARM_IDS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_output_at_every_byte_offset(ec, kind, arm):
    ct, what, flags, masked, want_mask, radius = kind
    cellwise = vector = 0
    with ec.tuned(**arm):
        for k, (cols, rows) in enumerate(SHAPES):
            a = K.raster_cells(ct, cols, rows, 0xB0 + ct + k)
            m = K.mask_bytes("hashed", cols, rows, 0xB1 + k) if masked else None
            if what == "convolve":
                exp, ev = R.convolve(a, m, K.weights(*radius), bool(flags & NORMALIZE), bool(flags & WHOLE))
            else:
                exp, ev = R.focal(what, a, m, radius[0], radius[1], bool(flags & WHOLE))
            src = operand(ec, a, offset_cells=k % 2, seed=k)
            smask = operand(ec, m, offset_cells=(k + 1) % 2, seed=k + 100) if masked else None
            for off in range(16):
                moff = (5 * off) % 16
                dst = Arena(exp.nbytes, GUARD, off, 7 * off + k, ec).expect(exp)
                dmask = Arena(ev.nbytes, GUARD, moff, 11 * off + k, ec).expect(ev) if want_mask else None
                st = call(ec, ct, what, flags, radius, src.ptr, smask.ptr if masked else None, cols, rows, dst.ptr, dmask.ptr if want_mask else None)
                assert st == OK, ec.lib().ec_last_error_string()
                case = (KIND_IDS[KINDS.index(kind)], cols, rows, off, moff)
                dst.check(exp, f"dst {case}")
                if want_mask:
                    dmask.check(ev, f"dst_mask {case}")
                aligned = dst.ptr % 16 == 0 and (dmask is None or dmask.ptr % 16 == 0) and cols % 16 == 0
                if arm and not aligned:
                    cellwise += 1
                else:
                    vector += 1
            src.check_unchanged(f"src {cols} x {rows}")
            if masked:
                smask.check_unchanged(f"src_mask {cols} x {rows}")
    assert vector > 0 and (cellwise > 0) == bool(arm)


def test_a_refused_call_writes_nothing(ec):
    cols, rows = K.TW + 1, 3
    a = K.raster_cells(1, cols, rows, 0xBAD)
    m = K.mask_bytes("hashed", cols, rows, 0xBAE)
    src, smask = operand(ec, a), operand(ec, m)
    zeros, zmask = np.zeros(cols * rows, np.float64), np.zeros(cols * rows, np.uint8)
    dst, dmask = Arena(zeros.nbytes, GUARD, 8, 1, ec).expect(zeros), Arena(zmask.nbytes, GUARD, 3, 2, ec).expect(zmask)
    L, s = ec.lib(), ec.stream()
    w = np.ascontiguousarray(K.weights(1, 1))
    wp = w.ctypes.data_as(C.POINTER(C.c_double))
    refused = [
        L.ec_focal(4, 1, src.ptr, smask.ptr, cols, rows, 1, 1, 0, dst.ptr, dmask.ptr, s),            # no such operation
        L.ec_focal(0, 1, src.ptr, smask.ptr, cols, rows, 1, 1, 4, dst.ptr, dmask.ptr, s),            # unknown flag
        L.ec_focal(0, 1, src.ptr, smask.ptr, cols, rows, 1, 1, NORMALIZE, dst.ptr, dmask.ptr, s),    # convolve's flag
        L.ec_focal(0, 1, src.ptr, smask.ptr, cols, rows, 8, 1, 0, dst.ptr, dmask.ptr, s),            # radius above the cap
        L.ec_focal(0, 1, src.ptr, smask.ptr, cols, rows, 1, 1, 0, dst.ptr, None, s),                 # dst_mask required
        L.ec_focal(0, 1, src.ptr, None, cols, rows, 1, 1, WHOLE, dst.ptr, None, s),
        L.ec_focal(0, 1, src.ptr, smask.ptr, 1 << 33, 1 << 31, 1, 1, 0, dst.ptr, dmask.ptr, s),      # cols * rows
        L.ec_focal(0, 1, src.ptr, smask.ptr, K.TW << 31, 1, 1, 1, 0, dst.ptr, dmask.ptr, s),         # tiles
        L.ec_focal(0, 1, dst.ptr, smask.ptr, cols, rows, 1, 1, 0, dst.ptr, dmask.ptr, s),            # in place
        L.ec_focal(0, 1, src.ptr, dmask.ptr, cols, rows, 1, 1, 0, dst.ptr, dmask.ptr, s),
        L.ec_focal(0, 1, None, smask.ptr, cols, rows, 1, 1, 0, dst.ptr, dmask.ptr, s),
        L.ec_focal_convolve(1, src.ptr, smask.ptr, cols, rows, None, 1, 1, 0, dst.ptr, dmask.ptr, s),
        L.ec_focal_convolve(1, src.ptr, smask.ptr, cols, rows, wp, 1, 8, 0, dst.ptr, dmask.ptr, s),
        L.ec_focal_convolve(1, src.ptr, smask.ptr, cols, rows, wp, 1, 1, 8, dst.ptr, dmask.ptr, s),
    ]
    assert refused == [ARG] * len(refused)
    assert L.ec_focal(0, 10, src.ptr, smask.ptr, cols, rows, 1, 1, 0, dst.ptr, dmask.ptr, s) == 2   # EC_ERR_UNSUPPORTED_TYPE
    assert L.ec_focal_convolve(255, src.ptr, smask.ptr, cols, rows, wp, 1, 1, 0, dst.ptr, dmask.ptr, s) == 2
    assert L.ec_focal(0, 1, src.ptr, smask.ptr, 0, rows, 1, 1, 0, dst.ptr, dmask.ptr, s) == OK       # nothing to do
    for arena in (dst, dmask, src, smask):
        arena.check_unchanged("a refused call")
