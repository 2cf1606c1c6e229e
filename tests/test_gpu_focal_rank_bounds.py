"""ec_focal_rank / ec_focal_majority write all of their output and nothing else — wherever it sits — and leave their inputs alone.

tests/test_gpu_focal_rank.py is strict about values, but its outputs are fresh 256-byte-aligned blocks of which only [0, n) is read
back.  Here every call goes through the C ABI with pointers into guarded arenas (tests/arena.py), as tests/test_gpu_focal_bounds.py does
for ec_focal:

  * `dst` and `dst_mask` each sit in an arena of their own, pre-filled with the complement of the expected result between random
    guards, at EVERY byte offset 0 .. 15 behind a 256-byte boundary (the mask at another one: offset 5 k mod 16 beside k), so the
    16-byte slot stores and the 16 / W-byte mask stores start on every residue: exactly cols * rows cells and mask bytes are written;
  * `src` and `src_mask` sit in operand arenas (at cell offsets 0 and 1) that are compared byte for byte, guards included, at the end;
  * both settings of "unaligned_vector" run: with 0 a slot that can start off a 16-byte boundary is stored cell by cell, and the sweep
    asserts from the pointers that it has made both kinds of launch;
  * shapes around one tile (TW x TH) and around one 16-byte slot;
  * a refused call writes nothing: the arenas still hold their before-image.

The guards are the default 32 KiB: more than a whole tile's stores, TW * TH * 8 = 8 KiB of 8-byte results and 1 KiB of mask bytes, so a
workgroup that stores its tile at a wrong place cannot jump over them unseen (asserted below)."""
import numpy as np
import pytest

import focal_rank_cases as K
import focal_rank_ref as R
from arena import GUARD, Arena, operand

pytestmark = pytest.mark.gpu

OK, UNSUPPORTED, ARG = 0, 2, 6
WHOLE = 1
ARMS = [dict(), dict(unaligned_vector=0)]
ARM_IDS = ["default", "cellwise-when-unaligned"]
SHAPES = [(K.TW, K.TH), (K.TW + 1, K.TH + 1), (K.TW - 1, 3), (17, 2), (16, 1), (15, 2), (1, 1), (2 * K.TW + 3, 2), (32, 3)]
# (cell type number, q or None for the majority, flags, source mask?, dst_mask?, radius): every cell width, so every slot and mask-store width
KINDS = [(0, (1, 2, K.LOWER), 0, True, True, (1, 1)), (0, None, 0, False, False, (2, 2)), (5, (1, 2, K.UPPER), 0, True, True, (2, 1)),
         (8, (9, 10, K.UPPER), WHOLE, False, True, (1, 3)), (9, None, 0, True, True, (1, 1)), (3, (1, 2, K.LOWER), 0, False, False, (3, 4)),
         (7, None, WHOLE, True, True, (7, 1))]
KIND_IDS = ["u8-median-masked", "u8-majority", "i16-upper-median-masked", "f32-q90-whole", "f64-majority-masked", "u64-median-7x9", "i64-majority-whole-masked"]

assert GUARD > K.TW * K.TH * 8 and GUARD > K.TW * K.TH   # one tile's 8-byte results, one tile's mask bytes


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def call(ec, ct, q, flags, radius, src, smask, cols, rows, dst, dmask):
    L = ec.lib()
    if q is None:
        return L.ec_focal_majority(ct, src, smask, cols, rows, radius[0], radius[1], flags, dst, dmask, ec.stream())
    return L.ec_focal_rank(ct, src, smask, cols, rows, radius[0], radius[1], q[0], q[1], q[2], flags, dst, dmask, ec.stream())


@pytest.mark.parametrize("arm", ARMS, ids=ARM_IDS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_output_at_every_byte_offset(ec, kind, arm):
    ct, q, flags, masked, want_mask, radius = kind
    cellwise = vector = 0
    with ec.tuned(**arm):
        for k, (cols, rows) in enumerate(SHAPES):
            a = K.class_raster(ct, cols, rows, 0xB0 + ct + k) if q is None else K.rank_raster(ct, cols, rows, 0xB0 + ct + k)
            m = K.mask_bytes("hashed", cols, rows, 0xB1 + k) if masked else None
            od = R.ordered(a, m, *radius)
            exp, ev = R.majority_pick(od, bool(flags), a.dtype) if q is None else R.pick(od, q[0], q[1], q[2], bool(flags), a.dtype)
            src = operand(ec, a, offset_cells=k % 2, seed=k)
            smask = operand(ec, m, offset_cells=(k + 1) % 2, seed=k + 100) if masked else None
            for off in range(16):
                moff = (5 * off) % 16
                dst = Arena(exp.nbytes, GUARD, off, 7 * off + k, ec).expect(exp)
                dmask = Arena(ev.nbytes, GUARD, moff, 11 * off + k, ec).expect(ev) if want_mask else None
                st = call(ec, ct, q, flags, radius, src.ptr, smask.ptr if masked else None, cols, rows, dst.ptr, dmask.ptr if want_mask else None)
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
    a = K.rank_raster(1, cols, rows, 0xBAD)
    m = K.mask_bytes("hashed", cols, rows, 0xBAE)
    src, smask = operand(ec, a), operand(ec, m)
    zeros, zmask = np.zeros(cols * rows, np.uint16), np.zeros(cols * rows, np.uint8)
    dst, dmask = Arena(zeros.nbytes, GUARD, 8, 1, ec).expect(zeros), Arena(zmask.nbytes, GUARD, 3, 2, ec).expect(zmask)
    L, s = ec.lib(), ec.stream()

    def rank(t=1, src=src.ptr, sm=smask.ptr, cols=cols, rows=rows, rx=1, ry=1, num=1, den=2, method=0, flags=0, dst=dst.ptr, dm=dmask.ptr):
        return L.ec_focal_rank(t, src, sm, cols, rows, rx, ry, num, den, method, flags, dst, dm, s)

    def majority(t=1, src=src.ptr, sm=smask.ptr, cols=cols, rows=rows, rx=1, ry=1, flags=0, dst=dst.ptr, dm=dmask.ptr):
        return L.ec_focal_majority(t, src, sm, cols, rows, rx, ry, flags, dst, dm, s)

    shared = [dict(src=None), dict(dst=None), dict(flags=2), dict(flags=4), dict(rx=8), dict(ry=8), dict(rx=4, ry=4), dict(rx=7, ry=2),
              dict(dm=None), dict(sm=None, flags=WHOLE, dm=None), dict(cols=1 << 33, rows=1 << 31), dict(cols=K.TW << 31, rows=1),
              dict(src=dst.ptr), dict(sm=dmask.ptr)]
    refused = [f(**kw) for kw in shared for f in (rank, majority)]
    refused += [rank(den=0), rank(den=65536), rank(num=3, den=2), rank(method=2), rank(method=-1)]
    assert refused == [ARG] * len(refused)
    assert rank(t=10) == UNSUPPORTED and majority(t=255) == UNSUPPORTED
    assert rank(cols=0) == OK and majority(rows=0) == OK       # nothing to do
    for arena in (dst, dmask, src, smask):
        arena.check_unchanged("a refused call")
