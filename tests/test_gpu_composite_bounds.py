"""ec_composite writes all of its output and nothing else — wherever it sits — and leaves its inputs alone.

tests/test_gpu_composite.py is strict about values, but its outputs are fresh 256-byte-aligned blocks of which only [0, n) is read
back.  Here every call goes through the C ABI with pointers into guarded arenas (tests/arena.py):

  * `dst`, `dst_mask` and `aux` each sit in an arena of their own, pre-filled with the complement of the expected result between
    random guards; `dst` starts on every cell-aligned residue mod 16 behind a 256-byte boundary, `dst_mask` and `aux` on every
    residue (5 k and 11 k mod 16 beside k), so the 16-byte value stores and the CPL-byte mask and aux stores start everywhere;
  * the layers and their masks sit in operand arenas (at cell offsets 0 and 1, by turns) that are compared byte for byte, guards included;
  * both settings of "unaligned_vector" run: with 0 a launch with a pointer off its group's alignment runs the cell-wise kernel, and
    the sweep asserts from the pointers that it has made both kinds of launch;
  * every size around one group (CPL cells) and around one tile;
  * a refused call writes nothing: the arenas still hold their before-image.

The guards are the default 32 KiB: more than a whole tile's stores (256 lanes x 2 groups x 16 B = 8 KiB of values), so a workgroup
that stores its tile at a wrong place cannot jump over them unseen (asserted below)."""
import ctypes as C

import numpy as np
import pytest

import composite_ref as R
from arena import GUARD, Arena, operand

pytestmark = pytest.mark.gpu

OK, UNSUPPORTED, ARG = 0, 2, 6
ARMS = [dict(), dict(unaligned_vector=0)]
ARM_IDS = ["default", "cellwise-when-unaligned"]
# (cell type, op, mask form, layers, min_count)
KINDS = [(R.U8, R.FIRST, "all", 5, 1), (R.I16, R.MAX, "some", 9, 2), (R.F32, R.MIN, "all", 4, 4), (R.U64, R.LAST, "none", 3, 1),
         (R.U16, R.MEAN, "all", 8, 2), (R.F64, R.SUM, "some", 7, 1), (R.I8, R.SUM, "none", 2, 2)]
KIND_IDS = ["u8-first", "i16-max-some-null", "f32-min-and-rule", "u64-last-unmasked", "u16-mean", "f64-sum-some-null", "i8-sum-unmasked"]

assert all(GUARD > R.tile_cells(op, ct) * R.NP[R.result_type(op, ct)].itemsize for ct, op, _, _, _ in KINDS)


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def sizes(op, ct):
    c, t = R.cpl(op, ct), R.tile_cells(op, ct)
    return sorted({1, c - 1, c, c + 1, 2 * c + 1, t - 1, t, t + 1, t + c + 1} - {0})


def ptrs(arenas):
    return (C.c_void_p * len(arenas))(*[None if a is None else a.ptr for a in arenas])


@pytest.mark.parametrize("arm", ARMS, ids=ARM_IDS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_output_at_every_offset(ec, kind, arm):
    ct, op, form, k, mc = kind
    L = ec.lib()
    rt = R.NP[R.result_type(op, ct)]
    cellwise = vector = 0
    with ec.tuned(**arm):
        for j, n in enumerate(sizes(op, ct)):
            layers, masks = R.stack(ct, k, n, form, seed=10 + j)
            exp, em, ea = R.composite(op, ct, layers, masks, mc)
            la = [operand(ec, a, offset_cells=j % 2, seed=i) for i, a in enumerate(layers)]
            ma = [None] * k if masks is None else [None if m is None else operand(ec, m, offset_cells=j % 2, seed=100 + i) for i, m in enumerate(masks)]
            masked = any(m is not None for m in ma)
            for off in range(0, 16, rt.itemsize):
                moff, aoff = (5 * off + j) % 16, (11 * off + 3 * j) % 16   # all zero for the first size at offset 0: one aligned launch
                dst = Arena(exp.nbytes, GUARD, off, 7 * off + j, ec).expect(exp)
                dmask = Arena(em.nbytes, GUARD, moff, 11 * off + j, ec).expect(em) if (masked or off % 2) else None   # asked for or not, when free
                aux = Arena(ea.nbytes, GUARD, aoff, 13 * off + j, ec).expect(ea) if (off // rt.itemsize) % 3 != 2 else None
                st = L.ec_composite(op, ct, ptrs(la), ptrs(ma) if masked else None, k, n, mc, dst.ptr, dmask.ptr if dmask else None,
                                    aux.ptr if aux else None, ec.stream())
                assert st == OK, L.ec_last_error_string()
                case = (KIND_IDS[KINDS.index(kind)], n, off, moff, aoff)
                dst.check(exp, f"dst {case}")
                if dmask:
                    dmask.check(em, f"dst_mask {case}")
                if aux:
                    aux.check(ea, f"aux {case}")
                c = R.cpl(op, ct)
                aligned = (dst.ptr % 16 == 0 and all(a.ptr % (c * R.NP[ct].itemsize) == 0 for a in la) and
                           all(a is None or a.ptr % c == 0 for a in ma + [dmask, aux]))
                if arm and not aligned:
                    cellwise += 1
                else:
                    vector += 1
            for i, a in enumerate(la):
                a.check_unchanged(f"layer {i}, n = {n}")
            for i, a in enumerate(ma):
                if a is not None:
                    a.check_unchanged(f"mask {i}, n = {n}")
    assert vector > 0 and (cellwise > 0) == bool(arm)


def test_a_refused_call_writes_nothing(ec):
    ct, k, n = R.U16, 3, 1000
    layers, masks = R.stack(ct, k, n, "all", seed=20)
    la, ma = [operand(ec, a, seed=i) for i, a in enumerate(layers)], [operand(ec, m, seed=50 + i) for i, m in enumerate(masks)]
    zeros, zbytes = np.zeros(n, np.float64), np.zeros(n, np.uint8)
    dst, dmask, aux = (Arena(zeros.nbytes, GUARD, 8, 1, ec).expect(zeros), Arena(n, GUARD, 3, 2, ec).expect(zbytes), Arena(n, GUARD, 5, 3, ec).expect(zbytes))
    L, s = ec.lib(), ec.stream()
    lp, mp = ptrs(la), ptrs(ma)
    holed = ptrs([la[0], None, la[2]])
    with_dst, with_dmask = ptrs([la[0], dst, la[2]]), ptrs([ma[0], ma[1], dmask])
    sixty_five = (C.c_void_p * 65)(*([la[0].ptr] * 65))
    refused = [
        L.ec_composite(6, ct, lp, mp, k, n, 1, dst.ptr, dmask.ptr, aux.ptr, s),            # no such operation
        L.ec_composite(-1, ct, lp, mp, k, n, 1, dst.ptr, dmask.ptr, aux.ptr, s),
        L.ec_composite(0, ct, lp, mp, 0, n, 1, dst.ptr, dmask.ptr, aux.ptr, s),            # the layer count
        L.ec_composite(0, ct, sixty_five, None, 65, n, 1, dst.ptr, dmask.ptr, aux.ptr, s),
        L.ec_composite(0, ct, lp, mp, k, n, 0, dst.ptr, dmask.ptr, aux.ptr, s),            # min_count
        L.ec_composite(0, ct, lp, mp, k, n, k + 1, dst.ptr, dmask.ptr, aux.ptr, s),
        L.ec_composite(0, ct, None, mp, k, n, 1, dst.ptr, dmask.ptr, aux.ptr, s),          # null pointers
        L.ec_composite(0, ct, holed, mp, k, n, 1, dst.ptr, dmask.ptr, aux.ptr, s),
        L.ec_composite(0, ct, lp, mp, k, n, 1, None, dmask.ptr, aux.ptr, s),
        L.ec_composite(0, ct, lp, mp, k, n, 1, dst.ptr, None, aux.ptr, s),                 # dst_mask required
        L.ec_composite(4, ct, lp, mp, k, 1 << 62, 1, dst.ptr, dmask.ptr, aux.ptr, s),      # tiles
        L.ec_composite(0, ct, with_dst, mp, k, n, 1, dst.ptr, dmask.ptr, aux.ptr, s),      # dst is a layer
        L.ec_composite(0, ct, lp, with_dmask, k, n, 1, dst.ptr, dmask.ptr, aux.ptr, s),    # dst_mask is a mask
        L.ec_composite(0, ct, lp, mp, k, n, 1, dst.ptr, dmask.ptr, ma[1].ptr, s),          # aux is a mask
        L.ec_composite(0, ct, lp, mp, k, n, 1, dst.ptr, dst.ptr, aux.ptr, s),              # outputs equal to each other
        L.ec_composite(0, ct, lp, mp, k, n, 1, dst.ptr, dmask.ptr, dst.ptr, s),
        L.ec_composite(0, ct, lp, mp, k, n, 1, dst.ptr, dmask.ptr, dmask.ptr, s),
    ]
    assert refused == [ARG] * len(refused)
    assert L.ec_composite(0, 10, lp, mp, k, n, 1, dst.ptr, dmask.ptr, aux.ptr, s) == UNSUPPORTED
    assert L.ec_composite(5, 255, lp, mp, k, n, 1, dst.ptr, dmask.ptr, aux.ptr, s) == UNSUPPORTED
    assert L.ec_composite(0, ct, lp, mp, k, 0, 1, dst.ptr, dmask.ptr, aux.ptr, s) == OK    # nothing to do
    for arena in [dst, dmask, aux] + la + ma:
        arena.check_unchanged("a refused call")
