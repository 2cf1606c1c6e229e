"""ec_composite_rank writes all of its output and nothing else — wherever it sits — and leaves its inputs alone.

tests/test_gpu_composite_rank.py is strict about values, but its outputs are fresh 256-byte-aligned blocks of which only [0, n) is
read back.  Here every call goes through the C ABI with pointers into guarded arenas (tests/arena.py):

  * `dst`, `dst_mask` and `aux` each sit in an arena of their own, pre-filled with the complement of the expected result between
    random guards; `dst` starts on every cell-aligned residue mod 16 behind a 256-byte boundary, `dst_mask` and `aux` on every
    residue (5 k and 11 k mod 16 beside k), so the group-wide value, mask and aux stores start everywhere;
  * the layers and their masks sit in operand arenas (at cell offsets 0 and 1, by turns) that are compared byte for byte, guards included;
  * both settings of "unaligned_vector" run: with 0 a launch with a pointer off its group's alignment runs the cell-wise kernel, and
    the sweep asserts from the pointers that it has made both kinds of launch;
  * every size around one group and around one tile, for buckets whose groups are 16 bytes, narrower, and a single cell;
  * a refused call writes nothing: the arenas still hold their before-image.

The guards are the default 32 KiB: more than a whole tile's stores (256 lanes x 16 B = 4 KiB of values), so a workgroup that stores
its tile at a wrong place cannot jump over them unseen (asserted below)."""
import ctypes as C

import numpy as np
import pytest

import composite_rank_ref as R
from arena import GUARD, Arena, operand

pytestmark = pytest.mark.gpu

OK, UNSUPPORTED, ARG = 0, 2, 6
ARMS = [dict(), dict(unaligned_vector=0)]
ARM_IDS = ["default", "cellwise-when-unaligned"]
# (cell type, mask form, layers, (num, den, method), min_count)
KINDS = [(R.CR.U8, "all", 5, (1, 2, R.LOWER), 1), (R.CR.I16, "some", 9, (1, 2, R.UPPER), 2), (R.CR.F32, "all", 4, (9, 10, R.LOWER), 4),
         (R.CR.U64, "none", 3, (1, 4, R.UPPER), 1), (R.CR.U16, "all", 33, (1, 2, R.LOWER), 2), (R.CR.F64, "some", 17, (1, 1, R.LOWER), 1),
         (R.CR.I8, "none", 2, (0, 1, R.UPPER), 2)]
KIND_IDS = ["u8-median", "i16-upper-some-null", "f32-and-rule", "u64-unmasked", "u16-33-layers", "f64-17-layers-some-null", "i8-unmasked"]

assert all(GUARD > R.tile_cells(ct, k) * R.NP[ct].itemsize for ct, _, k, _, _ in KINDS)
assert len({R.group_cells(ct, k) * R.NP[ct].itemsize for ct, _, k, _, _ in KINDS}) >= 3        # groups of several widths,
assert {R.group_cells(ct, k) for ct, _, k, _, _ in KINDS} >= {1, 2, 16}                         # single cells and whole 16-byte groups among them


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def sizes(ct, k):
    c, t = R.group_cells(ct, k), R.tile_cells(ct, k)
    return sorted({1, c - 1, c, c + 1, 2 * c + 1, t - 1, t, t + 1, t + c + 1} - {0})


def ptrs(arenas):
    return (C.c_void_p * len(arenas))(*[None if a is None else a.ptr for a in arenas])


@pytest.mark.parametrize("arm", ARMS, ids=ARM_IDS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_output_at_every_offset(ec, kind, arm):
    ct, form, k, (num, den, method), mc = kind
    L = ec.lib()
    dt = R.NP[ct]
    cellwise = vector = 0
    with ec.tuned(**arm):
        for j, n in enumerate(sizes(ct, k)):
            layers, masks = R.stack(ct, k, n, form, seed=10 + j)
            exp, em, ea = R.composite_rank(ct, layers, masks, num, den, method, mc)
            la = [operand(ec, a, offset_cells=j % 2, seed=i) for i, a in enumerate(layers)]
            ma = [None] * k if masks is None else [None if m is None else operand(ec, m, offset_cells=j % 2, seed=100 + i) for i, m in enumerate(masks)]
            masked = any(m is not None for m in ma)
            for off in range(0, 16, max(dt.itemsize, 2)):
                moff, aoff = (5 * off + j) % 16, (11 * off + 3 * j) % 16   # all zero for the first size at offset 0: one aligned launch
                dst = Arena(exp.nbytes, GUARD, off, 7 * off + j, ec).expect(exp)
                dmask = Arena(em.nbytes, GUARD, moff, 11 * off + j, ec).expect(em) if (masked or off % 4) else None   # asked for or not, when free
                aux = Arena(ea.nbytes, GUARD, aoff, 13 * off + j, ec).expect(ea) if (off // max(dt.itemsize, 2)) % 3 != 2 else None
                st = L.ec_composite_rank(ct, ptrs(la), ptrs(ma) if masked else None, k, n, num, den, method, mc, dst.ptr,
                                         dmask.ptr if dmask else None, aux.ptr if aux else None, ec.stream())
                assert st == OK, L.ec_last_error_string()
                case = (KIND_IDS[KINDS.index(kind)], n, off, moff, aoff)
                dst.check(exp, f"dst {case}")
                if dmask:
                    dmask.check(em, f"dst_mask {case}")
                if aux:
                    aux.check(ea, f"aux {case}")
                c = R.group_cells(ct, k)
                aligned = (dst.ptr % (c * dt.itemsize) == 0 and all(a.ptr % (c * dt.itemsize) == 0 for a in la) and
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
    # a group of one cell is aligned wherever a cell is: that bucket never needs the cell-wise kernel
    assert vector > 0 and (cellwise > 0) == (bool(arm) and R.group_cells(ct, k) > 1)


def test_a_refused_call_writes_nothing(ec):
    ct, k, n = R.CR.U16, 3, 1000
    layers, masks = R.stack(ct, k, n, "all", seed=20)
    la, ma = [operand(ec, a, seed=i) for i, a in enumerate(layers)], [operand(ec, m, seed=50 + i) for i, m in enumerate(masks)]
    zeros, zbytes = np.zeros(n, np.uint16), np.zeros(n, np.uint8)
    dst, dmask, aux = (Arena(zeros.nbytes, GUARD, 8, 1, ec).expect(zeros), Arena(n, GUARD, 3, 2, ec).expect(zbytes), Arena(n, GUARD, 5, 3, ec).expect(zbytes))
    L, s = ec.lib(), ec.stream()
    lp, mp = ptrs(la), ptrs(ma)
    holed = ptrs([la[0], None, la[2]])
    with_dst, with_dmask = ptrs([la[0], dst, la[2]]), ptrs([ma[0], ma[1], dmask])
    sixty_five = (C.c_void_p * 65)(*([la[0].ptr] * 65))
    call = lambda t=ct, l=lp, m=mp, kk=k, nn=n, num=1, den=2, method=0, mc=1, d=dst.ptr, dm=dmask.ptr, a=aux.ptr: \
        L.ec_composite_rank(t, l, m, kk, nn, num, den, method, mc, d, dm, a, s)
    refused = [
        call(kk=0), call(l=sixty_five, m=None, kk=65),                   # the layer count
        call(den=0), call(den=65536), call(num=3, den=2),                # q
        call(method=2), call(method=-1),                                 # the method
        call(mc=0), call(mc=k + 1),                                      # min_count
        call(l=None), call(l=holed), call(d=None),                       # null pointers
        call(dm=None),                                                   # dst_mask required
        call(nn=1 << 62),                                                # tiles
        call(l=with_dst),                                                # dst is a layer
        call(m=with_dmask),                                              # dst_mask is a mask
        call(a=ma[1].ptr),                                               # aux is a mask
        call(dm=dst.ptr), call(a=dst.ptr), call(a=dmask.ptr),            # outputs equal to each other
    ]
    assert refused == [ARG] * len(refused)
    assert call(t=10) == UNSUPPORTED and call(t=255) == UNSUPPORTED
    assert call(nn=0) == OK    # nothing to do
    for arena in [dst, dmask, aux] + la + ma:
        arena.check_unchanged("a refused call")
