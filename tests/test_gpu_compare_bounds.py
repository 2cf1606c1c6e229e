"""ec_compare, ec_compare_scalar, ec_select and ec_masked_select write exactly `n` cells of each output and nothing else —
wherever the output sits — and leave their operands alone: every call writes into guarded arenas (tests/arena.py), as
tests/test_gpu_output_bounds.py does for the other element-wise entry points.

Sizes are `sizes(T)` of that file — the base list and T - 1 .. 3 T + 7, each also one cell longer — for T = 256 x map_u x CPL
cells of each kernel (the family launches at map_u = 2 only; CPL = 16 / the widest cell).  One type pair per pair of byte
widths.  Mask and byte outputs at byte offsets 0, 1, 3, 8, 15, typed select outputs at cells 0, 1, 16 / W - 1, operands at cell
offsets 0 and 1.  With unaligned_vector = 0 every call with a pointer that is not 16-byte aligned takes the cell-wise kernel:
same cells, same guards.  Results are compare_ref's; the instantiations and the special values are covered by
tests/test_gpu_compare.py.  This file is about placement.
"""
import ctypes as C

import numpy as np
import pytest

import compare_ref as R
from arena import Arena, output
from test_gpu_output_bounds import BYTE_OFFS, IN_OFFS, WIDTH_PAIRS, Pool, sizes, size_of, typed_offs

pytestmark = pytest.mark.gpu

MAP_U = 2


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


@pytest.fixture(scope="module")
def pool(ec):
    return Pool(ec)


@pytest.fixture(scope="module")
def memo():
    return {}


@pytest.fixture(autouse=True)
def operands_stay_as_they_were(pool):
    yield
    pool.recheck()


def _seed(*parts):
    return hash(parts) & 0xFFFF


def _tile(widest):
    return 256 * MAP_U * (16 // widest)


UV = pytest.mark.parametrize("uv", [1, 0], ids=["vector", "cellwise-when-unaligned"])


@UV
def test_compare(ec, pool, memo, uv):
    """Unmasked, one mask, the other, both, in turn over the sizes; the operand masks share the operands' offset."""
    L, chk = ec.lib(), ec._ffi.check
    with ec.tuned(unaligned_vector=uv):
        for k, (w, (lt, rt)) in enumerate(WIDTH_PAIRS.items()):
            for io in IN_OFFS:
                (pl, hl), (pr, hr) = pool.get(lt, io), pool.get(rt, io, slot=1)
                (plm, hlm), (prm, hrm) = pool.mask(io, 0), pool.mask(io, 1)
                for mo in BYTE_OFFS:
                    for j, n in enumerate(sizes(_tile(max(w)))):
                        rel = R.RELS[(j + k) % 6]
                        a, ha, b, hb = [(None, None, None, None), (plm, hlm, None, None), (None, None, prm, hrm), (plm, hlm, prm, hrm)][(j + mo) % 4]
                        if ("cmp", lt, rt, rel) not in memo:
                            memo["cmp", lt, rt, rel] = R.relation(rel, lt, hl, rt, hr)
                        want = memo["cmp", lt, rt, rel][:n]
                        for hm in (ha, hb):
                            if hm is not None:
                                want = want & hm[:n]
                        out = output(ec, want, mo, _seed(lt, rt, n, mo))
                        chk(L.ec_compare(rel, lt, pl, a, rt, pr, b, n, out.ptr, ec.stream()))
                        out.check(want, f"ec_compare {R.NAMES[lt]} rel {rel} {R.NAMES[rt]} n {n} in +{io} cells, mask out +{mo} bytes, "
                                        f"masks {a is not None}/{b is not None}")


@UV
def test_compare_scalar(ec, pool, uv):
    L, chk = ec.lib(), ec._ffi.check
    cases = [(R.U8, R.I8, -3), (R.I16, R.U16, 40000), (R.F32, R.F64, 0.25), (R.U64, R.I64, 2**62), (R.I8, R.F64, 0.5)]   # CPL 16, 8, 4, 2, 16
    with ec.tuned(unaligned_vector=uv):
        for k, (ct, st, s) in enumerate(cases):
            v = ec.CellValue(st, s).to_ec()
            for io in IN_OFFS:
                p, h = pool.get(ct, io)
                pm, hm = pool.mask(io, 0)
                for mo in BYTE_OFFS:
                    for j, n in enumerate(sizes(_tile(size_of(ct)))):
                        rel = R.RELS[(j + k) % 6]
                        masked = (j + mo) % 2 == 1
                        want = R.relation(rel, ct, h[:n], st, R.NP[st].type(s))
                        want = want & hm[:n] if masked else want
                        out = output(ec, want, mo, _seed(ct, n, mo))
                        chk(L.ec_compare_scalar(rel, ct, p, pm if masked else None, n, C.byref(v), out.ptr, ec.stream()))
                        out.check(want, f"ec_compare_scalar {R.NAMES[ct]} rel {rel} {s} n {n} in +{io} mask out +{mo} masked {masked}")


SELECT_TYPES = (R.U8, R.I16, R.F32, R.U64)   # one per cell width


@UV
def test_select(ec, pool, uv):
    """ec_select, and ec_masked_select with `out` and `out_mask` each in an arena of its own, each offset on its own."""
    L, chk = ec.lib(), ec._ffi.check
    with ec.tuned(unaligned_vector=uv):
        for ct in SELECT_TYPES:
            w = size_of(ct)
            for io in IN_OFFS:
                (pa, ha), (pb, hb) = pool.get(ct, io), pool.get(ct, io, slot=1)
                (ps, hs), (pam, ham), (pbm, hbm) = pool.mask(io, 0), pool.mask(io, 1), pool.mask(io, 2)
                full, full_m = R.masked_select(hs, ha, ham, hb, hbm)
                for oo in typed_offs(w):
                    for j, n in enumerate(sizes(_tile(w))):
                        what = f"{R.NAMES[ct]} n {n} in +{io} out +{oo} cells"
                        out = output(ec, full[:n], oo, _seed(ct, n, oo))
                        chk(L.ec_select(ct, pa, pb, ps, n, out.ptr, ec.stream()))
                        out.check(full[:n], "ec_select " + what)
                        mo = BYTE_OFFS[(j + oo + io) % len(BYTE_OFFS)]
                        out, om = output(ec, full[:n], oo, _seed(ct, n, oo, 1)), output(ec, full_m[:n], mo, _seed(ct, n, mo, 2))
                        chk(L.ec_masked_select(ct, pa, pam, pb, pbm, ps, n, out.ptr, om.ptr, ec.stream()))
                        out.check(full[:n], "ec_masked_select " + what + ": values")
                        om.check(full_m[:n], "ec_masked_select " + what + f": mask +{mo} bytes")


def test_select_in_place(ec, pool):
    """The documented in-place patch: out == a and out == b, a window in the middle of an arena, the bytes in front of it and
    behind it kept; with unaligned_vector = 0 the odd offsets take the cell-wise kernel."""
    L, chk = ec.lib(), ec._ffi.check
    for uv in (1, 0):
        with ec.tuned(unaligned_vector=uv):
            for ct in SELECT_TYPES:
                w = size_of(ct)
                (pa, ha), (pb, hb) = pool.get(ct, 0), pool.get(ct, 0, slot=1)
                (ps, hs), (pam, ham), (pbm, hbm) = pool.mask(0, 0), pool.mask(0, 1), pool.mask(0, 2)
                full, full_m = R.masked_select(hs, ha, ham, hb, hbm)
                for oo in typed_offs(w):
                    for n in sizes(_tile(w)):
                        what = f"in place {R.NAMES[ct]} n {n} at +{oo} cells, unaligned_vector {uv}"
                        win = Arena(n * w, offset=oo * w, seed=_seed(ct, n, oo, 3), ec=ec).hold(ha[:n])   # out == a
                        chk(L.ec_select(ct, win.ptr, pb, ps, n, win.ptr, ec.stream()))
                        win.check(full[:n], "ec_select out == a " + what)
                        win = Arena(n * w, offset=oo * w, seed=_seed(ct, n, oo, 4), ec=ec).hold(hb[:n])   # out == b
                        chk(L.ec_select(ct, pa, win.ptr, ps, n, win.ptr, ec.stream()))
                        win.check(full[:n], "ec_select out == b " + what)
                    # the masked form at both aliases, values and mask in place, at the sizes around one tile
                    for n in sizes(_tile(w))[-10:]:
                        va = Arena(n * w, offset=oo * w, seed=_seed(ct, n, 5), ec=ec).hold(ha[:n])
                        ma = Arena(n, offset=oo, seed=_seed(ct, n, 6), ec=ec).hold(ham[:n])
                        chk(L.ec_masked_select(ct, va.ptr, ma.ptr, pb, pbm, ps, n, va.ptr, ma.ptr, ec.stream()))
                        va.check(full[:n], f"ec_masked_select out == a n {n}: values")
                        ma.check(full_m[:n], f"ec_masked_select out_mask == amask n {n}")
                        vb = Arena(n * w, offset=oo * w, seed=_seed(ct, n, 7), ec=ec).hold(hb[:n])
                        mb = Arena(n, offset=oo, seed=_seed(ct, n, 8), ec=ec).hold(hbm[:n])
                        chk(L.ec_masked_select(ct, pa, pam, vb.ptr, mb.ptr, ps, n, vb.ptr, mb.ptr, ec.stream()))
                        vb.check(full[:n], f"ec_masked_select out == b n {n}: values")
                        mb.check(full_m[:n], f"ec_masked_select out_mask == bmask n {n}")


def test_refused_calls_write_nothing(ec, pool):
    L, E = ec.lib(), ec._ffi
    n = 1000
    (pa, _), (pb, _) = pool.get(R.U16, 0), pool.get(R.U16, 0, slot=1)
    pm, _ = pool.mask(0, 0)
    v = ec.CellValue(ec.UInt16, 7).to_ec()
    bad_v = ec.CellValue(ec.UInt16, 7).to_ec()
    bad_v.dtype = 10
    out = Arena(2 * n, seed=1, ec=ec).hold(np.zeros(2 * n, np.uint8))
    om = Arena(n, seed=2, ec=ec).hold(np.zeros(n, np.uint8))
    s = ec.stream()
    refused = [
        (L.ec_compare(0, R.U16, pa, None, R.U16, pb, None, n, om.ptr, s), E.EC_ERR_ARG),
        (L.ec_compare(7, R.U16, pa, pm, R.U16, pb, pm, n, om.ptr, s), E.EC_ERR_ARG),
        (L.ec_compare(R.LT, 10, pa, None, R.U16, pb, None, n, om.ptr, s), E.EC_ERR_UNSUPPORTED_TYPE),
        (L.ec_compare(R.LT, R.U16, pa, None, 10, pb, None, n, om.ptr, s), E.EC_ERR_UNSUPPORTED_TYPE),
        (L.ec_compare(R.LT, R.U16, None, None, R.U16, pb, None, n, om.ptr, s), E.EC_ERR_ARG),
        (L.ec_compare(R.LT, R.U16, pa, None, R.U16, None, None, n, om.ptr, s), E.EC_ERR_ARG),
        (L.ec_compare_scalar(9, R.U16, pa, None, n, C.byref(v), om.ptr, s), E.EC_ERR_ARG),
        (L.ec_compare_scalar(R.GT, R.U16, pa, None, n, None, om.ptr, s), E.EC_ERR_ARG),
        (L.ec_compare_scalar(R.GT, R.U16, pa, None, n, C.byref(bad_v), om.ptr, s), E.EC_ERR_UNSUPPORTED_TYPE),
        (L.ec_compare_scalar(R.GT, R.U16, None, None, n, C.byref(v), om.ptr, s), E.EC_ERR_ARG),
        (L.ec_select(10, pa, pb, pm, n, out.ptr, s), E.EC_ERR_UNSUPPORTED_TYPE),
        (L.ec_select(R.U16, pa, None, pm, n, out.ptr, s), E.EC_ERR_ARG),
        (L.ec_select(R.U16, pa, pb, None, n, out.ptr, s), E.EC_ERR_ARG),
        (L.ec_masked_select(10, pa, pm, pb, pm, pm, n, out.ptr, om.ptr, s), E.EC_ERR_UNSUPPORTED_TYPE),
        (L.ec_masked_select(R.U16, pa, None, pb, pm, pm, n, out.ptr, om.ptr, s), E.EC_ERR_ARG),
        (L.ec_masked_select(R.U16, pa, pm, pb, None, pm, n, out.ptr, om.ptr, s), E.EC_ERR_ARG),
        (L.ec_masked_select(R.U16, pa, pm, pb, pm, None, n, out.ptr, om.ptr, s), E.EC_ERR_ARG),
    ]
    assert [st for st, _ in refused] == [e for _, e in refused]
    # n == 0 launches nothing
    assert L.ec_compare(R.LT, R.U16, pa, None, R.U16, pb, None, 0, om.ptr, s) == 0
    assert L.ec_compare_scalar(R.LT, R.U16, pa, None, 0, C.byref(v), om.ptr, s) == 0
    assert L.ec_select(R.U16, pa, pb, pm, 0, out.ptr, s) == 0 and L.ec_masked_select(R.U16, pa, pm, pb, pm, pm, 0, out.ptr, om.ptr, s) == 0
    out.check_unchanged("the values output of refused calls")
    om.check_unchanged("the mask output of refused calls")
