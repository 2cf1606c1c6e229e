"""ec_cast and ec_cast_scaled write exactly `n` cells of `dst` and nothing else — wherever `dst` sits — and leave their operands
alone: every call writes into guarded arenas (tests/arena.py), as tests/test_gpu_output_bounds.py does for the other
element-wise entry points.  These are the kernels whose stored stream can be narrower than the loaded one, so the (source
width, destination width) combination decides how many bytes a lane stores: one type pair for each of the 16.

Sizes are `sizes(T)` of that file — the base list and T - 1 .. 3 T + 7, each also one cell longer — for T = 256 x map_u x CPL
cells (the family launches at map_u = 2 only; CPL = 16 / the widest cell of the pair).  Inputs at cell offsets 0 and 1, outputs
at cells 0, 1, 16 / W - 1 of the destination's width, masks at byte offsets 0, 1, 3, 8, 15.  With unaligned_vector = 0 every call
with a pointer that is not aligned takes the cell-wise kernel: same cells, same guards.  Results are cast_ref's; the special
values and all 100 pairs are covered by tests/test_gpu_cast.py.  This file is about placement.
"""
import ctypes as C

import numpy as np
import pytest

import cast_ref as R
from arena import Arena, output
from test_gpu_output_bounds import BYTE_OFFS, IN_OFFS, Pool, sizes, typed_offs

pytestmark = pytest.mark.gpu

MAP_U = 2
# one pair per (source width, destination width); none fits (a fitting pair is ec_convert's kernel, tests/test_gpu_output_bounds.py),
# and a float destination has an integer source, so that no NaN's payload is in question
PAIRS = {(1, 1): (R.I8, R.U8), (1, 2): (R.I8, R.U16), (1, 4): (R.I8, R.U32), (1, 8): (R.I8, R.U64),
         (2, 1): (R.U16, R.I8), (2, 2): (R.U16, R.I16), (2, 4): (R.I16, R.U32), (2, 8): (R.I16, R.U64),
         (4, 1): (R.F32, R.U8), (4, 2): (R.I32, R.I16), (4, 4): (R.U32, R.F32), (4, 8): (R.F32, R.I64),
         (8, 1): (R.F64, R.U8), (8, 2): (R.F64, R.I16), (8, 4): (R.I64, R.F32), (8, 8): (R.F64, R.U64)}


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


def test_the_pairs_are_what_they_claim():
    for (ws, wd), (st, dt) in PAIRS.items():
        assert (R.NP[st].itemsize, R.NP[dt].itemsize) == (ws, wd) and not R.can_fit_into(st, dt)
        assert R.is_int(st) or R.is_int(dt)
    assert len(PAIRS) == 16


UV = pytest.mark.parametrize("uv", [1, 0], ids=["vector", "cellwise-when-unaligned"])


@UV
def test_cast(ec, pool, memo, uv):
    L, chk = ec.lib(), ec._ffi.check
    with ec.tuned(unaligned_vector=uv):
        for (ws, wd), (st, dt) in PAIRS.items():
            for io in IN_OFFS:
                p, h = pool.get(st, io)
                for oo in typed_offs(wd):
                    for j, n in enumerate(sizes(_tile(max(ws, wd)))):
                        mode = (j + oo + io) % 2
                        if (st, dt, mode) not in memo:
                            memo[st, dt, mode] = R.cast(mode, st, h, dt)
                        want = memo[st, dt, mode][:n]
                        out = output(ec, want, oo, _seed(st, dt, n, oo))
                        chk(L.ec_cast(mode, st, p, dt, out.ptr, n, ec.stream()))
                        out.check(want, f"ec_cast mode {mode} {R.NAMES[st]} -> {R.NAMES[dt]} n {n} in +{io} out +{oo} cells")


@UV
def test_cast_scaled(ec, pool, memo, uv):
    """Unmasked and masked in turn over the sizes; the mask at a byte offset of its own."""
    L, chk = ec.lib(), ec._ffi.check
    scale, offset = 0.001, 3.5
    with ec.tuned(unaligned_vector=uv):
        for k, ((ws, wd), (st, dt)) in enumerate(PAIRS.items()):
            nd = R.nodata_of(dt)
            v = ec.CellValue(dt, nd).to_ec()
            for io in IN_OFFS:
                p, h = pool.get(st, io)
                for oo in typed_offs(wd):
                    mo = BYTE_OFFS[(k + oo + io) % len(BYTE_OFFS)]
                    pm, hm = pool.mask(mo, 0)
                    if ("scaled", st, dt) not in memo:
                        with np.errstate(all="ignore"):
                            plain = R.scaled(st, h, None, scale, offset, dt)
                        assert R.is_int(dt) or not np.isnan(plain).any()   # the arenas compare bytes: no NaN's payload may be in question
                        memo["scaled", st, dt] = (plain, np.where(hm.astype(bool), plain, nd))
                    plain, masked_want = memo["scaled", st, dt]
                    for j, n in enumerate(sizes(_tile(max(ws, wd)))):
                        masked = (j + oo) % 2 == 1
                        want = (masked_want if masked else plain)[:n]
                        out = output(ec, want, oo, _seed(st, dt, n, oo, 1))
                        chk(L.ec_cast_scaled(st, p, pm if masked else None, n, scale, offset, dt, C.byref(v) if masked else None, out.ptr, ec.stream()))
                        out.check(want, f"ec_cast_scaled {R.NAMES[st]} -> {R.NAMES[dt]} n {n} in +{io} out +{oo} cells, mask +{mo} bytes, masked {masked}")


def test_refused_calls_write_nothing(ec, pool):
    L, E = ec.lib(), ec._ffi
    n = 1000
    p, _ = pool.get(R.F64, 0)
    pm, _ = pool.mask(0, 0)
    nd16, nd32 = ec.CellValue(ec.Int16, -9999).to_ec(), ec.CellValue(ec.Int32, -9999).to_ec()
    out = Arena(2 * n, seed=1, ec=ec).hold(np.zeros(2 * n, np.uint8))
    s = ec.stream()
    refused = [
        (L.ec_cast(2, R.F64, p, R.I16, out.ptr, n, s), E.EC_ERR_ARG),
        (L.ec_cast(-1, R.F64, p, R.I16, out.ptr, n, s), E.EC_ERR_ARG),
        (L.ec_cast(R.ROUND, 10, p, R.I16, out.ptr, n, s), E.EC_ERR_UNSUPPORTED_TYPE),
        (L.ec_cast(R.ROUND, R.F64, p, 10, out.ptr, n, s), E.EC_ERR_UNSUPPORTED_TYPE),
        (L.ec_cast(R.ROUND, R.F64, None, R.I16, out.ptr, n, s), E.EC_ERR_ARG),
        (L.ec_cast_scaled(R.F64, p, pm, n, 1.0, 0.0, R.I16, None, out.ptr, s), E.EC_ERR_ARG),
        (L.ec_cast_scaled(R.F64, p, None, n, 1.0, 0.0, R.I16, C.byref(nd16), out.ptr, s), E.EC_ERR_ARG),
        (L.ec_cast_scaled(R.F64, p, pm, n, 1.0, 0.0, R.I16, C.byref(nd32), out.ptr, s), E.EC_ERR_ARG),
        (L.ec_cast_scaled(R.F64, p, pm, n, float("nan"), 0.0, R.I16, C.byref(nd16), out.ptr, s), E.EC_ERR_ARG),
        (L.ec_cast_scaled(R.F64, p, pm, n, 1.0, float("-inf"), R.I16, C.byref(nd16), out.ptr, s), E.EC_ERR_ARG),
        (L.ec_cast_scaled(10, p, None, n, 1.0, 0.0, R.I16, None, out.ptr, s), E.EC_ERR_UNSUPPORTED_TYPE),
        (L.ec_cast_scaled(R.F64, None, None, n, 1.0, 0.0, R.I16, None, out.ptr, s), E.EC_ERR_ARG),
    ]
    assert [st for st, _ in refused] == [e for _, e in refused]
    # n == 0 launches nothing
    assert L.ec_cast(R.AS, R.F64, p, R.I16, out.ptr, 0, s) == 0 and L.ec_cast_scaled(R.F64, p, pm, 0, 1.0, 0.0, R.I16, C.byref(nd16), out.ptr, s) == 0
    out.check_unchanged("the output of refused calls")
