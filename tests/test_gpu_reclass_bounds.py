"""ec_reclass writes exactly `n` cells of dst and — when asked — `n` bytes of dst_mask and nothing else, wherever they sit, and
leaves the raster, its mask and the table alone: every call writes into guarded arenas (tests/arena.py), as
tests/test_gpu_compare_bounds.py does for its family.

Sizes are `sizes(T)` of tests/test_gpu_output_bounds.py — the base list and T - 1 .. 3 T + 7, each also one cell longer — for
T = 256 x 2 x CPL cells (the family launches at map_u = 2 only; CPL = 16 / the wider of the two cells).  One (t, dt) per pair of
byte widths.  Typed outputs at cells 0, 1, 16 / W - 1, mask outputs at byte offsets 0, 1, 3, 8, 15, the raster and its mask at
cell offsets 0 and 1.  With unaligned_vector = 0 every call with a pointer that is not vector-aligned takes the cell-wise kernel:
same cells, same guards.  Results are reclass_ref's; this file is about placement."""
import numpy as np
import pytest

import reclass_ref as Q
from arena import Arena, operand, output
from test_gpu_output_bounds import BYTE_OFFS, IN_OFFS, WIDTH_PAIRS, Pool, sizes, typed_offs
from test_gpu_reclass import class_values, some_valid

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


@pytest.fixture(scope="module")
def pool(ec):
    return Pool(ec)


@pytest.fixture(autouse=True)
def operands_stay_as_they_were(pool):
    yield
    pool.recheck()


def _seed(*parts):
    return hash(parts) & 0xFFFF


def _table(ec, t, dt, h, masked, seed):
    """a table whose breaks are cells of the raster itself (ties), in a guarded arena of its own -> (arena, breaks, values, valid, nodata)"""
    nb = (3, 40, 255)[seed % 3]
    with np.errstate(all="ignore"):
        cand = h[:4000][~np.isnan(h[:4000])] if Q.NP[t].kind == "f" else h[:4000]
    key = Q.order_key(t, cand)
    breaks = cand[np.unique(key, return_index=True)[1]]
    breaks = breaks[np.linspace(0, breaks.size - 1, min(nb, breaks.size)).astype(np.int64)]
    values, nodata = class_values(dt, breaks.size + 1, seed)
    valid = some_valid(breaks.size + 1, seed)
    tab = ec.ReclassTable(t, breaks, values, right=bool(seed & 1), valid=valid, nodata=nodata if masked else None)
    return operand(ec, np.frombuffer(tab.bytes(), np.uint8), 0, seed=seed + 5), breaks, values, valid, nodata


@pytest.mark.parametrize("uv", [1, 0], ids=["vector", "cellwise-when-unaligned"])
def test_reclass_writes_its_n_cells_and_nothing_else(ec, pool, uv):
    L, chk = ec.lib(), ec._ffi.check
    tables = []
    with ec.tuned(unaligned_vector=uv):
        for k, ((wt, wd), (t, dt)) in enumerate(WIDTH_PAIRS.items()):
            for io in IN_OFFS:
                p, h = pool.get(t, io)
                pm, hm = pool.mask(io, 0)
                for masked in (False, True):
                    tab, breaks, values, valid, nodata = _table(ec, t, dt, h, masked, k + io)
                    tables.append(tab)
                    full, full_ok = Q.reclass(t, h, hm if masked else None, t, breaks, bool((k + io) & 1), dt, values, valid, nodata if masked else None)
                    for oo in typed_offs(wd):
                        for j, n in enumerate(sizes(Q.tile(t, dt))):
                            mo = BYTE_OFFS[(j + oo + io) % len(BYTE_OFFS)]
                            what = f"ec_reclass {Q.NAMES[t]} -> {Q.NAMES[dt]} n {n} in +{io} out +{oo} cells, mask out +{mo} bytes, masked {masked}, unaligned_vector {uv}"
                            out, om = output(ec, full[:n], oo, _seed(t, dt, n, oo)), output(ec, full_ok[:n], mo, _seed(t, dt, n, mo, 1))
                            chk(L.ec_reclass(t, p, pm if masked else None, n, dt, tab.ptr, out.ptr, om.ptr, ec.stream()))
                            out.check(full[:n], what + ": values")
                            om.check(full_ok[:n], what + ": dst_mask")
    for tab in tables:
        tab.check_unchanged("the table")


def test_without_a_dst_mask_only_dst_is_written(ec, pool):
    L, chk = ec.lib(), ec._ffi.check
    for (wt, wd), (t, dt) in list(WIDTH_PAIRS.items())[::3]:
        p, h = pool.get(t, 1)
        tab = ec.ReclassTable(t, np.sort(h[:4000][~np.isnan(h[:4000].astype(np.float64))])[[10, 2000, 3900]], class_values(dt, 4, 1)[0])
        dev = operand(ec, np.frombuffer(tab.bytes(), np.uint8), 0, seed=9)
        for n in sizes(Q.tile(t, dt))[-6:]:
            full = Q.kernel_model(None, Q.parse(tab.bytes()), t, h[:n], None, dt)[0]
            out = output(ec, full, 1, _seed(t, n))
            chk(L.ec_reclass(t, p, None, n, dt, dev.ptr, out.ptr, None, ec.stream()))
            out.check(full, f"ec_reclass without dst_mask {Q.NAMES[t]} -> {Q.NAMES[dt]} n {n}")
        dev.check_unchanged("the table")


def test_refused_calls_write_nothing(ec, pool):
    L, E = ec.lib(), ec._ffi
    n = 1000
    p, h = pool.get(Q.U16, 0)
    pm, _ = pool.mask(0, 0)
    tab = ec.ReclassTable(ec.UInt16, [100, 1000], np.array([0, 1, 2], np.uint8))
    dev = operand(ec, np.frombuffer(tab.bytes(), np.uint8), 0, seed=3)
    out = Arena(n, seed=1, ec=ec).hold(np.zeros(n, np.uint8))
    om = Arena(n, seed=2, ec=ec).hold(np.zeros(n, np.uint8))
    s = ec.stream()
    refused = [
        (L.ec_reclass(10, p, None, n, Q.U8, dev.ptr, out.ptr, om.ptr, s), E.EC_ERR_UNSUPPORTED_TYPE),
        (L.ec_reclass(Q.U16, p, None, n, 10, dev.ptr, out.ptr, om.ptr, s), E.EC_ERR_UNSUPPORTED_TYPE),
        (L.ec_reclass(Q.U16, None, None, n, Q.U8, dev.ptr, out.ptr, om.ptr, s), E.EC_ERR_ARG),
        (L.ec_reclass(Q.U16, p, None, n, Q.U8, None, out.ptr, om.ptr, s), E.EC_ERR_ARG),
        (L.ec_reclass(Q.U16, p, None, n, Q.U8, dev.ptr, None, om.ptr, s), E.EC_ERR_ARG),
        (L.ec_reclass(Q.U16, p, None, n, Q.U8, dev.ptr + 8, out.ptr, om.ptr, s), E.EC_ERR_ARG),
        (L.ec_reclass(Q.U16, p, None, n, Q.U8, dev.ptr, out.ptr, out.ptr + n - 1, s), E.EC_ERR_ARG),
        (L.ec_reclass(Q.U16, p, pm, n, Q.U8, dev.ptr, out.ptr, pm, s), E.EC_ERR_ARG),
        (L.ec_reclass(Q.U16, out.ptr, None, n // 2, Q.U8, dev.ptr, out.ptr + 1, om.ptr, s), E.EC_ERR_ARG),
    ]
    assert [st for st, _ in refused] == [e for _, e in refused]
    assert L.ec_reclass(Q.U16, p, None, 0, Q.U8, dev.ptr, out.ptr, om.ptr, s) == 0   # n == 0 launches nothing
    out.check_unchanged("the values output of refused calls")
    om.check_unchanged("the mask output of refused calls")
    dev.check_unchanged("the table")
