"""ec_sharded_zonal_table over an EC_GROUP_HOST_COMBINE group that lists device 0 once and three times, with uneven shard lengths
— one of them 0, a hole.  Kind 0 equals the unsharded figures bit for bit; kind 1 equals stats_ref.fold of the shards' own
reference records (tests/zonal_table_ref.py: each shard's truncated sums over its own cells and pivot) in shard order.  More than
256 zones throughout.  A refused call launches nothing."""
import ctypes as C

import numpy as np
import pytest

import stats_ref as R
import zonal_table_cases as K
import zonal_table_ref as ZT
from test_gpu_composite_sharded import _scatter
from test_gpu_stats import NAMES, NP, random_cells, random_mask
from test_gpu_zonal_table import assert_rows

pytestmark = pytest.mark.gpu

LAYOUTS = ((2051,), (700, 1, 1350), (2051, 0, 0), (531, 0, 1520))


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


@pytest.mark.parametrize("lens", LAYOUTS, ids=lambda t: "+".join(str(x) for x in t))
def test_sharded_zonal_table(ec, lens):
    from erased_cells_hip.sharded import ShardGroup
    n, nz = sum(lens), 300
    cuts = np.concatenate([[0], np.cumsum(lens)])
    with ShardGroup([0] * len(lens), host_combine=len(lens) > 1) as g:
        made = []
        for ct, zt in ((R.I16, R.U16), (R.U32, R.I32), (R.F64, R.U16), (R.I64, R.I32)):
            cells, mask, zones = random_cells(ct, n, 0x5A0 + ct), random_mask(n, 0x5A1 + ct), K.ids("runs37", n, nz + 2, zt)   # nz, nz + 1: foreign
            if ct == R.F64:
                cells = K.general_raster(n, 2, R.U8, seed=0x5A2)[0]
                cells[[3, 900]] = [2.0**75, -2.0**90]   # zones that truncate, in two shards
            sb, sm, sz = _scatter(g, cells, lens, ct), _scatter(g, mask, lens, ec.UInt8), _scatter(g, zones, lens, zt)
            made += [sb, sm, sz]
            whole, wz = ec.CellBuffer.from_vec(cells), ec.CellBuffer.from_vec(zones)
            for mk, dm in ((None, None), (mask, sm)):
                got = g.zonal_table(sb, sz, nz, dm)
                hm = None if mk is None else mk.tolist()
                parts = [ZT.records(ct, cells[a:b].tolist(), zones[a:b].tolist(), nz, None if hm is None else hm[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
                want = [R.fold([p[z] for p in parts]) for z in range(nz)]   # the shards' records, in shard order
                assert_rows(got, want, ct, (NAMES[ct], NAMES[zt], lens, "masked", mk is not None))
                if R.KIND[ct] == 0:   # exact integers: the cut does not matter — the unsharded figures bit for bit
                    one = (whole if mk is None else ec.MaskedCellBuffer(whole, ec.Mask.new(mk.astype(bool)))).zonal_table(wz, nz)
                    assert got.tobytes() == one.tobytes()
                    assert_rows(got, ZT.stats(ct, cells.tolist(), zones.tolist(), nz, hm), ct, ("against the whole raster", NAMES[ct], lens))
        g.sync()
        for b in made:
            b.free()


def test_a_refused_call_launches_nothing(ec):
    from erased_cells_hip.sharded import ShardGroup
    L, E = ec.lib(), ec._ffi
    lens = (1000, 24)
    ct, zt, nz = R.I16, R.U16, 400
    cells, zones = random_cells(ct, sum(lens), 1), K.ids("runs37", sum(lens), nz, zt)
    with ShardGroup([0, 0], host_combine=True) as g:
        sb, sz = _scatter(g, cells, lens, ct), _scatter(g, zones, lens, zt)
        n = (C.c_size_t * 2)(*lens)
        out = (E.EcStats * nz)()
        before = bytes(out)
        holed = (C.c_void_p * 2)(sb.ptrs[0], None)
        call = lambda t=ct, p=sb.ptrs, m=None, z_t=zt, z=sz.ptrs, nn=n, k=nz, o=out: L.ec_sharded_zonal_table(g.handle, t, p, m, z_t, z, nn, k, o)
        allocs = C.c_int64()
        E.check(L.ec_stat_get(b"pool_allocs", C.byref(allocs)))
        refused = [(call(k=0), E.EC_ERR_ARG), (call(k=2**24 + 1), E.EC_ERR_ARG), (call(t=10), E.EC_ERR_UNSUPPORTED_TYPE), (call(z_t=R.U32), E.EC_ERR_UNSUPPORTED_TYPE),
                   (call(p=None), E.EC_ERR_ARG), (call(z=None), E.EC_ERR_ARG), (call(nn=None), E.EC_ERR_ARG), (call(o=None), E.EC_ERR_ARG),
                   (call(p=holed), E.EC_ERR_ARG), (call(z=holed), E.EC_ERR_ARG)]
        assert [st for st, _ in refused] == [e for _, e in refused]
        after = C.c_int64()
        E.check(L.ec_stat_get(b"pool_allocs", C.byref(after)))
        assert after.value == allocs.value and bytes(out) == before, "a refused call reached the pool or wrote its result"
        with pytest.raises(ec.EcError):
            g.zonal_table(sb, sz, 0)
        with pytest.raises(ec.EcError):
            g.zonal_table(sb, g.alloc(zt, (1000, 25)), nz)   # cut another way
        got = g.zonal_table(sb, sz, np.int64(nz))             # the group is unharmed: the next call works; a numpy K is taken as CellBuffer.zonal_table takes it
        want = ZT.stats(ct, cells.tolist(), zones.tolist(), nz)
        assert got["count"].tolist() == [w["count"] for w in want] and got["sum"].tolist() == [w["sum"] for w in want]
        sb.free()
        sz.free()
