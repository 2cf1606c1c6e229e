"""ec_sharded_zonal_stats over an EC_GROUP_HOST_COMBINE group that lists device 0 once, twice and three times, with uneven shard
lengths — one of them 0.  Kind 0 equals the unsharded figures bit for bit (which tests/test_gpu_zonal.py holds to
tests/zonal_ref.py, and which are checked against it here too); kind 1 equals stats_ref.fold of the shards' own reference
records in shard order.  A refused call launches nothing."""
import ctypes as C

import numpy as np
import pytest

import stats_ref as R
import zonal_ref as Z
from test_gpu_composite_sharded import _scatter
from test_gpu_stats import NAMES, bits, random_cells, random_mask
from test_gpu_zonal import zone_ids

pytestmark = pytest.mark.gpu

LAYOUTS = ((2051,), (531, 1520), (2051, 0), (0, 2051), (700, 1, 1350))


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def same(got, want, ct, what):
    assert got.count == want["count"], what
    for name in ("sum", "mean", "stddev"):
        g, w = getattr(got, name), want[name]
        assert bits(g) == bits(w) or (np.isnan(g) and np.isnan(w)), (what, name, g, w)
    assert (R.order_key(ct, got.min.value.item()), R.order_key(ct, got.max.value.item())) == (R.order_key(ct, want["min"]), R.order_key(ct, want["max"])), what


@pytest.mark.parametrize("lens", LAYOUTS, ids=lambda t: "+".join(str(x) for x in t))
def test_sharded_zonal_stats(ec, lens):
    from erased_cells_hip.sharded import ShardGroup
    n, nz = sum(lens), 11
    cuts = np.concatenate([[0], np.cumsum(lens)])
    with ShardGroup([0] * len(lens), host_combine=len(lens) > 1) as g:
        made = []
        for ct, zt in ((R.I16, R.U8), (R.U32, R.I32), (R.F64, R.U16), (R.I64, R.U8)):
            cells, mask, zones = random_cells(ct, n, 0x5A0 + ct), random_mask(n, 0x5A1 + ct), zone_ids("runs37", n, nz + 2, zt)   # nz, nz + 1: foreign
            sb, sm, sz = _scatter(g, cells, lens, ct), _scatter(g, mask, lens, ec.UInt8), _scatter(g, zones, lens, zt)
            made += [sb, sm, sz]
            whole, wz = ec.CellBuffer.from_vec(cells), ec.CellBuffer.from_vec(zones)
            for mk, dm in ((None, None), (mask, sm)):
                got = g.zonal_stats(sb, sz, nz, dm)
                hm = None if mk is None else mk.tolist()
                parts = [Z.records(ct, cells[a:b].tolist(), zones[a:b].tolist(), nz, None if hm is None else hm[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
                assert len(got) == nz
                for z in range(nz):
                    what = (NAMES[ct], NAMES[zt], lens, "masked", mk is not None, "zone", z)
                    same(got[z], R.fold([p[z] for p in parts]), ct, what)   # the shards' records, in shard order
                if R.KIND[ct] == 0:   # exact integers: the cut does not matter — the unsharded figures bit for bit
                    one = (whole if mk is None else ec.MaskedCellBuffer(whole, ec.Mask.new(mk.astype(bool)))).zonal_stats(wz, nz)
                    want = Z.stats(ct, cells.tolist(), zones.tolist(), nz, hm)
                    for z in range(nz):
                        same(got[z], want[z], ct, ("against the whole raster", NAMES[ct], lens, z))
                        assert (got[z].count, bits(got[z].sum), bits(got[z].mean), bits(got[z].stddev)) == \
                            (one[z].count, bits(one[z].sum), bits(one[z].mean), bits(one[z].stddev))
        g.sync()
        for b in made:
            b.free()


def test_a_refused_call_launches_nothing(ec):
    from erased_cells_hip.sharded import ShardGroup
    L, E = ec.lib(), ec._ffi
    lens = (1000, 24)
    ct, zt, nz = R.I16, R.U8, 4
    cells, zones = random_cells(ct, sum(lens), 1), zone_ids("runs37", sum(lens), nz, zt)
    with ShardGroup([0, 0], host_combine=True) as g:
        sb, sz = _scatter(g, cells, lens, ct), _scatter(g, zones, lens, zt)
        n = (C.c_size_t * 2)(*lens)
        out = (E.EcStats * nz)()
        before = bytes(out)
        holed = (C.c_void_p * 2)(sb.ptrs[0], None)
        call = lambda t=ct, p=sb.ptrs, m=None, z_t=zt, z=sz.ptrs, nn=n, k=nz, o=out: L.ec_sharded_zonal_stats(g.handle, t, p, m, z_t, z, nn, k, o)
        allocs = C.c_int64()
        E.check(L.ec_stat_get(b"pool_allocs", C.byref(allocs)))
        refused = [(call(k=0), E.EC_ERR_ARG), (call(k=257), E.EC_ERR_ARG), (call(t=10), E.EC_ERR_UNSUPPORTED_TYPE), (call(z_t=R.U32), E.EC_ERR_UNSUPPORTED_TYPE),
                   (call(p=None), E.EC_ERR_ARG), (call(z=None), E.EC_ERR_ARG), (call(nn=None), E.EC_ERR_ARG), (call(o=None), E.EC_ERR_ARG),
                   (call(p=holed), E.EC_ERR_ARG), (call(z=holed), E.EC_ERR_ARG)]
        assert [st for st, _ in refused] == [e for _, e in refused]
        after = C.c_int64()
        E.check(L.ec_stat_get(b"pool_allocs", C.byref(after)))
        assert after.value == allocs.value and bytes(out) == before, "a refused call reached the pool or wrote its result"
        with pytest.raises(ec.EcError):
            g.zonal_stats(sb, sz, 0)
        with pytest.raises(ec.EcError):
            g.zonal_stats(sb, g.alloc(zt, (1000, 25)), nz)   # cut another way
        got = g.zonal_stats(sb, sz, nz)                       # the group is unharmed: the next call works
        want = Z.stats(ct, cells.tolist(), zones.tolist(), nz)
        assert [s.count for s in got] == [w["count"] for w in want] and [s.sum for s in got] == [w["sum"] for w in want]
        again = g.zonal_stats(sb, sz, np.int64(nz))           # a numpy K is taken as CellBuffer.zonal_stats and ShardGroup.zonal_table take it
        assert [(s.count, s.sum) for s in again] == [(s.count, s.sum) for s in got]
        sb.free()
        sz.free()
