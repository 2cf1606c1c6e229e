"""ec_sharded_reclass over an EC_GROUP_HOST_COMBINE group that lists device 0 once, twice and three times, with uneven shard
lengths — one of them 0: the gathered result equals the unsharded call bit for bit (which tests/test_gpu_reclass.py holds to
tests/reclass_ref.py, and which is checked against it here too).  A refused call posts nothing."""
import ctypes as C

import numpy as np
import pytest

import reclass_ref as Q
from test_gpu_composite_sharded import _scatter
from test_gpu_reclass import bits, class_values, some_valid
from vectors import rand_cells

pytestmark = pytest.mark.gpu

LAYOUTS = ((9001,), (4531, 4470), (9001, 0), (0, 9001), (4100, 1, 4900))


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


@pytest.mark.parametrize("lens", LAYOUTS, ids=lambda t: "+".join(str(x) for x in t))
def test_sharded_reclass(ec, lens):
    from erased_cells_hip.sharded import ShardGroup
    n = sum(lens)
    with ShardGroup([0] * len(lens), host_combine=len(lens) > 1) as g:
        made = []
        for k, (t, bt, dt, nb) in enumerate(((Q.U8, Q.F64, Q.U8, 5), (Q.U16, Q.U16, Q.I16, 255), (Q.F32, Q.F64, Q.U8, 9), (Q.I64, Q.U64, Q.F64, 40))):
            breaks = Q.gpu_tables(t, bt, nb, seed=k)
            x = Q.gpu_inputs(t, bt, breaks, n_random=n)[-n:]
            mask = Q.gpu_masks(n, seed=k)
            values, nodata = class_values(dt, breaks.size + 1, k)
            valid = some_valid(breaks.size + 1, k)
            sb, sm = _scatter(g, x, lens, t), _scatter(g, mask, lens, ec.UInt8)
            made += [sb, sm]
            # unmasked, no class dropped: one sharded buffer comes back
            plain = ec.ReclassTable(t, breaks, values, right=bool(k & 1))
            tabs = g.reclass_table(plain)
            out = g.reclassify(sb, tabs)
            want, _ = Q.reclass(t, x, None, bt, breaks, bool(k & 1), dt, values)
            got = g.gather(out)
            assert np.array_equal(bits(got), bits(want)), (Q.NAMES[t], lens)
            assert np.array_equal(bits(got), bits(ec.CellBuffer.from_vec(x).reclassify(plain).to_numpy())), "sharded and unsharded differ"
            # masked, with a dropped class, the table made by the call
            out2, om2 = g.reclassify(sb, breaks, values, right=bool(k & 1), valid=valid, mask=sm, nodata=nodata)
            want, want_ok = Q.reclass(t, x, mask, bt, breaks, bool(k & 1), dt, values, valid, nodata)
            assert np.array_equal(bits(g.gather(out2)), bits(want)) and np.array_equal(g.gather(om2), want_ok), (Q.NAMES[t], lens, "masked")
            made += [out, out2, om2, tabs]
        cls = g.classify(made[0], [10.5, 100.5])
        assert np.array_equal(g.gather(cls), np.digitize(g.gather(made[0]), [10.5, 100.5]).astype(np.uint8))
        made.append(cls)
        g.sync()
        for b in made:
            b.free()


def test_a_refusal_posts_nothing(ec):
    from erased_cells_hip.sharded import ShardGroup
    L, E = ec.lib(), ec._ffi
    lens = (5000, 24)
    x = rand_cells(Q.U16, sum(lens), 1)
    with ShardGroup([0, 0], host_combine=True) as g:
        sb = _scatter(g, x, lens, Q.U16)
        table = ec.ReclassTable(ec.UInt16, [100, 1000], np.array([7, 8, 9], np.uint8))
        tabs = g.reclass_table(table)
        out = _scatter(g, np.full(sum(lens), 0xEE, np.uint8), lens, Q.U8)
        n = (C.c_size_t * 2)(*lens)
        holed = (C.c_void_p * 2)(sb.ptrs[0], None)
        askew = (C.c_void_p * 2)(tabs.ptrs[0], tabs.ptrs[1] + 8)
        call = lambda t=Q.U16, p=sb.ptrs, m=None, nn=n, dt=Q.U8, tb=tabs.ptrs, d=out.ptrs, dm=None: L.ec_sharded_reclass(g.handle, t, p, m, nn, dt, tb, d, dm)
        refused = [(call(t=10), E.EC_ERR_UNSUPPORTED_TYPE), (call(dt=10), E.EC_ERR_UNSUPPORTED_TYPE), (call(p=None), E.EC_ERR_ARG), (call(nn=None), E.EC_ERR_ARG),
                   (call(tb=None), E.EC_ERR_ARG), (call(d=None), E.EC_ERR_ARG), (call(p=holed), E.EC_ERR_ARG), (call(tb=holed), E.EC_ERR_ARG),
                   (call(d=holed), E.EC_ERR_ARG), (call(m=holed), E.EC_ERR_ARG), (call(dm=holed), E.EC_ERR_ARG), (call(tb=askew), E.EC_ERR_ARG),
                   (call(d=sb.ptrs), E.EC_ERR_ARG)]
        assert [st for st, _ in refused] == [e for _, e in refused]
        g.sync()
        assert np.all(g.gather(out) == 0xEE), "a refused call wrote its output"
        assert call() == 0                                  # the group is unharmed: the next call works
        assert np.array_equal(g.gather(out), (np.digitize(x, [100, 1000]) + 7).astype(np.uint8))
        for b in (sb, tabs, out):
            b.free()
