"""ec_sharded_cast / ec_sharded_cast_scaled over an EC_GROUP_HOST_COMBINE group that lists device 0 twice, with uneven shard
lengths — one of them 0: the gathered result equals the unsharded one (which tests/test_gpu_cast.py holds to tests/cast_ref.py,
and which is checked against it here too), and a refused call posts nothing."""
import ctypes as C

import numpy as np
import pytest

import cast_ref as R

pytestmark = pytest.mark.gpu

LAYOUTS = ((531, 1520), (2051, 0), (0, 2051))   # 2051 = cast_ref.gpu_len(Float64, UInt8)


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def _scatter(g, a, lens, ct):
    """`a` cut into shards of the given lengths (ShardGroup.scatter cuts by rows)."""
    a = np.ascontiguousarray(a)
    sb = g.alloc(ct, lens)
    sz = a.dtype.itemsize
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]) * sz
    n = len(lens)
    from erased_cells_hip._ffi import check, lib
    check(lib().ec_sharded_upload(g.handle, sb.ptrs, a.ctypes.data_as(C.c_void_p), (C.c_size_t * n)(*[int(o) for o in offs]),
                                  (C.c_size_t * n)(*[ln * sz for ln in lens])))
    return sb


@pytest.mark.parametrize("lens", LAYOUTS, ids=lambda t: f"{t[0]}+{t[1]}")
def test_sharded_cast_equals_the_unsharded_call(ec, lens):
    from erased_cells_hip.sharded import ShardGroup
    n = sum(lens)
    x, m = (a[:n] for a in R.scaled_inputs(R.F64, R.U8))
    assert x.size == n
    whole = ec.CellBuffer.from_vec(x)
    masked = ec.MaskedCellBuffer(whole, ec.Mask.new(m))
    with ShardGroup([0, 0], host_combine=True) as g:
        sx, sm = _scatter(g, x, lens, ec.Float64), _scatter(g, m, lens, ec.UInt8)
        made = [sx, sm]
        for dt, mode in ((ec.UInt8, "round"), (ec.Int16, "as"), (ec.Float32, "round"), (ec.UInt64, "round"), (ec.Float64, "as")):
            out = g.cast(sx, dt, mode)
            made.append(out)
            got, want = g.gather(out), whole.cast(dt, mode).to_numpy()
            assert R.same_cells(got, want).all() and R.same_cells(want, R.cast(R.CAST_MODE[mode], R.F64, x, dt)).all(), (dt, mode)
        for dt, (scale, offset) in ((ec.Int16, (10000.0, 0.0)), (ec.UInt8, (-0.37, 100.25)), (ec.Float64, (10.0, -1.0))):
            nd = R.nodata_of(dt)
            out, out_m = g.to_scaled(sx, dt, scale, offset), g.to_scaled(sx, dt, scale, offset, mask=sm, no_data=nd)
            made += [out, out_m]
            want, want_m = whole.to_scaled(dt, scale, offset).to_numpy(), masked.to_scaled(dt, scale, offset, ec.NoData.new(nd)).to_numpy()
            assert R.same_cells(g.gather(out), want).all() and R.same_cells(want, R.scaled(R.F64, x, None, scale, offset, dt)).all(), dt
            assert R.same_cells(g.gather(out_m), want_m).all() and R.same_cells(want_m, R.scaled(R.F64, x, m, scale, offset, dt, nd)).all(), dt
        g.sync()
        for b in made:
            b.free()


def test_a_refused_call_posts_nothing(ec):
    from erased_cells_hip.sharded import ShardGroup
    L, E = ec.lib(), ec._ffi
    lens = (1000, 24)
    x = R.gpu_inputs(R.F64, R.I16)[:sum(lens)]
    with ShardGroup([0, 0], host_combine=True) as g:
        sx = _scatter(g, x, lens, ec.Float64)
        sm = _scatter(g, np.ones(sum(lens), np.uint8), lens, ec.UInt8)
        out = g.alloc(ec.Int16, lens)
        n = (C.c_size_t * 2)(*lens)
        nd16, nd32 = ec.CellValue(ec.Int16, -9999).to_ec(), ec.CellValue(ec.Int32, -9999).to_ec()
        holed = (C.c_void_p * 2)(sx.ptrs[0], None)
        g.sync()
        posted = g.stat("jobs_posted")
        refused = [
            (L.ec_sharded_cast(g.handle, 2, ec.Float64, sx.ptrs, ec.Int16, out.ptrs, n), E.EC_ERR_ARG),
            (L.ec_sharded_cast(g.handle, E.EC_CAST_ROUND, 10, sx.ptrs, ec.Int16, out.ptrs, n), E.EC_ERR_UNSUPPORTED_TYPE),
            (L.ec_sharded_cast(g.handle, E.EC_CAST_ROUND, ec.Float64, sx.ptrs, 10, out.ptrs, n), E.EC_ERR_UNSUPPORTED_TYPE),
            (L.ec_sharded_cast(g.handle, E.EC_CAST_ROUND, ec.Float64, None, ec.Int16, out.ptrs, n), E.EC_ERR_ARG),
            (L.ec_sharded_cast(g.handle, E.EC_CAST_ROUND, ec.Float64, holed, ec.Int16, out.ptrs, n), E.EC_ERR_ARG),
            (L.ec_sharded_cast(g.handle, E.EC_CAST_ROUND, ec.Float64, sx.ptrs, ec.Int16, out.ptrs, None), E.EC_ERR_ARG),
            (L.ec_sharded_cast_scaled(g.handle, ec.Float64, sx.ptrs, sm.ptrs, n, 1.0, 0.0, ec.Int16, None, out.ptrs), E.EC_ERR_ARG),
            (L.ec_sharded_cast_scaled(g.handle, ec.Float64, sx.ptrs, None, n, 1.0, 0.0, ec.Int16, C.byref(nd16), out.ptrs), E.EC_ERR_ARG),
            (L.ec_sharded_cast_scaled(g.handle, ec.Float64, sx.ptrs, sm.ptrs, n, 1.0, 0.0, ec.Int16, C.byref(nd32), out.ptrs), E.EC_ERR_ARG),
            (L.ec_sharded_cast_scaled(g.handle, ec.Float64, sx.ptrs, None, n, float("nan"), 0.0, ec.Int16, None, out.ptrs), E.EC_ERR_ARG),
            (L.ec_sharded_cast_scaled(g.handle, ec.Float64, sx.ptrs, None, n, 1.0, float("inf"), ec.Int16, None, out.ptrs), E.EC_ERR_ARG),
            (L.ec_sharded_cast_scaled(g.handle, ec.Float64, sx.ptrs, None, n, 1.0, 0.0, 10, None, out.ptrs), E.EC_ERR_UNSUPPORTED_TYPE),
            (L.ec_sharded_cast_scaled(g.handle, ec.Float64, holed, None, n, 1.0, 0.0, ec.Int16, None, out.ptrs), E.EC_ERR_ARG),
        ]
        assert [st for st, _ in refused] == [e for _, e in refused]
        assert g.stat("jobs_posted") == posted, "a refused call posted a job"
        with pytest.raises(ec.EcError):
            g.cast(sx, ec.Int16, "floor")
        # the group is unharmed: the next call works
        done = g.cast(sx, ec.Int16)
        assert np.array_equal(g.gather(done), R.cast(R.ROUND, R.F64, x, R.I16)) and g.stat("jobs_posted") > posted
        for b in (sx, sm, out, done):
            b.free()
