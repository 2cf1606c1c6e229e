"""ec_sharded_composite_rank over an EC_GROUP_HOST_COMBINE group that lists device 0 twice, with uneven shard lengths — one of them
0: the gathered result, mask and aux equal the unsharded call (which tests/test_gpu_composite_rank.py holds to
tests/composite_rank_ref.py, and which is checked against it here too), and a refused call posts nothing."""
import ctypes as C

import numpy as np
import pytest

import composite_ref as CR
import composite_rank_ref as R

pytestmark = pytest.mark.gpu

LAYOUTS = ((531, 1520), (2051, 0), (0, 2051))   # the uneven layouts of tests/test_gpu_cast_sharded.py


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
def test_sharded_composite_rank_equals_the_unsharded_call(ec, lens):
    from erased_cells_hip.sharded import ShardGroup
    n = sum(lens)
    with ShardGroup([0, 0], host_combine=True) as g:
        made = []
        for ct, k, form in ((CR.U16, 5, "all"), (CR.F64, 9, "some"), (CR.I64, 3, "none"), (CR.U8, 64, "all")):
            layers, masks = R.stack(ct, k, n, form, seed=30)
            sl = [_scatter(g, a, lens, ct) for a in layers]
            sm = None if masks is None else [None if m is None else _scatter(g, m, lens, ec.UInt8) for m in masks]
            made += sl + ([] if sm is None else [m for m in sm if m is not None])
            whole = [ec.CellBuffer.from_vec(a) if (masks is None or masks[i] is None) else
                     ec.MaskedCellBuffer(ec.CellBuffer.from_vec(a), ec.Mask.new(masks[i])) for i, a in enumerate(layers)]
            masked = masks is not None and any(m is not None for m in masks)
            od = R.ordered(ct, layers, masks)
            for q, method in (((1, 2), "lower"), ((1, 2), "upper"), ((9, 10), "lower"), ((0, 1), "upper")):
                for mc in (1, min(2, k)):
                    res = g.composite_rank(sl, q, method, mc, aux=True, masks=sm)
                    made += list(res)
                    want = R.pick(ct, od, q[0], q[1], R.METHOD_NAMES.index(method), mc)
                    one, one_aux = ec.composite_rank(whole, q, method, mc, aux=True)
                    cells, aux = g.gather(res[0]), g.gather(res[-1])
                    where = (R.NAMES[ct], q, method, k, form, mc)
                    assert R.same_cells(cells, want[0]).all() and np.array_equal(aux, want[2]), where
                    assert R.same_cells(cells, (one.buffer() if masked else one).to_numpy()).all() and np.array_equal(aux, one_aux.to_numpy()), where
                    if masked:
                        assert len(res) == 3 and np.array_equal(g.gather(res[1]), want[1]) and np.array_equal(want[1], one.mask().to_numpy()), where
                    else:
                        assert len(res) == 2 and want[1].all(), where
        g.sync()
        for b in made:
            b.free()


def test_a_refused_call_posts_nothing(ec):
    from erased_cells_hip._ffi import PVP
    from erased_cells_hip.sharded import ShardGroup
    L, E = ec.lib(), ec._ffi
    lens = (1000, 24)
    ct, k = CR.I16, 3
    layers, masks = R.stack(ct, k, sum(lens), "all", seed=31)
    with ShardGroup([0, 0], host_combine=True) as g:
        sl, sm = [_scatter(g, a, lens, ct) for a in layers], [_scatter(g, m, lens, ec.UInt8) for m in masks]
        out, om, aux = g.alloc(ct, lens), g.alloc(ec.UInt8, lens), g.alloc(ec.UInt8, lens)
        n = (C.c_size_t * 2)(*lens)
        cols = lambda bufs: (PVP * len(bufs))(*[PVP() if b is None else C.cast(b if isinstance(b, C.Array) else b.ptrs, PVP) for b in bufs])
        lp, mp = cols(sl), cols(sm)
        holed = (C.c_void_p * 2)(sl[0].ptrs[0], None)
        g.sync()
        posted = g.stat("jobs_posted")
        call = lambda t=ct, l=lp, m=mp, kk=k, nn=n, num=1, den=2, method=0, mc=1, d=out.ptrs, dm=om.ptrs, a=aux.ptrs: \
            L.ec_sharded_composite_rank(g.handle, t, l, m, kk, nn, num, den, method, mc, d, dm, a)
        said = lambda st: (st, L.ec_last_error_string().decode())   # the status and the text the calling thread was left with
        own, pre = "ec_sharded_composite_rank: ", "ec_composite_rank: "   # refused by the group's entry point, or by its pre-check
        refused = [
            (said(call(kk=0)), E.EC_ERR_ARG, pre, "EC_COMPOSITE_MAX_LAYERS"), (said(call(kk=65)), E.EC_ERR_ARG, pre, "EC_COMPOSITE_MAX_LAYERS"),
            (said(call(den=0)), E.EC_ERR_ARG, pre, "EC_RANK_MAX_DEN"), (said(call(num=3, den=2)), E.EC_ERR_ARG, pre, "num <= den"),
            (said(call(den=65536)), E.EC_ERR_ARG, pre, "EC_RANK_MAX_DEN"),
            (said(call(method=2)), E.EC_ERR_ARG, pre, "ec_rank_method"), (said(call(method=-1)), E.EC_ERR_ARG, pre, "ec_rank_method"),
            (said(call(mc=0)), E.EC_ERR_ARG, pre, "min_count"), (said(call(mc=k + 1)), E.EC_ERR_ARG, pre, "min_count"),
            (said(call(t=10)), E.EC_ERR_UNSUPPORTED_TYPE, pre, "bad dtype 10"), (said(call(t=255)), E.EC_ERR_UNSUPPORTED_TYPE, pre, "bad dtype 255"),
            (said(call(l=None)), E.EC_ERR_ARG, own, "null argument"), (said(call(d=None)), E.EC_ERR_ARG, own, "null argument"),
            (said(call(nn=None)), E.EC_ERR_ARG, own, "null argument"),
            (said(call(l=cols([sl[0], None, sl[2]]))), E.EC_ERR_ARG, own, "layer 1 is a null column"),
            # a null pointer in a column of a shard that has cells
            (said(call(l=cols([sl[0], holed, sl[2]]))), E.EC_ERR_ARG, own, "layers[k][1] is null with n[1] = 24"),
            (said(call(dm=None)), E.EC_ERR_ARG, own, "a layer has a mask, so the result needs dst_mask"),
        ]
        assert [st for (st, _), *_ in refused] == [e for _, e, *_ in refused]
        for (_, text), _, head, words in refused:
            assert text.startswith(head) and words in text, text
        assert g.stat("jobs_posted") == posted, "a refused call posted a job"
        with pytest.raises(ec.EcError):
            g.composite_rank(sl, (1, 2), "median")
        with pytest.raises(ec.EcError):
            g.composite_rank(sl, 0.5)
        with pytest.raises(ec.EcError):
            g.composite_rank(sl, (1, 2), min_count=4)
        with pytest.raises(ec.EcError):
            g.composite_rank(sl + [om])                                # another cell type
        assert g.stat("jobs_posted") == posted
        # the group is unharmed: the next call works
        done, done_mask = g.composite_rank(sl, (1, 2), "upper", 2, masks=sm)
        want = R.composite_rank(ct, layers, masks, 1, 2, R.UPPER, 2)
        assert np.array_equal(g.gather(done), want[0]) and np.array_equal(g.gather(done_mask), want[1]) and g.stat("jobs_posted") > posted
        for b in sl + sm + [out, om, aux, done, done_mask]:
            b.free()
