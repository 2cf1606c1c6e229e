"""ec_focal_rank and ec_focal_majority on the GPU, through the C ABI, against tests/focal_rank_ref.py, the rule of
include/erased_cells.h in numpy.  Both operations copy bits, so every comparison is on the raw bits, NaN payloads included.  Inputs,
radii and shapes come from tests/focal_rank_cases.py; tests/test_focal_rank_faults.py shows that they expose the mistakes the kernel can
make.  Nothing expected comes from the library."""
import ctypes as C

import numpy as np
import pytest

import focal_rank_cases as K
import focal_rank_ref as R
import focal_ref as FR

pytestmark = pytest.mark.gpu

WHOLE = 1
MASKS = (None,) + K.MASK_KINDS
MASK_IDS = ["plain"] + list(K.MASK_KINDS)
NAMES = ["u8", "u16", "u32", "u64", "i8", "i16", "i32", "i64", "f32", "f64"]


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(K.UINT[a.dtype.itemsize])


def same(got, exp):
    """(cells, mask bytes or None) of a call against (cells, mask bytes) of the reference"""
    cells, mask = got
    assert cells.dtype == exp[0].dtype and cells.size == exp[0].size
    return np.array_equal(bits(cells), bits(exp[0].ravel())) and (mask is None or np.array_equal(mask, exp[1].ravel()))


def run(ec, ct, src, smask, cols, rows, radius, q, flags, want_mask):
    """one call through the C ABI -> (cells, mask bytes or None); q = (num, den, method), or None for the majority"""
    L = ec.lib()
    n = cols * rows
    out = ec.CellBuffer.empty(n, ct)
    om = ec.Mask.empty(n) if want_mask else None
    sm, dm = (smask.mem.ptr if smask is not None else None), (om.mem.ptr if om is not None else None)
    if q is None:
        ec._ffi.check(L.ec_focal_majority(ct, src.mem.ptr, sm, cols, rows, radius[0], radius[1], flags, out.mem.ptr, dm, ec.stream()))
    else:
        ec._ffi.check(L.ec_focal_rank(ct, src.mem.ptr, sm, cols, rows, radius[0], radius[1], q[0], q[1], q[2], flags, out.mem.ptr, dm, ec.stream()))
    return out.to_numpy(), (om.to_numpy() if om is not None else None)


def one_shape(ec, ct, kind, radius, cols, rows, raw=False):
    """every q, WHOLE on and off, and the majority, on one raster of each kind; -> launches made"""
    a, c, m = K.sources(ct, kind, cols, rows, raw)
    smask = ec.Mask.new(m.ravel()) if m is not None else None
    if raw:
        assert np.isnan(a).any() and np.isinf(a).any() and (bits(a) == bits(np.array([-0.0], a.dtype))[0]).any()
    src = ec.CellBuffer.from_vec(a.ravel())
    od = R.ordered(a, m, *radius)
    made = 0
    for flags in (0, WHOLE):
        want_mask = m is not None or bool(flags) or (cols + rows) % 2 == 0   # optional: given for half of the shapes
        for q in K.QS:
            got = run(ec, ct, src, smask, cols, rows, radius, q, flags, want_mask)
            assert same(got, R.pick(od, q[0], q[1], q[2], bool(flags), a.dtype)), (ct, kind, radius, cols, rows, q, flags)
            made += 1
    csrc = ec.CellBuffer.from_vec(c.ravel())
    cod = R.ordered(c, m, *radius)
    for flags in (0, WHOLE):
        want_mask = m is not None or bool(flags) or (cols + rows) % 2 == 1
        got = run(ec, ct, csrc, smask, cols, rows, radius, None, flags, want_mask)
        assert same(got, R.majority_pick(cod, bool(flags), c.dtype)), (ct, kind, radius, cols, rows, "majority", flags)
        made += 1
    return made


@pytest.mark.parametrize("kind", (None, "hashed"), ids=("plain", "hashed"))
@pytest.mark.parametrize("ct", range(10), ids=NAMES)
def test_every_cell_type(ec, ct, kind):
    """all ten cell types at 3 x 3 (the 16-word network) and 7 x 9 (the 64-word one): a shape below the footprint, one tile and its
    neighbours, more than one tile each way"""
    for radius in ((1, 1), (3, 4)):
        for cols, rows in ((2, 3), (K.TW, K.TH), (K.TW + 1, K.TH + 1), (2 * K.TW + 1, 2 * K.TH + 1)):
            one_shape(ec, ct, kind, radius, cols, rows)


@pytest.mark.parametrize("kind", MASKS, ids=MASK_IDS)
@pytest.mark.parametrize("ct", K.WORD_FORM_TYPES, ids=[NAMES[t] for t in K.WORD_FORM_TYPES])
def test_every_radius_shape_and_mask_kind(ec, ct, kind):
    made = 0
    for radius in K.RADII:
        assert 9 <= len(K.shapes(*radius)) <= 16
        for cols, rows in K.shapes(*radius):
            made += one_shape(ec, ct, kind, radius, cols, rows)
    assert made == 12 * sum(len(K.shapes(*r)) for r in K.RADII)


@pytest.mark.parametrize("ct", (K.F32, K.F64), ids=("f32", "f64"))
def test_raw_float_bits(ec, ct):
    """raw hashed bits with NaNs of many payloads, infinities of both signs, both zeros and the all-ones NaNs planted: bits are copied,
    so NaNs compare by payload too"""
    for kind in (None, "hashed"):
        for radius in ((1, 1), (2, 2), (7, 1)):
            for cols, rows in ((K.TW + 1, K.TH + 1), (37, 5)):
                one_shape(ec, ct, kind, radius, cols, rows, raw=True)


@pytest.mark.parametrize("arm", (dict(), dict(unaligned_vector=0), dict(mall_mb=0)), ids=("default", "cellwise-when-unaligned", "every-load-nt"))
def test_the_tuning_arms(ec, arm):
    """"unaligned_vector" off: cols = TW + 1 puts slots off a 16-byte boundary, so they are stored cell by cell; mall_mb = 0: every
    staged load is non-temporal"""
    with ec.tuned(**arm):
        for ct in K.WORD_FORM_TYPES:
            for radius in ((1, 1), (2, 2), (4, 3)):
                for cols, rows in ((K.TW + 1, K.TH + 1), (2 * K.TW, 3)):
                    one_shape(ec, ct, "hashed", radius, cols, rows)
                    one_shape(ec, ct, None, radius, cols, rows)


@pytest.mark.parametrize("ct", range(10), ids=NAMES)
def test_the_ends_are_ec_focal_min_and_max_on_the_device(ec, ct):
    """num = 0 is ec_focal MIN and num = den ec_focal MAX, bits and mask: both sides computed on the device, and held to focal_ref"""
    L = ec.lib()
    for radius in ((1, 1), (3, 3), (7, 1)):
        for cols, rows in ((K.TW + 3, K.TH + 2), (9, 2)):
            a = K.rank_raster(ct, cols, rows, 0xE0D + ct)
            m = K.mask_bytes("hashed", cols, rows, 0xE0E)
            src, smask = ec.CellBuffer.from_vec(a.ravel()), ec.Mask.new(m.ravel())
            for flags in (0, WHOLE):
                for op, q in ((FR.MIN, (0, 3, K.UPPER)), (FR.MAX, (3, 3, K.LOWER))):
                    out, om = ec.CellBuffer.empty(cols * rows, ct), ec.Mask.empty(cols * rows)
                    ec._ffi.check(L.ec_focal(op, ct, src.mem.ptr, smask.mem.ptr, cols, rows, radius[0], radius[1], flags, out.mem.ptr, om.mem.ptr, ec.stream()))
                    got = run(ec, ct, src, smask, cols, rows, radius, q, flags, True)
                    assert np.array_equal(bits(got[0]), bits(out.to_numpy())) and np.array_equal(got[1], om.to_numpy()), (ct, radius, cols, rows, op, flags)
                    assert same(got, FR.focal(op, a, m, radius[0], radius[1], bool(flags)))


def test_the_medians_agree_where_the_count_is_odd_and_follow_the_clipped_count(ec):
    cols, rows, radius = K.TW + 2, K.TH + 1, (1, 1)
    for ct in K.WORD_FORM_TYPES:
        a = K.rank_raster(ct, cols, rows, 0x0DD + ct)
        m = K.mask_bytes("hashed", cols, rows, 0x0DE)
        src, smask = ec.CellBuffer.from_vec(a.ravel()), ec.Mask.new(m.ravel())
        count = R.ordered(a, m, *radius)[2].ravel()
        lo, _ = run(ec, ct, src, smask, cols, rows, radius, (1, 2, K.LOWER), 0, True)
        hi, _ = run(ec, ct, src, smask, cols, rows, radius, (1, 2, K.UPPER), 0, True)
        odd = count % 2 == 1
        assert odd.any() and (~odd & (count > 0)).any()
        assert np.array_equal(bits(lo)[odd], bits(hi)[odd])
        if ct != 0:   # wider cells hardly tie: where the count is even the two medians are different taps
            assert (bits(lo)[~odd & (count > 0)] != bits(hi)[~odd & (count > 0)]).any()


def test_impulses_at_tile_and_raster_corners(ec):
    """one cell of another class at each position of the 2 x 2 block around every tile corner and at each raster corner: the median and
    the majority of a 5 x 3 footprint remove it everywhere, the 14/14 quantile (the maximum) spreads it over exactly its clipped
    footprint"""
    rx, ry = 2, 1
    for cols, rows in ((2 * K.TW + 1, 2 * K.TH + 1), (K.TW + 1, K.TH - 1)):
        for ct, value in ((0, 200), (8, 2.5)):
            dt = K.NP_DTYPES[ct]
            for y, x in K.impulse_positions(cols, rows):
                a = np.zeros((rows, cols), dtype=dt)
                a[y, x] = value
                foot = np.zeros((rows, cols), dtype=bool)
                foot[max(0, y - ry):y + ry + 1, max(0, x - rx):x + rx + 1] = True
                src = ec.CellBuffer.from_vec(a.ravel())
                assert not run(ec, ct, src, None, cols, rows, (rx, ry), (1, 2, K.LOWER), 0, False)[0].any(), (ct, y, x)
                assert not run(ec, ct, src, None, cols, rows, (rx, ry), None, 0, False)[0].any(), (ct, y, x)
                top = run(ec, ct, src, None, cols, rows, (rx, ry), (14, 14, K.LOWER), 0, False)[0]
                assert np.array_equal(top.reshape(rows, cols), np.where(foot, dt.type(value), dt.type(0))), (ct, y, x, cols, rows)


def test_more_than_a_grid_row_of_tiles_both_fronts(ec):
    """5 x 4 tiles with a ragged last row and column, masked: the two fronts and the tile numbering"""
    cols, rows = 4 * K.TW + 9, 3 * K.TH + 5
    for ct in (1, 9):
        for radius in ((3, 2), (2, 2)):
            one_shape(ec, ct, "hashed", radius, cols, rows)


def test_captured_in_a_graph_and_replayed_without_allocation(ec):
    import torch
    L = ec.lib()
    side = torch.cuda.Stream()
    ec._ffi.check(L.ec_prepare_stream(side.cuda_stream))
    cols, rows, radius = 2 * K.TW + 5, K.TH + 3, (2, 1)
    a = K.rank_raster(5, cols, rows, 0x6A9)
    m = K.mask_bytes("hashed", cols, rows, 0x6AA)
    t_src, t_mask = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(m.copy()).cuda()
    t_out = [torch.zeros(cols * rows, dtype=torch.int16, device="cuda") for _ in range(2)]
    t_om = [torch.zeros(cols * rows, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    before, after = C.c_int64(), C.c_int64()
    ec._ffi.check(L.ec_stat_get(b"pool_allocs", C.byref(before)))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        ec._ffi.check(L.ec_focal_rank(5, t_src.data_ptr(), t_mask.data_ptr(), cols, rows, 2, 1, 1, 2, K.UPPER, 0, t_out[0].data_ptr(), t_om[0].data_ptr(), s))
        ec._ffi.check(L.ec_focal_majority(5, t_src.data_ptr(), t_mask.data_ptr(), cols, rows, 2, 1, 0, t_out[1].data_ptr(), t_om[1].data_ptr(), s))
    for trial in range(2):
        if trial:
            a = K.class_raster(5, cols, rows, 0x6A9 + trial)
            t_src.copy_(torch.from_numpy(a.copy()))
        g.replay()
        torch.cuda.synchronize()
        od = R.ordered(a, m, *radius)
        assert same((t_out[0].cpu().numpy(), t_om[0].cpu().numpy()), R.pick(od, 1, 2, K.UPPER, False, a.dtype))
        assert same((t_out[1].cpu().numpy(), t_om[1].cpu().numpy()), R.majority_pick(od, False, a.dtype))
    ec._ffi.check(L.ec_stat_get(b"pool_allocs", C.byref(after)))
    assert after.value == before.value
