"""Every typed entry point that asks for the device before it looks at the cell type, called with a code that is no cell type
(10 and 255) in each type position, a pair form with the bad code in either position: the call returns the status and leaves
the text in ec_last_error_string() that its `set_error` states, and writes nothing — the 16-cell device buffers and the host
results keep their sentinel.  Only code that refuses runs here: nothing is launched.

The expected (status, text) pairs are written out literally, per entry point: each has its own, and a dispatch that falls out
of its type table anywhere but at its refusal shows as a different pair.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UNSUPPORTED, ARG = 2, 6   # EC_ERR_UNSUPPORTED_TYPE, EC_ERR_ARG (include/erased_cells.h)
BAD = (10, 255)
N = 16
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def test_bad_codes_are_refused_with_each_entry_points_own_text(ec):
    L, E = ec.lib(), ec._ffi
    assert (E.EC_ERR_UNSUPPORTED_TYPE, E.EC_ERR_ARG) == (UNSUPPORTED, ARG)
    s = ec.stream()
    nbytes = N * 8 + 64                                    # 16 cells of the widest type, a stats record
    fill = np.full(nbytes, SENTINEL, np.uint8)
    mems = [ec.DeviceMem(nbytes) for _ in range(6)]
    for m in mems:
        E.check(L.ec_upload(m.ptr, fill.ctypes.data_as(C.c_void_p), nbytes, s))
    E.check(L.ec_stream_sync(s))
    a, b, out, ma, mb, mo = (m.ptr for m in mems)
    U8, F64 = ec.UInt8, ec.Float64

    def value(dtype):
        v = E.EcValue()
        C.memset(C.byref(v), SENTINEL, C.sizeof(v))
        v.dtype = dtype
        return v

    mn, mx = value(SENTINEL), value(SENTINEL)
    index, ordering = C.c_uint64(0xA5A5A5A5A5A5A5A5), C.c_int32(0x5A5A5A5A)
    stats = (C.c_uint8 * 64)(*([SENTINEL] * 64))             # an ec_stats
    host = lambda: (bytes(mn), bytes(mx), index.value, ordering.value, bytes(stats))
    host_before = host()
    v_u8, v_f64 = value(U8), value(F64)

    calls = []   # (what, status, text, call)

    def expect(what, status, text, call):
        calls.append((what, status, text, call))

    for bad in BAD:
        for op in (0, 3):   # EC_ADD, EC_DIV
            for lt, rt in ((bad, U8), (U8, bad), (F64, bad), (bad, bad)):
                expect(f"ec_binop {op} ({lt}, {rt})", UNSUPPORTED, "binop: bad dtype", lambda op=op, lt=lt, rt=rt: L.ec_binop(op, lt, a, rt, b, N, out, s))
                expect(f"ec_masked_binop {op} ({lt}, {rt})", UNSUPPORTED, "masked_binop: bad dtype",
                       lambda op=op, lt=lt, rt=rt: L.ec_masked_binop(op, lt, a, ma, rt, b, mb, N, out, mo, s))
            expect(f"ec_binop_scalar {op} ({bad})", UNSUPPORTED, "binop_scalar: bad dtype", lambda op=op, bad=bad: L.ec_binop_scalar(op, bad, a, N, C.byref(v_f64), out, s))
            expect(f"ec_binop_scalar {op}, scalar of dtype {bad}", ARG, "ec_binop_scalar: bad rhs", lambda op=op, bad=bad: L.ec_binop_scalar(op, U8, a, N, C.byref(value(bad)), out, s))
        expect(f"ec_neg ({bad})", UNSUPPORTED, f"ec_neg: bad dtype {bad}", lambda bad=bad: L.ec_neg(bad, a, N, out, s))
        for st, dt in ((bad, F64), (U8, bad), (bad, bad)):
            expect(f"ec_convert ({st}, {dt})", UNSUPPORTED, "ec_convert: bad dtype", lambda st=st, dt=dt: L.ec_convert(st, a, dt, out, N, s))
        for t, v in ((bad, v_u8), (bad, value(bad)), (U8, value(bad))):
            expect(f"ec_fill ({t}, value of dtype {v.dtype})", ARG, "ec_fill: value dtype must equal t", lambda t=t, v=v: L.ec_fill(t, out, N, C.byref(v), s))
        for m in (None, ma):
            expect(f"ec_min_max ({bad})", UNSUPPORTED, "min_max: bad dtype", lambda bad=bad, m=m: L.ec_min_max(bad, a, m, N, C.byref(mn), C.byref(mx), s))
            expect(f"ec_min_max_keys ({bad})", UNSUPPORTED, "min_max: bad dtype", lambda bad=bad, m=m: L.ec_min_max_keys(bad, a, m, N, out, s))
            expect(f"ec_stats_device ({bad})", UNSUPPORTED, f"ec_stats_device: bad dtype {bad}", lambda bad=bad, m=m: L.ec_stats_device(bad, a, m, N, out, s))
            expect(f"ec_stats_compute ({bad})", UNSUPPORTED, f"ec_stats_compute: bad dtype {bad}", lambda bad=bad, m=m: L.ec_stats_compute(bad, a, m, N, C.cast(stats, C.c_void_p), s))
        expect(f"ec_first_difference ({bad})", UNSUPPORTED, f"ec_first_difference: bad dtype {bad}", lambda bad=bad: L.ec_first_difference(bad, a, b, N, C.byref(index), s))
        for lt, rt in ((bad, U8), (U8, bad), (bad, bad)):
            expect(f"ec_buffer_cmp ({lt}, {rt})", UNSUPPORTED, "ec_buffer_cmp: bad dtype", lambda lt=lt, rt=rt: L.ec_buffer_cmp(lt, a, N, rt, b, N, C.byref(ordering), s))
        for nd in (None, v_u8, value(bad)):
            ndp = C.byref(nd) if nd is not None else None
            expect(f"ec_mask_from_nodata ({bad})", UNSUPPORTED, f"ec_mask_from_nodata: bad dtype {bad}", lambda bad=bad, ndp=ndp: L.ec_mask_from_nodata(bad, a, N, ndp, mo, s))
            expect(f"ec_mask_select ({bad})", UNSUPPORTED, f"ec_mask_select: bad dtype {bad}", lambda bad=bad, ndp=ndp: L.ec_mask_select(bad, a, ma, N, ndp, out, s))
        nd_bad = value(bad)
        expect(f"ec_mask_from_nodata, nodata of dtype {bad}", ARG, "ec_mask_from_nodata: nodata dtype must equal t", lambda nd=nd_bad: L.ec_mask_from_nodata(U8, a, N, C.byref(nd), mo, s))
        expect(f"ec_mask_select, nodata of dtype {bad}", ARG, "ec_mask_select: nodata dtype must equal t", lambda nd=nd_bad: L.ec_mask_select(U8, a, ma, N, C.byref(nd), out, s))
        expect(f"ec_synth_fill ({bad})", UNSUPPORTED, f"ec_synth_fill: dtype {bad} not supported", lambda bad=bad: L.ec_synth_fill(bad, out, N, 1, 0, 0.0, 1.0, s))
    # ec_synth_fill generates five of the ten types: the others are refused alike
    for t in (ec.UInt64, ec.Int8, ec.Int16, ec.Int32, ec.Int64):
        expect(f"ec_synth_fill ({t})", UNSUPPORTED, f"ec_synth_fill: dtype {t} not supported", lambda t=t: L.ec_synth_fill(t, out, N, 1, 0, 0.0, 1.0, s))

    assert len(calls) >= 100
    for what, status, text, call in calls:
        assert L.ec_tune_set(b"no such knob", 0) == ARG   # another text in between: the next one is this call's own
        got = call()
        assert (got, L.ec_last_error_string().decode()) == (status, text), what

    E.check(L.ec_stream_sync(s))
    for k, m in enumerate(mems):
        back = np.empty(nbytes, np.uint8)
        E.check(L.ec_download(back.ctypes.data_as(C.c_void_p), m.ptr, nbytes, s))
        assert np.array_equal(back, fill), f"device buffer {k} changed"
    assert host() == host_before, "a refused call wrote a host result"
