"""ec_cast, ec_cast_scaled and their sharded forms refuse bad arguments before any device work and WITHOUT a device: a mode outside
{0, 1}, a bad dtype, a null pointer with n > 0, a mask without a nodata value or the reverse, a nodata value of another type than
the destination, a scale or offset that is not finite.  n == 0 is EC_OK.  No GPU needed (the checks come before the library asks
for one; on a box with a GPU nothing here initialises it either)."""
import ctypes as C
import math

import pytest


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    return ec


def _initialised(ec):
    v = C.c_int64(-1)
    assert ec.lib().ec_stat_get(b"devices", C.byref(v)) == 0
    return v.value > 0


def test_refusals_need_no_device(ec):
    L, E = ec.lib(), ec._ffi
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    m = p
    nd16 = ec.CellValue(ec.Int16, -9999).to_ec()
    nd32 = ec.CellValue(ec.Int32, -9999).to_ec()
    # ec_cast: the mode, the dtypes, the pointers
    for mode in (2, -1, 99):
        assert L.ec_cast(mode, ec.Float64, p, ec.UInt8, p, 4, None) == E.EC_ERR_ARG and b"mode" in L.ec_last_error_string()
        assert L.ec_cast(mode, ec.UInt8, p, ec.Float64, p, 4, None) == E.EC_ERR_ARG       # a pair that fits is no exception
    for st, dt in ((10, 0), (0, 10), (255, 255)):
        for mode in (E.EC_CAST_AS, E.EC_CAST_ROUND):
            assert L.ec_cast(mode, st, p, dt, p, 4, None) == E.EC_ERR_UNSUPPORTED_TYPE
        assert L.ec_cast_scaled(st, p, None, 4, 1.0, 0.0, dt, None, p, None) == E.EC_ERR_UNSUPPORTED_TYPE
    for st, dt in ((ec.Float64, ec.UInt8), (ec.UInt8, ec.Float64), (ec.Int32, ec.Int32)):   # narrowing, fitting, the same type
        for k in range(2):
            a = [p, p]
            a[k] = None
            assert L.ec_cast(E.EC_CAST_ROUND, st, a[0], dt, a[1], 4, None) == E.EC_ERR_ARG, (st, dt, k)
            assert b"null pointer" in L.ec_last_error_string()
            assert L.ec_cast_scaled(st, a[0], None, 4, 2.0, 1.0, dt, None, a[1], None) == E.EC_ERR_ARG, (st, dt, k)
    # ec_cast_scaled: mask and nodata together or not at all; the nodata value has the destination's type; finite parameters
    assert L.ec_cast_scaled(ec.Float64, p, m, 4, 1.0, 0.0, ec.Int16, None, p, None) == E.EC_ERR_ARG
    assert L.ec_cast_scaled(ec.Float64, p, None, 4, 1.0, 0.0, ec.Int16, C.byref(nd16), p, None) == E.EC_ERR_ARG
    assert b"together" in L.ec_last_error_string()
    assert L.ec_cast_scaled(ec.Float64, p, m, 4, 1.0, 0.0, ec.Int16, C.byref(nd32), p, None) == E.EC_ERR_ARG
    assert b"nodata" in L.ec_last_error_string()
    for scale, offset in ((math.nan, 0.0), (math.inf, 0.0), (-math.inf, 0.0), (1.0, math.nan), (1.0, math.inf), (1.0, -math.inf)):
        assert L.ec_cast_scaled(ec.Float64, p, m, 4, scale, offset, ec.Int16, C.byref(nd16), p, None) == E.EC_ERR_ARG, (scale, offset)
        assert b"finite" in L.ec_last_error_string()
        assert L.ec_cast_scaled(ec.UInt8, p, None, 0, scale, offset, ec.Float64, None, p, None) == E.EC_ERR_ARG, (scale, offset)
    # never EC_ERR_NARROWING: all 100 pairs pass the checks (n == 0 is EC_OK and launches nothing, null pointers and all)
    for st in range(10):
        for dt in range(10):
            for mode in (E.EC_CAST_AS, E.EC_CAST_ROUND):
                assert L.ec_cast(mode, st, None, dt, None, 0, None) == E.EC_OK, (st, dt)
            assert L.ec_cast_scaled(st, None, None, 0, 10000.0, 0.0, dt, None, None, None) == E.EC_OK, (st, dt)
    assert L.ec_cast_scaled(ec.Float64, None, m, 0, 10000.0, 0.0, ec.Int16, C.byref(nd16), None, None) == E.EC_OK
    # the refused calls wrote nothing
    assert bytes(buf) == bytes(64)


def test_well_formed_calls_fail_loudly_without_a_device(ec):
    """Past the checks the library asks for a device: without one the call is an error, never a CPU fallback."""
    import torch
    if torch.cuda.is_available() or _initialised(ec):
        pytest.skip("a HIP device is present")
    L, E = ec.lib(), ec._ffi
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    assert L.ec_cast(E.EC_CAST_ROUND, ec.Float64, p, ec.UInt8, p, 4, None) == E.EC_ERR_NOT_INITIALIZED
    assert L.ec_cast(E.EC_CAST_AS, ec.UInt8, p, ec.Float64, p, 4, None) == E.EC_ERR_NOT_INITIALIZED
    assert L.ec_cast_scaled(ec.Float64, p, None, 4, 10000.0, 0.0, ec.Int16, None, p, None) == E.EC_ERR_NOT_INITIALIZED
    assert bytes(buf) == bytes(64)


def test_sharded_forms_refuse_a_null_group(ec):
    L, E = ec.lib(), ec._ffi
    n1, p1 = (C.c_size_t * 1)(4), (C.c_void_p * 1)()
    assert L.ec_sharded_cast(None, E.EC_CAST_ROUND, ec.Float64, p1, ec.UInt8, p1, n1) == E.EC_ERR_ARG
    assert b"null shard group" in L.ec_last_error_string()
    assert L.ec_sharded_cast_scaled(None, ec.Float64, p1, None, n1, 1.0, 0.0, ec.Int16, None, p1) == E.EC_ERR_ARG
    assert b"null shard group" in L.ec_last_error_string()


def test_python_mirror_refuses_an_unknown_mode(ec):
    from erased_cells_hip import buffer as B
    assert [B._cast_mode(s) for s in ("as", "round")] == [0, 1] and B._cast_mode(ec._ffi.EC_CAST_ROUND) == 1
    for bad in ("floor", "", 2, -1, None, True, 1.0):
        with pytest.raises(ec.EcError):
            B._cast_mode(bad)
