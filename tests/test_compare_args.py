"""ec_compare, ec_compare_scalar, ec_select, ec_masked_select and their sharded forms refuse bad arguments before any device work
and WITHOUT a device: a relation outside 1..6, a bad dtype, a null pointer with n > 0.  n == 0 is a no-op.  No GPU needed (the
checks come before the library asks for one; on a box with a GPU nothing here initialises it either)."""
import ctypes as C

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
    v = ec.CellValue(ec.Int32, 4).to_ec()
    bad_v = ec.CellValue(ec.Int32, 4).to_ec()
    bad_v.dtype = 10
    for rel in (0, 7, -1, 99):
        assert L.ec_compare(rel, 0, p, None, 0, p, None, 4, p, None) == E.EC_ERR_ARG and b"relation" in L.ec_last_error_string()
        assert L.ec_compare_scalar(rel, 0, p, None, 4, C.byref(v), p, None) == E.EC_ERR_ARG and b"relation" in L.ec_last_error_string()
    for lt, rt in ((10, 0), (0, 10), (255, 255)):
        assert L.ec_compare(E.EC_CMP_LT, lt, p, None, rt, p, None, 4, p, None) == E.EC_ERR_UNSUPPORTED_TYPE
    assert L.ec_compare_scalar(E.EC_CMP_LT, 10, p, None, 4, C.byref(v), p, None) == E.EC_ERR_UNSUPPORTED_TYPE
    assert L.ec_compare_scalar(E.EC_CMP_LT, 0, p, None, 4, C.byref(bad_v), p, None) == E.EC_ERR_UNSUPPORTED_TYPE
    assert L.ec_compare_scalar(E.EC_CMP_LT, 0, p, None, 4, None, p, None) == E.EC_ERR_ARG
    assert L.ec_select(10, p, p, p, 4, p, None) == E.EC_ERR_UNSUPPORTED_TYPE
    assert L.ec_masked_select(10, p, p, p, p, p, 4, p, p, None) == E.EC_ERR_UNSUPPORTED_TYPE
    # a null pointer with n > 0, one argument at a time
    for k in range(3):
        a = [p, p, p]
        a[k] = None
        assert L.ec_compare(E.EC_CMP_EQ, 0, a[0], None, 9, a[1], None, 4, a[2], None) == E.EC_ERR_ARG, k
    for k in range(2):
        a = [p, p]
        a[k] = None
        assert L.ec_compare_scalar(E.EC_CMP_EQ, 0, a[0], None, 4, C.byref(v), a[1], None) == E.EC_ERR_ARG, k
    for k in range(4):
        a = [p, p, p, p]
        a[k] = None
        assert L.ec_select(1, a[0], a[1], a[2], 4, a[3], None) == E.EC_ERR_ARG, k
    for k in range(7):
        a = [p] * 7
        a[k] = None
        assert L.ec_masked_select(1, a[0], a[1], a[2], a[3], a[4], 4, a[5], a[6], None) == E.EC_ERR_ARG, k
    assert b"null pointer" in L.ec_last_error_string()
    # n == 0 is a no-op, null pointers and all
    assert L.ec_compare(E.EC_CMP_GE, 3, None, None, 7, None, None, 0, None, None) == E.EC_OK
    assert L.ec_compare_scalar(E.EC_CMP_GE, 3, None, None, 0, C.byref(v), None, None) == E.EC_OK
    assert L.ec_select(9, None, None, None, 0, None, None) == E.EC_OK
    assert L.ec_masked_select(9, None, None, None, None, None, 0, None, None, None) == E.EC_OK
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
    v = ec.CellValue(ec.Float64, 0.3).to_ec()
    assert L.ec_compare(E.EC_CMP_LT, 0, p, None, 0, p, None, 4, p, None) == E.EC_ERR_NOT_INITIALIZED
    assert L.ec_compare_scalar(E.EC_CMP_GT, 0, p, None, 4, C.byref(v), p, None) == E.EC_ERR_NOT_INITIALIZED
    assert L.ec_select(0, p, p, p, 4, p, None) == E.EC_ERR_NOT_INITIALIZED
    assert L.ec_masked_select(0, p, p, p, p, p, 4, p, p, None) == E.EC_ERR_NOT_INITIALIZED
    assert bytes(buf) == bytes(64)


def test_sharded_forms_refuse_a_null_group(ec):
    L, E = ec.lib(), ec._ffi
    n1, p1 = (C.c_size_t * 1)(4), (C.c_void_p * 1)()
    v = ec.CellValue(ec.Int32, 4).to_ec()
    assert L.ec_sharded_compare(None, E.EC_CMP_LT, 0, p1, None, 0, p1, None, n1, p1) == E.EC_ERR_ARG
    assert b"null shard group" in L.ec_last_error_string()
    assert L.ec_sharded_compare_scalar(None, E.EC_CMP_LT, 0, p1, None, n1, C.byref(v), p1) == E.EC_ERR_ARG
    assert b"null shard group" in L.ec_last_error_string()


def test_python_mirror_refuses_an_unknown_relation(ec):
    from erased_cells_hip import buffer as B
    assert [B._relation(s) for s in ("<", "==", "<=", ">", "!=", ">=")] == [1, 2, 3, 4, 5, 6]
    assert B._relation(ec._ffi.EC_CMP_NE) == 5
    for bad in ("=>", "", 0, 7, None, True, 2.0):
        with pytest.raises(ec.EcError):
            B._relation(bad)
