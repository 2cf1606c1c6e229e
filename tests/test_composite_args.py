"""Every refusal of ec_composite (include/erased_cells.h), each decided before the library asks for a device: this file needs none.
Only calls that are refused, or that have nothing to do, are made — the pointers are addresses that are never dereferenced.  Also
here: ec_composite_result_type, that the symbols are exported, the spellings the Python mirror accepts, and that the batch and tile
shape the tests restate (tests/composite_ref.py) are the ones the kernels are built with."""
import ctypes as C
import os
import re

import pytest

import composite_ref as R
from host_program import run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED, ARG = 0, 2, 6
L0, L1, L2, DST, M0, M1, DMASK, AUX = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000   # never dereferenced


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    return ec


def arr(ptrs):
    return None if ptrs is None else (C.c_void_p * len(ptrs))(*ptrs)


def composite(L, op=0, t=1, layers=(L0, L1, L2), masks=None, k=None, n=1000, min_count=1, dst=DST, dmask=None, aux=None):
    k = len(layers) if k is None else k
    return L.ec_composite(op, t, arr(layers), arr(masks), k, n, min_count, dst, dmask, aux, None)


SIXTY_FIVE = tuple(0x100000 + 0x1000 * i for i in range(65))

REFUSALS = [
    ("no layers", dict(layers=(L0,), k=0), "EC_COMPOSITE_MAX_LAYERS"),
    ("a negative layer count", dict(k=-1), "EC_COMPOSITE_MAX_LAYERS"),
    ("65 layers", dict(layers=SIXTY_FIVE), "EC_COMPOSITE_MAX_LAYERS"),
    ("min_count 0", dict(min_count=0), "min_count"),
    ("min_count above the layer count", dict(min_count=4), "min_count"),
    ("min_count 2^32 - 1", dict(min_count=0xffffffff), "min_count"),
    ("null layers", dict(layers=None, k=3), "null pointer"),
    ("a null layer", dict(layers=(L0, None, L2)), "layer 1 is a null pointer"),
    ("null dst", dict(dst=None), "null pointer"),
    ("a mask and no dst_mask", dict(masks=(None, M0, None)), "needs dst_mask"),
    ("dst is a layer", dict(dst=L2), "dst is layer 2"),
    ("dst_mask is a mask", dict(masks=(M0, None, M1), dmask=M1), "mask of layer 2"),
    ("aux is a mask", dict(masks=(M0, None, M1), dmask=DMASK, aux=M0), "mask of layer 0"),
    ("dst_mask is dst", dict(dmask=DST), "dst_mask is dst"),
    ("aux is dst", dict(aux=DST), "aux is dst or dst_mask"),
    ("aux is dst_mask", dict(dmask=DMASK, aux=DMASK), "aux is dst or dst_mask"),
]


def test_every_refusal(ec):
    L = ec.lib()
    for what, kw, text in REFUSALS:
        for op in R.OPS:
            assert L.ec_tune_set(b"no such knob", 0) == ARG   # another text in between: the next one is this call's own
            assert composite(L, op=op, **kw) == ARG, (what, op)
            msg = L.ec_last_error_string().decode()
            assert msg.startswith("ec_composite: ") and text in msg, (what, msg)
    for op in (-1, 6, 255):
        assert composite(L, op=op) == ARG and "ec_composite_op" in L.ec_last_error_string().decode(), op


def test_the_order_of_the_refusals(ec):
    """op, layer count, min_count, (dtype), null pointers, dst_mask, tiles, dst, the mask and aux outputs"""
    L = ec.lib()
    text = lambda: L.ec_last_error_string().decode()
    assert composite(L, op=9, k=0, min_count=0, t=10, dst=None) == ARG and "ec_composite_op" in text()
    assert composite(L, k=0, min_count=0, t=10, dst=None) == ARG and "EC_COMPOSITE_MAX_LAYERS" in text()
    assert composite(L, min_count=0, t=10, dst=None) == ARG and "min_count" in text()
    assert composite(L, t=10, dst=None) == UNSUPPORTED
    assert composite(L, dst=None, masks=(M0, M0, M0), n=1 << 62) == ARG and "null pointer" in text()
    assert composite(L, masks=(M0, M0, M0), n=1 << 62, dst=L0) == ARG and "needs dst_mask" in text()
    assert composite(L, n=1 << 62, dst=L0) == ARG and "2^31 - 1 tiles" in text()
    assert composite(L, dst=L0, masks=(M0, M0, M0), dmask=M0) == ARG and "dst is layer 0" in text()
    assert composite(L, masks=(M0, M0, M0), dmask=M0, aux=DST) == ARG and "mask of layer 0" in text()


def test_more_than_2_31_minus_1_tiles(ec):
    L = ec.lib()
    for op in R.OPS:
        for t in range(R.NT):
            tile = R.tile_cells(op, t)
            most = (2 ** 31 - 1) * tile + R.cpl(op, t) - 1          # the last length with 2^31 - 1 tiles of groups
            assert composite(L, op=op, t=t, n=most + 1) == ARG, (op, t)
            assert "2^31 - 1 tiles" in L.ec_last_error_string().decode()
            # one cell fewer passes this check: the call is refused by the next one (nothing may be launched from here)
            assert composite(L, op=op, t=t, n=most, dst=L1) == ARG and "dst is layer 1" in L.ec_last_error_string().decode(), (op, t)


def test_a_bad_dtype_is_unsupported_type(ec):
    L = ec.lib()
    for bad in (10, 255):
        assert composite(L, t=bad) == UNSUPPORTED
        assert L.ec_last_error_string().decode() == f"ec_composite: bad dtype {bad}"
        assert composite(L, t=bad, n=0) == UNSUPPORTED   # also for an empty stack


def test_an_empty_stack_is_ok_and_launches_nothing(ec):
    L = ec.lib()
    for op in R.OPS:
        for t in range(R.NT):
            assert composite(L, op=op, t=t, n=0) == OK
            assert composite(L, op=op, t=t, n=0, layers=None, k=3, dst=None) == OK   # the form the sharded entry point checks with
    assert composite(L, n=0, min_count=4) == ARG    # the checks come first


def test_result_type_and_symbols(ec):
    L = ec.lib()
    for t in range(R.NT):
        assert [L.ec_composite_result_type(op, t) for op in R.OPS] == [t, t, t, t, ec.Float64, ec.Float64] == [R.result_type(op, t) for op in R.OPS]
    assert [L.ec_composite_result_type(op, 0) for op in (-1, 6)] == [255, 255]
    assert [L.ec_composite_result_type(0, t) for t in (10, 255)] == [255, 255]
    raw = C.CDLL(ec._ffi.SO_PATH)
    for name in ("ec_composite", "ec_composite_result_type", "ec_sharded_composite"):
        assert hasattr(raw, name) and name in ec._ffi.SIGNATURES
    assert L.ec_abi_version() == 1


def test_the_sharded_form_refuses_a_null_group(ec):
    L = ec.lib()
    assert L.ec_sharded_composite(None, 0, 1, None, None, 1, None, 1, None, None, None) == ARG


def test_the_python_spellings(ec):
    from erased_cells_hip import buffer as B
    assert [B._composite_op(s) for s in R.OP_NAMES] == list(R.OPS) == [B._composite_op(k) for k in range(6)]
    E = ec._ffi
    assert (E.EC_COMPOSITE_FIRST, E.EC_COMPOSITE_LAST, E.EC_COMPOSITE_MIN, E.EC_COMPOSITE_MAX, E.EC_COMPOSITE_SUM, E.EC_COMPOSITE_MEAN) == R.OPS
    assert (E.EC_COMPOSITE_MAX_LAYERS, E.EC_COMPOSITE_NONE) == (R.MAX_LAYERS, R.NONE) == (64, 255)
    assert ec.COMPOSITE_OPS == dict(zip(R.OP_NAMES, R.OPS))
    for bad in ("median", "First", 6, -1, True, 1.0, None):
        with pytest.raises(ec.EcError):
            B._composite_op(bad)


def test_the_shape_the_tests_restate_is_the_kernels():
    text = open(os.path.join(ROOT, "erased-cells_amd", "csrc", "ec_composite_kernels.hpp")).read()
    batch = re.search(r"constexpr\s+int\s+kCompositeBatch\s*=\s*(\d+)\s*;", text)
    assert batch and int(batch.group(1)) == R.BATCH
    u = re.search(r"constexpr int composite_u\(bool sums, size_t cell_bytes\) \{ return sums \? (\d+) : cell_bytes == 1 \? (\d+) : (\d+); \}", text)
    assert u, "composite_u changed its form: restate it in tests/composite_ref.py"
    s, b, o = (int(x) for x in u.groups())
    for t in range(R.NT):
        assert R.groups_per_lane(R.SUM, t) == s and R.groups_per_lane(R.MAX, t) == (b if R.NP[t].itemsize == 1 else o)
    header = open(os.path.join(ROOT, "include", "erased_cells.h")).read()
    assert re.search(r"EC_COMPOSITE_MAX_LAYERS\s*=\s*64\b", header) and re.search(r"EC_COMPOSITE_NONE\s*=\s*255\b", header)
    i = header.index("ec_status ec_composite(")
    assert re.search(r"src/[a-z_/]+\.rs:\d+", header[i - 4500:i]), "ec_composite's comment cites the reference"


@pytest.mark.parametrize("target", ["test_composite_cell", "test_composite_cell_san"])
def test_the_cell_header_alone_and_under_sanitizers(target):
    """erased-cells_amd/host/test_composite_cell.cpp: the fold steps of csrc/ec_composite_cell.hpp for every type and op against
    an independent statement of the rule — a stand-alone program, built plainly and with -fsanitize=address,undefined"""
    run_host_program(target)
