"""Every refusal of ec_zonal_stats_device, ec_zonal_stats_compute, ec_sharded_zonal_stats and ec_zonal_broadcast
(include/erased_cells.h), each decided before the library asks for a device: this file needs none.  Only calls that are refused,
or that have nothing to do, are made — the pointers are addresses that are never dereferenced.  Also here: that the symbols are
exported, ec_zonal_workspace_bytes, the spellings the Python mirror accepts, that the launch shape the GPU tests restate
(tests/zonal_ref.py) is the one the kernels are built with, and the plan header's stand-alone program."""
import ctypes as C
import os
import re

import pytest

import stats_ref as R
import zonal_ref as Z
from host_program import run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED, ARG = 0, 2, 6
P, M, ZN, OUT, WS, TAB, DST, DMASK = 0x100000, 0x200000, 0x300000, 0x400000, 0x10000000, 0x500000, 0x600000, 0x700000   # never dereferenced


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    return ec


def device(L, t=R.U16, p=P, mask=None, zt=R.U8, zones=ZN, n=1000, nz=4, out=OUT, ws=WS):
    return L.ec_zonal_stats_device(t, p, mask, zt, zones, n, nz, out, ws, None)


def compute(L, t=R.U16, p=P, mask=None, zt=R.U8, zones=ZN, n=1000, nz=4, out=OUT):
    return L.ec_zonal_stats_compute(t, p, mask, zt, zones, n, nz, out, None)


def broadcast(L, zt=R.U8, zones=ZN, n=1000, nz=4, t=R.F64, table=TAB, dst=DST, dmask=None):
    return L.ec_zonal_broadcast(zt, zones, n, nz, t, table, dst, dmask, None)


STATS_REFUSALS = [
    ("no zones", dict(nz=0), "EC_ZONAL_MAX_ZONES"),
    ("a negative zone count", dict(nz=-1), "EC_ZONAL_MAX_ZONES"),
    ("257 zones", dict(nz=257), "EC_ZONAL_MAX_ZONES"),
    ("null values", dict(p=None), "null pointer"),
    ("null zones", dict(zones=None), "null pointer"),
    ("null records", dict(out=None), "null pointer"),
    ("more than 2^32 cells of 2 bytes", dict(n=2**32 + 1), "more cells than one exact record covers"),
    ("more than 2^31 cells of 4 bytes", dict(t=R.I32, n=2**31 + 1), "more cells than one exact record covers"),
]
DEVICE_ONLY = [
    ("null workspace", dict(ws=None), "null pointer"),
    ("the records on the values", dict(out=P + 1999), "records overlap an input"),
    ("the records on the zones", dict(out=ZN - 255), "records overlap an input"),
    ("the records on the mask", dict(mask=M, out=M + 999), "records overlap an input"),
    ("the workspace on the values", dict(ws=P - Z.workspace_bytes(4) + 1), "workspace overlaps an input"),
    ("the workspace on the zones", dict(ws=ZN + 999), "workspace overlaps an input"),
    ("the workspace on the mask", dict(mask=M, ws=M), "workspace overlaps an input"),
    ("the records in the workspace", dict(out=WS + 64), "records overlap the workspace"),
]


def test_every_refusal_of_the_statistics(ec):
    L = ec.lib()
    for call, name, cases in ((device, "ec_zonal_stats_device", STATS_REFUSALS + DEVICE_ONLY), (compute, "ec_zonal_stats_compute", STATS_REFUSALS)):
        for what, kw, text in cases:
            assert L.ec_tune_set(b"no such knob", 0) == ARG   # another text in between: the next one is this call's own
            assert call(L, **kw) == ARG, (name, what)
            msg = L.ec_last_error_string().decode()
            assert msg.startswith(name + ": ") and text in msg, (what, msg)
    # just inside every bound: refused by nothing here would mean a launch, so these stop at the NEXT refusal
    assert device(L, out=P + 2000, ws=None) == ARG and "null pointer" in L.ec_last_error_string().decode()
    assert device(L, n=2**32, out=P) == ARG and "records overlap an input" in L.ec_last_error_string().decode()
    assert device(L, t=R.F64, n=2**40, out=P) == ARG and "records overlap an input" in L.ec_last_error_string().decode()  # kind 1: no bound


def test_the_order_of_the_refusals(ec):
    """n_zones, the value type, the zone type, null pointers, the cell bound, the overlaps"""
    L = ec.lib()
    text = lambda: L.ec_last_error_string().decode()
    assert device(L, nz=0, t=10, zt=2, p=None, n=2**33, out=None) == ARG and "EC_ZONAL_MAX_ZONES" in text()
    assert device(L, t=10, zt=2, p=None, n=2**33, out=None) == UNSUPPORTED and "bad dtype" in text()
    assert device(L, zt=2, p=None, n=2**33, out=None) == UNSUPPORTED and "zone raster's type" in text()
    assert device(L, p=None, n=2**33, out=P) == ARG and "null pointer" in text()
    assert device(L, n=2**33, out=P) == ARG and "more cells" in text()
    assert device(L, out=P, ws=P) == ARG and "records overlap an input" in text()
    assert device(L, out=WS, ws=P) == ARG and "workspace overlaps an input" in text()
    assert broadcast(L, nz=0, t=10, zt=2, zones=None) == ARG and "EC_ZONAL_MAX_ZONES" in text()
    assert broadcast(L, t=10, zt=2, zones=None) == UNSUPPORTED and "bad dtype" in text()
    assert broadcast(L, zt=2, zones=None) == UNSUPPORTED and "zone raster's type" in text()
    assert broadcast(L, zones=None, n=2**62, dst=ZN) == ARG and "null pointer" in text()
    assert broadcast(L, n=2**62, dst=ZN) == ARG and "2^31 - 1 tiles" in text()
    assert broadcast(L, dst=ZN, dmask=ZN) == ARG and "dst overlaps an input" in text()


def test_a_bad_zone_type(ec):
    L = ec.lib()
    for zt in list(range(12)) + [255]:
        want = OK if zt in Z.ZONE_TYPES else UNSUPPORTED
        # n == 0 with null cell pointers: nothing to launch for the broadcast; the statistics are refused next (null records)
        assert broadcast(L, zt=zt, n=0, zones=None, table=None, dst=None) == want, zt
        assert device(L, zt=zt, out=None) == (ARG if want == OK else UNSUPPORTED), zt
        assert compute(L, zt=zt, out=None) == (ARG if want == OK else UNSUPPORTED), zt
    for bad in (10, 255):
        assert device(L, t=bad) == UNSUPPORTED and compute(L, t=bad) == UNSUPPORTED and broadcast(L, t=bad) == UNSUPPORTED


def test_every_refusal_of_the_broadcast(ec):
    L = ec.lib()
    for what, kw, text in [("no zones", dict(nz=0), "EC_ZONAL_MAX_ZONES"), ("257 zones", dict(nz=257), "EC_ZONAL_MAX_ZONES"),
                           ("null zones", dict(zones=None), "null pointer"), ("null table", dict(table=None), "null pointer"),
                           ("null dst", dict(dst=None), "null pointer"), ("dst on the zones", dict(dst=ZN + 999), "dst overlaps an input"),
                           ("dst on the table", dict(dst=TAB + 31), "dst overlaps an input"), ("dst_mask on the zones", dict(dmask=ZN), "dst_mask overlaps an input"),
                           ("dst_mask on the table", dict(dmask=TAB - 999), "dst_mask overlaps an input"), ("dst_mask in dst", dict(dmask=DST + 7999), "dst_mask overlaps dst")]:
        assert L.ec_tune_set(b"no such knob", 0) == ARG
        assert broadcast(L, **kw) == ARG, what
        msg = L.ec_last_error_string().decode()
        assert msg.startswith("ec_zonal_broadcast: ") and text in msg, (what, msg)
    assert broadcast(L, n=0) == OK and broadcast(L, n=0, zones=None, table=None, dst=None) == OK   # nothing to do
    assert broadcast(L, n=0, nz=300) == ARG                                                        # the checks come first
    # the statistics of no cells are n_zones empty records: the record pointer (and the device form's workspace) are still asked for
    assert device(L, n=0, p=None, zones=None, out=None) == ARG and "null pointer" in L.ec_last_error_string().decode()
    assert device(L, n=0, p=None, zones=None, ws=None) == ARG and compute(L, n=0, p=None, zones=None, out=None) == ARG
    assert device(L, n=0, nz=0) == ARG and compute(L, n=0, t=10) == UNSUPPORTED
    for t in range(10):
        for zt in Z.ZONE_TYPES:
            most = (2**31 - 1) * Z.broadcast_tile(t, zt) + Z.broadcast_cpl(t, zt) - 1
            assert broadcast(L, t=t, zt=zt, n=most + 1) == ARG and "2^31 - 1 tiles" in L.ec_last_error_string().decode(), (t, zt)
            assert broadcast(L, t=t, zt=zt, n=most, dst=ZN) == ARG and "dst overlaps" in L.ec_last_error_string().decode(), (t, zt)


def test_workspace_bytes_and_symbols(ec):
    L = ec.lib()
    assert [L.ec_zonal_workspace_bytes(k) for k in (0, 1, 256, 257)] == [0, 4096 * 48, 256 * 4096 * 48, 0]
    assert [L.ec_zonal_workspace_bytes(k) for k in (-1, 2, 255)] == [Z.workspace_bytes(k) for k in (-1, 2, 255)]
    raw = C.CDLL(ec._ffi.SO_PATH)
    for name in ("ec_zonal_workspace_bytes", "ec_zonal_stats_device", "ec_zonal_stats_compute", "ec_sharded_zonal_stats", "ec_zonal_broadcast"):
        assert hasattr(raw, name) and name in ec._ffi.SIGNATURES
    assert L.ec_abi_version() == 1


def test_the_sharded_form_refuses_a_null_group(ec):
    assert ec.lib().ec_sharded_zonal_stats(None, 1, None, None, 0, None, None, 4, None) == ARG


def test_the_python_spellings(ec):
    assert ec.EC_ZONAL_MAX_ZONES == ec._ffi.EC_ZONAL_MAX_ZONES == Z.MAX_ZONES == 256
    for cls in (ec.CellBuffer, ec.MaskedCellBuffer):
        assert callable(getattr(cls, "zonal_stats"))
    assert callable(ec.CellBuffer.broadcast)
    from erased_cells_hip import sharded
    assert callable(sharded.ShardGroup.zonal_stats)
    from erased_cells_hip import buffer as B

    class Fake(B.CellBuffer):   # no device memory: the spellings are refused before the library is called
        def __init__(self, ct, n):
            self.ct, self.n, self.mem = ct, n, None
    v, z = Fake(ec.UInt16, 10), Fake(ec.UInt8, 10)
    for bad in (0, 257, -1, True, 2.0, None, "4"):
        with pytest.raises(ec.EcError):
            v.zonal_stats(z, bad)
    with pytest.raises(ec.EcError):
        v.zonal_stats(Fake(ec.UInt8, 9), 4)       # another length
    with pytest.raises(ec.EcError):
        v.zonal_stats([0] * 10, 4)                # not a CellBuffer
    with pytest.raises(ec.EcError):
        z.broadcast(Fake(ec.Float64, 257))
    with pytest.raises(ec.EcError):
        z.broadcast(Fake(ec.Float64, 3), ec.Float32)   # the table is not of the type named


def test_the_shape_the_tests_restate_is_the_kernels():
    plan = open(os.path.join(ROOT, "erased-cells_amd", "csrc", "ec_zonal_plan.hpp")).read()

    def const(name):
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(\d+)\s*;", plan)
        assert m, name
        return int(m.group(1))
    assert (const("kBlock"), const("kWave"), const("kU"), const("kBroadcastU")) == (Z.BLOCK, Z.WAVE, Z.U, Z.BROADCAST_U)
    assert (const("kMaxZones"), const("kPartialBytes"), const("kRecordBytes")) == (Z.MAX_ZONES, Z.PARTIAL_BYTES, Z.RECORD_BYTES)
    reduce_plan = open(os.path.join(ROOT, "erased-cells_amd", "csrc", "ec_reduce_plan.hpp")).read()
    assert int(re.search(r"kMaxReduceBlocks\s*=\s*(\d+)", reduce_plan).group(1)) == Z.MAX_BLOCKS
    kernels = open(os.path.join(ROOT, "erased-cells_amd", "csrc", "ec_zonal_kernels.hpp")).read()
    assert "__launch_bounds__(ecz::kBlock) void k_zonal_partials(" in kernels and "constexpr int CPL = 16 / sizeof(T);" in kernels
    assert "atomicAdd(" not in kernels and "unsafeAtomicAdd" not in kernels   # integer LDS atomics are __hip_atomic_*; no float atomic
    for line in kernels.split("\n"):
        if "__hip_atomic_" in line:
            assert "double" not in line and "float" not in line, line
    header = open(os.path.join(ROOT, "include", "erased_cells.h")).read()
    assert re.search(r"EC_ZONAL_MAX_ZONES\s*=\s*256\b", header)


@pytest.mark.parametrize("target", ["test_zonal_plan", "test_zonal_plan_san"])
def test_the_plan_header_alone_and_under_sanitizers(target):
    """erased-cells_amd/host/test_zonal_plan.cpp: the LDS layout of csrc/ec_zonal_plan.hpp for every n_zones, the workspace size
    and the refusals — a stand-alone program, built plainly and with -fsanitize=address,undefined"""
    run_host_program(target)
