"""Every refusal of ec_zonal_table_device, ec_zonal_table_compute, ec_sharded_zonal_table and ec_zonal_lookup
(include/erased_cells.h), each decided before the library asks for a device: this file needs none.  Only calls that are refused,
or that have nothing to do, are made — the pointers are addresses that are never dereferenced.  Also here: that the symbols are
exported, ec_zonal_table_workspace_bytes, the constants against the headers, the spellings the Python mirror accepts, and the
cell header's stand-alone program, plain and under the sanitizers."""
import ctypes as C
import os
import re

import pytest

import stats_ref as R
import zonal_ref as Z
import zonal_table_ref as ZT
from host_program import run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED, ARG = 0, 2, 6
P, M, ZN, OUT, WS, TAB, DST, DMASK = 0x100000, 0x200000, 0x300000, 0x400000, 0x10000000, 0x500000, 0x600000, 0x700000   # never dereferenced


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    return ec


def device(L, t=R.U16, p=P, mask=None, zt=R.U8, zones=ZN, n=1000, nz=4, out=OUT, ws=WS):
    return L.ec_zonal_table_device(t, p, mask, zt, zones, n, nz, out, ws, None)


def compute(L, t=R.U16, p=P, mask=None, zt=R.U8, zones=ZN, n=1000, nz=4, out=OUT):
    return L.ec_zonal_table_compute(t, p, mask, zt, zones, n, nz, out, None)


def lookup(L, zt=R.U8, zones=ZN, n=1000, nz=4, t=R.F64, table=TAB, dst=DST, dmask=None):
    return L.ec_zonal_lookup(zt, zones, n, nz, t, table, dst, dmask, None)


TABLE_REFUSALS = [
    ("no zones", dict(nz=0), "EC_ZONAL_TABLE_MAX_ZONES"),
    ("a negative zone count", dict(nz=-1), "EC_ZONAL_TABLE_MAX_ZONES"),
    ("2^24 + 1 zones", dict(nz=2**24 + 1), "EC_ZONAL_TABLE_MAX_ZONES"),
    ("null values", dict(p=None), "null pointer"),
    ("null zones", dict(zones=None), "null pointer"),
    ("null records", dict(out=None), "null pointer"),
    ("more than 2^32 cells of 2 bytes", dict(n=2**32 + 1), "more cells than one exact record covers"),
    ("more than 2^31 cells of 4 bytes", dict(t=R.I32, n=2**31 + 1), "more cells than one exact record covers"),
    ("more than 2^32 cells of the f64 kind", dict(t=R.F64, n=2**32 + 1), "more than 2^32 cells"),
    ("more than 2^32 cells of u64", dict(t=R.U64, n=2**32 + 1), "more than 2^32 cells"),
]
DEVICE_ONLY = [
    ("null workspace", dict(ws=None), "null pointer"),
    ("records off a 16-byte line", dict(out=OUT + 8), "records are not 16-byte aligned"),
    ("workspace off a 16-byte line", dict(ws=WS + 4), "workspace is not 16-byte aligned"),
    ("the records on the values", dict(out=P + 1984), "records overlap an input"),
    ("the records on the zones", dict(out=ZN - 240), "records overlap an input"),
    ("the records on the mask", dict(mask=M, out=M + 992), "records overlap an input"),
    ("the workspace on the values", dict(ws=P - 4 * 48 + 16), "workspace overlaps an input"),
    ("the workspace on the zones", dict(ws=ZN + 992), "workspace overlaps an input"),
    ("the workspace on the mask", dict(mask=M, ws=M), "workspace overlaps an input"),
    ("the records in the workspace", dict(out=WS + 64), "records overlap the workspace"),
]


def test_every_refusal_with_its_text(ec):
    L = ec.lib()
    for call, name, cases in ((device, "ec_zonal_table_device", TABLE_REFUSALS + DEVICE_ONLY), (compute, "ec_zonal_table_compute", TABLE_REFUSALS)):
        for what, kw, text in cases:
            assert L.ec_tune_set(b"no such knob", 0) == ARG   # another text in between: the next one is this call's own
            assert call(L, **kw) == ARG, (name, what)
            msg = L.ec_last_error_string().decode()
            assert msg.startswith(name + ": ") and text in msg, (what, msg)
    # just inside every bound: these stop at the NEXT refusal
    assert device(L, nz=2**24, ws=None) == ARG and "null pointer" in L.ec_last_error_string().decode()
    assert device(L, n=2**32, out=P) == ARG and "records overlap an input" in L.ec_last_error_string().decode()
    assert device(L, t=R.F64, n=2**32, out=P) == ARG and "records overlap an input" in L.ec_last_error_string().decode()
    # the host form takes records of any alignment: aligned or not, this one is refused for its null values alone
    assert compute(L, out=OUT + 1, p=None) == ARG and "null pointer" in L.ec_last_error_string().decode()


def test_the_order_of_the_refusals(ec):
    """n_zones, the value type, the zone type, null pointers, the cell bound, the alignment, the overlaps"""
    L = ec.lib()
    text = lambda: L.ec_last_error_string().decode()
    assert device(L, nz=0, t=10, zt=2, p=None, n=2**33, out=None) == ARG and "EC_ZONAL_TABLE_MAX_ZONES" in text()
    assert device(L, t=10, zt=2, p=None, n=2**33, out=None) == UNSUPPORTED and "bad dtype" in text()
    assert device(L, zt=2, p=None, n=2**33, out=None) == UNSUPPORTED and "zone raster's type" in text()
    assert device(L, p=None, n=2**33, out=P + 8) == ARG and "null pointer" in text()
    assert device(L, n=2**33, out=P + 8) == ARG and "more cells" in text()
    assert device(L, out=P + 8, ws=P + 8) == ARG and "records are not 16-byte aligned" in text()
    assert device(L, out=P, ws=P + 8) == ARG and "workspace is not 16-byte aligned" in text()
    assert device(L, out=P, ws=P) == ARG and "records overlap an input" in text()
    assert device(L, out=WS, ws=P) == ARG and "workspace overlaps an input" in text()
    assert device(L, out=WS, ws=WS) == ARG and "records overlap the workspace" in text()
    # the reference's order, on the same calls
    assert ZT.refusal(0, 10, 2, 0, ZN, 2**33, 0, WS) == "EC_ZONAL_TABLE_MAX_ZONES" and ZT.refusal(4, 10, 2, 0, ZN, 2**33, 0, WS) == "bad dtype"
    assert ZT.refusal(4, R.U16, 2, 0, ZN, 2**33, 0, WS) == "zone raster's type" and ZT.refusal(4, R.U16, R.U8, 0, ZN, 2**33, P + 8, WS) == "null pointer"
    assert ZT.refusal(4, R.U16, R.U8, P, ZN, 2**33, P + 8, WS) == "more cells" and ZT.refusal(4, R.F64, R.U8, P, ZN, 2**33, P + 8, WS) == "more than 2^32 cells"
    assert ZT.refusal(4, R.U16, R.U8, P, ZN, 10, P + 8, WS + 8) == "records are not 16-byte aligned"
    assert ZT.refusal(4, R.U16, R.U8, P, ZN, 10, OUT, WS + 8) == "workspace is not 16-byte aligned" and ZT.refusal(4, R.U16, R.U8, P, ZN, 10, OUT, WS) is None
    assert lookup(L, nz=0, t=10, zt=2, zones=None) == ARG and "EC_ZONAL_TABLE_MAX_ZONES" in text()
    assert lookup(L, t=10, zt=2, zones=None) == UNSUPPORTED and "bad dtype" in text()
    assert lookup(L, zt=2, zones=None) == UNSUPPORTED and "zone raster's type" in text()
    assert lookup(L, zones=None, n=2**62, dst=ZN) == ARG and "null pointer" in text()
    assert lookup(L, n=2**62, dst=ZN) == ARG and "2^31 - 1 tiles" in text()
    assert lookup(L, dst=ZN, dmask=ZN) == ARG and "dst overlaps an input" in text()


def test_a_bad_type(ec):
    L = ec.lib()
    for zt in list(range(12)) + [255]:
        want = OK if zt in Z.ZONE_TYPES else UNSUPPORTED
        assert lookup(L, zt=zt, n=0, zones=None, table=None, dst=None) == want, zt
        assert device(L, zt=zt, out=None) == (ARG if want == OK else UNSUPPORTED), zt
        assert compute(L, zt=zt, out=None) == (ARG if want == OK else UNSUPPORTED), zt
    for bad in (10, 255):
        assert device(L, t=bad) == UNSUPPORTED and compute(L, t=bad) == UNSUPPORTED and lookup(L, t=bad) == UNSUPPORTED


def test_every_refusal_of_the_lookup(ec):
    L = ec.lib()
    for what, kw, text in [("no zones", dict(nz=0), "EC_ZONAL_TABLE_MAX_ZONES"), ("2^24 + 1 zones", dict(nz=2**24 + 1), "EC_ZONAL_TABLE_MAX_ZONES"),
                           ("null zones", dict(zones=None), "null pointer"), ("null table", dict(table=None), "null pointer"),
                           ("null dst", dict(dst=None), "null pointer"), ("dst on the zones", dict(dst=ZN + 999), "dst overlaps an input"),
                           ("dst on the table", dict(dst=TAB + 31), "dst overlaps an input"), ("dst on a long table", dict(nz=2**20, dst=TAB + 8 * 2**20 - 1), "dst overlaps an input"),
                           ("dst_mask on the zones", dict(dmask=ZN), "dst_mask overlaps an input"),
                           ("dst_mask on the table", dict(dmask=TAB - 999), "dst_mask overlaps an input"), ("dst_mask in dst", dict(dmask=DST + 7999), "dst_mask overlaps dst")]:
        assert L.ec_tune_set(b"no such knob", 0) == ARG
        assert lookup(L, **kw) == ARG, what
        msg = L.ec_last_error_string().decode()
        assert msg.startswith("ec_zonal_lookup: ") and text in msg, (what, msg)
    assert lookup(L, n=0) == OK and lookup(L, n=0, nz=2**24, zones=None, table=None, dst=None) == OK   # nothing to do
    assert lookup(L, n=0, nz=2**24 + 1) == ARG                                                          # the checks come first
    assert device(L, n=0, p=None, zones=None, out=None) == ARG and "null pointer" in L.ec_last_error_string().decode()
    assert device(L, n=0, p=None, zones=None, ws=None) == ARG and compute(L, n=0, p=None, zones=None, out=None) == ARG
    for t in range(10):
        for zt in Z.ZONE_TYPES:
            most = (2**31 - 1) * Z.broadcast_tile(t, zt) + Z.broadcast_cpl(t, zt) - 1
            assert lookup(L, t=t, zt=zt, n=most + 1) == ARG and "2^31 - 1 tiles" in L.ec_last_error_string().decode(), (t, zt)
            assert lookup(L, t=t, zt=zt, n=most, dst=ZN) == ARG and "dst overlaps" in L.ec_last_error_string().decode(), (t, zt)


def test_workspace_bytes_and_symbols(ec):
    L = ec.lib()
    for t in range(10):
        words = ZT.WORDS[R.KIND[t]]
        assert [L.ec_zonal_table_workspace_bytes(t, k) for k in (0, 1, 2**24, 2**24 + 1)] == [0, 8 * words, 2**24 * 8 * words, 0], t
        assert [L.ec_zonal_table_workspace_bytes(t, k) for k in (-1, 2, 257, 65537)] == [ZT.workspace_bytes(t, k) for k in (-1, 2, 257, 65537)]
        assert L.ec_zonal_table_workspace_bytes(t, 2**24) < 2**32 and L.ec_zonal_table_workspace_bytes(t, 5) % 16 == 0
    assert L.ec_zonal_table_workspace_bytes(10, 4) == 0 and L.ec_zonal_table_workspace_bytes(255, 4) == 0
    raw = C.CDLL(ec._ffi.SO_PATH)
    for name in ("ec_zonal_table_workspace_bytes", "ec_zonal_table_device", "ec_zonal_table_compute", "ec_sharded_zonal_table", "ec_zonal_lookup"):
        assert hasattr(raw, name) and name in ec._ffi.SIGNATURES
    assert L.ec_abi_version() == 1


def test_the_sharded_form_refuses_a_null_group(ec):
    assert ec.lib().ec_sharded_zonal_table(None, 1, None, None, 0, None, None, 4, None) == ARG


def test_the_constants_against_the_headers(ec):
    assert ec.EC_ZONAL_TABLE_MAX_ZONES == ec._ffi.EC_ZONAL_TABLE_MAX_ZONES == ZT.MAX_ZONES == 2**24
    assert ec.EC_ZONAL_MAX_ZONES == 256   # the first family keeps its cap
    header = open(os.path.join(ROOT, "include", "erased_cells.h")).read()
    assert re.search(r"EC_ZONAL_TABLE_MAX_ZONES\s*=\s*1\s*<<\s*24\b", header) and re.search(r"EC_ZONAL_MAX_ZONES\s*=\s*256\b", header)
    rust = open(os.path.join(ROOT, "erased-cells_amd", "rust", "erased-cells-hip", "src", "ffi.rs")).read()
    assert re.search(r"EC_ZONAL_TABLE_MAX_ZONES: usize = 1 << 24;", rust)
    plan = open(os.path.join(ROOT, "erased-cells_amd", "csrc", "ec_zonal_table_plan.hpp")).read()

    def const(name):
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", plan)
        assert m, name
        return eval(m.group(1).replace("uint64_t(1)", "1"))   # noqa: S307 — `1 << 24`, `256`
    assert (const("kMaxZones"), const("kBlock"), const("kU"), const("kMaxCellsKind1")) == (ZT.MAX_ZONES, ZT.BLOCK, ZT.U, ZT.MAX_CELLS_KIND1)
    assert re.search(r"words\(int kind\) \{ return kind == 0 \? (\d+) : (\d+); \}", plan).groups() == (str(ZT.WORDS[0]), str(ZT.WORDS[1]))
    kernels = open(os.path.join(ROOT, "erased-cells_amd", "csrc", "ec_zonal_table_kernels.hpp")).read()
    assert "__launch_bounds__(ezt::kBlock) void k_ztable_pass(" in kernels and "constexpr int CPL = 16 / sizeof(T);" in kernels
    assert "atomicAdd(" not in kernels and "unsafeAtomicAdd" not in kernels and "__shared__" not in kernels   # integer atomics on global words only
    for line in kernels.split("\n"):
        if "__hip_atomic_" in line:
            assert "double" not in line and "float" not in line and "__HIP_MEMORY_SCOPE_AGENT" in line, line


def test_the_python_refusals(ec):
    for cls in (ec.CellBuffer, ec.MaskedCellBuffer):
        assert callable(getattr(cls, "zonal_table"))
    assert callable(ec.CellBuffer.lookup)
    from erased_cells_hip import buffer as B
    from erased_cells_hip import sharded
    assert callable(sharded.ShardGroup.zonal_table)

    class Fake(B.CellBuffer):   # no device memory: the spellings are refused before the library is called
        def __init__(self, ct, n):
            self.ct, self.n, self.mem = ct, n, None
    v, z = Fake(ec.UInt16, 10), Fake(ec.UInt8, 10)
    for bad in (0, 2**24 + 1, -1, True, 2.0, None, "4"):
        with pytest.raises(ec.EcError):
            v.zonal_table(z, bad)
    with pytest.raises(ec.EcError):
        v.zonal_table(Fake(ec.UInt8, 9), 4)       # another length
    with pytest.raises(ec.EcError):
        v.zonal_table([0] * 10, 4)                # not a CellBuffer
    with pytest.raises(ec.EcError):
        z.lookup(Fake(ec.Float64, 2**24 + 1))
    with pytest.raises(ec.EcError):
        z.lookup(Fake(ec.Float64, 3), ec.Float32)   # the table is not of the type named
    for bad in (0, 257):                            # the first family still refuses what it refused
        with pytest.raises(ec.EcError):
            v.zonal_stats(z, bad)
    with pytest.raises(ec.EcError):
        z.broadcast(Fake(ec.Float64, 257))
    # the rows of ec_stats as numpy sees them
    raw = (ec._ffi.EcStats * 2)()
    raw[1].count, raw[1].sum, raw[1].mean, raw[1].stddev = 7, 1.5, 2.5, 3.5
    raw[1].min.dtype = raw[1].max.dtype = ec.Int16
    raw[1].min.v.i16, raw[1].max.v.i16 = -3, 9
    rows = B.stats_table(bytes(raw), ec.Int16)
    assert rows.dtype.names == ("count", "min", "max", "sum", "mean", "stddev")
    assert rows[1].tolist() == (7, -3, 9, 1.5, 2.5, 3.5) and rows["min"].dtype == "int16"


@pytest.mark.parametrize("target", ["test_zonal_table_cell", "test_zonal_table_cell_san", "test_zonal_table_cell_tsan"])
def test_the_cell_header_alone_and_under_sanitizers(target):
    """erased-cells_amd/host/test_zonal_table_cell.cpp: csrc/ec_zonal_table_cell.hpp against 128-bit arithmetic — a stand-alone program,
    built plainly, with -fsanitize=address,undefined and with -fsanitize=thread"""
    run_host_program(target)
