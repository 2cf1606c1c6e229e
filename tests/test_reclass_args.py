"""ec_reclass_table_build, ec_reclass and ec_sharded_reclass (include/erased_cells.h) without a device: every refusal, in the
header's order, with its text; that a refused build writes nothing and a build defines every byte; and THE THRESHOLDS — the
record read back and the class the kernels compute through it (reclass_ref.classes_through) against reclass_ref.classes, which
knows no thresholds: every cell of the 1- and 2-byte types for every break type and both `right`, planted cells for the wider
ones, unreachable suffixes, repeated thresholds.  Only calls that are refused, or that run on the host, are made — device
pointers are addresses that are never dereferenced.  Also: the symbols, the Python spellings, the launch shape the GPU tests
restate, and the plan header's stand-alone program."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import reclass_ref as Q
from host_program import run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED, ARG = 0, 2, 6
SRC, M, TAB, DST, DMASK = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000   # never dereferenced


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    return ec


def values_of(ec, dt, xs):
    return (ec._ffi.EcValue * len(xs))(*[ec.CellValue(dt, x).to_ec() for x in xs])


def build(ec, t=Q.F32, bt=Q.F64, breaks=(0.2, 0.4, 0.6), n=None, right=0, dt=Q.U8, values=(0, 1, 2, 3), valid=None, nodata=None, out="canary",
          null_breaks=False, null_values=False):
    """-> (status, the 4384 bytes of the output block afterwards); the block starts as 0xA5 bytes"""
    L = ec.lib()
    b = np.asarray(breaks, dtype=Q.NP[bt] if 0 <= bt < 10 else np.float64)
    vals = values if not isinstance(values, (tuple, list)) else values_of(ec, dt if 0 <= dt < 10 else 0, list(values))
    block = (C.c_uint8 * Q.TABLE_BYTES)(*([0xA5] * Q.TABLE_BYTES))
    vb = None if valid is None else (C.c_uint8 * len(valid))(*valid)
    nd = None if nodata is None else C.byref(nodata)
    st = L.ec_reclass_table_build(t, bt, None if null_breaks else b.ctypes.data_as(C.c_void_p), b.size if n is None else n, right, dt,
                                  None if null_values else vals, vb, nd, None if out is None else C.byref(block))
    return st, bytes(block)


def reclass(L, t=Q.U16, src=SRC, mask=None, n=1000, dt=Q.U8, table=TAB, dst=DST, dmask=None):
    return L.ec_reclass(t, src, mask, n, dt, table, dst, dmask, None)


def test_every_refusal_of_the_builder_in_order(ec):
    L = ec.lib()
    text = lambda: L.ec_last_error_string().decode()
    untouched = bytes([0xA5] * Q.TABLE_BYTES)
    u16 = lambda x: ec.CellValue(Q.U16, x).to_ec()
    bad_vals = values_of(ec, Q.U16, [0, 1, 2, 3])
    bad_vals[3].dtype = Q.U8
    good = values_of(ec, Q.U16, [0, 1, 2, 3])
    nan_b, flat, back = (0.2, float("nan"), 0.6), (0.2, 0.4, 0.4), (0.2, 0.6, 0.4)
    cases = [   # each is wrong in everything that comes later in the order, too
        (dict(n=0, right=7, t=10, null_breaks=True), ARG, "n_breaks"),
        (dict(n=-1, right=7, t=10), ARG, "n_breaks"),
        (dict(n=256, right=7, t=10), ARG, "n_breaks"),
        (dict(right=2, t=10, null_breaks=True), ARG, "right is not 0 or 1"),
        (dict(right=-1, t=10), ARG, "right is not 0 or 1"),
        (dict(t=10, null_breaks=True, dt=Q.U16, values=bad_vals), UNSUPPORTED, "bad dtype"),
        (dict(bt=10, null_breaks=True, dt=Q.U16, values=bad_vals), UNSUPPORTED, "bad dtype"),
        (dict(dt=255, null_breaks=True, values=bad_vals), UNSUPPORTED, "bad dtype"),
        (dict(null_breaks=True, dt=Q.U16, values=bad_vals), ARG, "null pointer"),
        (dict(null_values=True, dt=Q.U16, breaks=nan_b), ARG, "null pointer"),
        (dict(dt=Q.U16, values=bad_vals, nodata=u16(9), breaks=nan_b), ARG, "class value"),
        (dict(dt=Q.U16, values=good, nodata=ec.CellValue(Q.I16, 9).to_ec(), breaks=nan_b), ARG, "nodata value"),
        (dict(dt=Q.U16, values=good, nodata=u16(9), breaks=nan_b), ARG, "a break is NaN"),
        (dict(dt=Q.U16, values=good, nodata=u16(9), breaks=flat), ARG, "not strictly ascending"),
        (dict(dt=Q.U16, values=good, breaks=back), ARG, "not strictly ascending"),
        (dict(t=Q.F32, bt=Q.I64, breaks=(2**53, 2**53 + 1), dt=Q.U16, values=values_of(ec, Q.U16, [0, 1, 2])), ARG, "not strictly ascending"),   # equal in Float64
    ]
    for kw, status, why in cases:
        assert L.ec_tune_set(b"no such knob", 0) == ARG   # another text in between: the next one is this call's own
        st, block = build(ec, **kw)
        assert st == status, (kw, text())
        assert text().startswith("ec_reclass_table_build: ") and why in text(), (kw, text())
        assert block == untouched, ("a refused build wrote to its output", kw)
    assert build(ec, out=None)[0] == ARG and "null pointer" in text()
    # the neighbours of the refused: accepted
    assert build(ec, breaks=[0.5], values=(0, 1))[0] == OK and build(ec, bt=Q.U8, breaks=range(255), values=tuple(range(256)), dt=Q.U16)[0] == OK
    assert build(ec, right=1)[0] == OK and build(ec, breaks=(-0.0, 0.0, 0.6))[0] == OK
    assert build(ec, t=Q.I64, bt=Q.I64, breaks=(2**53, 2**53 + 1), values=(0, 1, 2))[0] == OK   # exact in Int64
    assert build(ec, bt=Q.F32, breaks=(-np.inf, 0.0, np.inf))[0] == OK


def test_the_record_is_deterministic_and_every_byte_of_it_defined(ec):
    nd = ec.CellValue(Q.I16, -1).to_ec()
    kw = dict(t=Q.F32, bt=Q.F64, breaks=(0.2, 0.4, 0.6), right=1, dt=Q.I16, values=(10, -20, 30, -40), valid=(1, 0, 9, 1), nodata=nd)
    st, a = build(ec, **kw)
    assert st == OK and a != bytes([0xA5] * Q.TABLE_BYTES)
    L = ec.lib()
    other = (C.c_uint8 * Q.TABLE_BYTES)()   # a block that starts as zeros
    b = np.asarray(kw["breaks"], np.float64)
    assert L.ec_reclass_table_build(Q.F32, Q.F64, b.ctypes.data_as(C.c_void_p), 3, 1, Q.I16, values_of(ec, Q.I16, [10, -20, 30, -40]),
                                    (C.c_uint8 * 4)(1, 0, 9, 1), C.byref(nd), C.byref(other)) == OK
    assert bytes(other) == a, "the record depends on what its memory held before"
    tab = Q.parse(a)
    assert (tab["t"], tab["dt"], tab["n_breaks"], tab["n_reached"], tab["flags"]) == (Q.F32, Q.I16, 3, 3, Q.HAS_NODATA | Q.DROPS)
    assert tab["reserved0"] == 0 and tab["reserved1"] == 0 and tab["nodata_bits"] == 0xFFFF
    assert tab["value_bits"][:4].tolist() == [10, 0xFFEC, 30, 0xFFD8] and not tab["value_bits"][4:].any()   # low bytes only
    assert tab["valid"][:4].tolist() == [1, 0, 1, 1] and not tab["valid"][4:].any() and not tab["thr"][3:].any()
    assert Q.from_key(Q.F32, tab["thr"][:3]).tolist() == [np.nextafter(np.float32(v), np.float32(1)) if np.float64(np.float32(v)) <= v else np.float32(v) for v in (0.2, 0.4, 0.6)]
    st, plain = build(ec, **dict(kw, valid=None, nodata=None))
    assert st == OK and Q.parse(plain)["flags"] == 0 and Q.parse(plain)["valid"][:4].tolist() == [1, 1, 1, 1] and Q.parse(plain)["valid"][4] == 0
    assert ec.ReclassTable(ec.Float32, [0.2, 0.4, 0.6], np.array([10, -20, 30, -40], np.int16), right=True, valid=(1, 0, 9, 1), nodata=-1).bytes() == a


def table(ec, t, bt, breaks, right):
    st, blob = build(ec, t=t, bt=bt, breaks=breaks, right=right, dt=Q.U8, values=values_of(ec, Q.U8, [c % 256 for c in range(len(breaks) + 1)]))
    assert st == OK, ec.lib().ec_last_error_string().decode()
    tab = Q.parse(blob)
    nr = int(tab["n_reached"])
    assert 0 <= nr <= tab["n_breaks"] == len(breaks) and np.all(tab["thr"][1:nr] >= tab["thr"][:max(nr - 1, 0)]) and not tab["thr"][nr:].any()
    return tab


@pytest.mark.parametrize("t", (Q.U8, Q.I8, Q.U16, Q.I16), ids=lambda t: Q.NAMES[t])
def test_thresholds_for_every_cell_of_the_narrow_types(ec, t):
    x = np.arange(np.iinfo(Q.NP[t]).min, np.iinfo(Q.NP[t]).max + 1).astype(Q.NP[t])
    for bt in range(Q.NT):
        for nb in (255, 7):
            breaks = Q.gpu_tables(t, bt, nb, seed=nb)
            for right in (0, 1):
                tab = table(ec, t, bt, breaks, right)
                assert np.array_equal(Q.classes_through(tab, t, x), Q.classes(t, x, bt, breaks, right)), (Q.NAMES[t], Q.NAMES[bt], nb, right)


@pytest.mark.parametrize("t", (Q.U32, Q.U64, Q.I32, Q.I64, Q.F32, Q.F64), ids=lambda t: Q.NAMES[t])
def test_thresholds_at_planted_cells_of_the_wide_types(ec, t):
    """each break as a cell and its two neighbours in t's order, 2^24 +- 1, 2^53 +- 1, the limits, +-0.0, +-inf, NaNs of both signs"""
    for bt in range(Q.NT):
        for nb in (255, 8, 1):
            breaks = Q.gpu_tables(t, bt, nb, seed=nb + 1)
            x = Q.gpu_inputs(t, bt, breaks, n_random=500)
            x = np.concatenate([x, Q.neighbours(t, Q.special_cells(t))])
            for right in (0, 1):
                tab = table(ec, t, bt, breaks, right)
                assert np.array_equal(Q.classes_through(tab, t, x), Q.classes(t, x, bt, breaks, right)), (Q.NAMES[t], Q.NAMES[bt], nb, right)


def test_unreachable_suffixes_and_repeated_thresholds(ec):
    tab = table(ec, Q.U8, Q.F64, [-1.5, 0.2, 0.7, 255.0, 300.0], 0)
    assert tab["n_reached"] == 4 and tab["thr"][:4].tolist() == [0, 1, 1, 255]
    tab = table(ec, Q.U8, Q.F64, [-1.5, 0.2, 0.7, 255.0, 300.0], 1)
    assert tab["n_reached"] == 3 and tab["thr"][:3].tolist() == [0, 1, 1]          # no u8 cell is past 255.0
    assert table(ec, Q.U8, Q.F64, [1e9, 2e9], 0)["n_reached"] == 0                   # every cell is class 0
    assert table(ec, Q.U8, Q.I16, [-300, -200], 0)["thr"][:2].tolist() == [0, 0]     # all breaks lie below: every cell is class 2
    assert table(ec, Q.I8, Q.U64, [2**40], 0)["n_reached"] == 0
    # NaN cells against infinite breaks: the thresholds are the first NaN keys
    f32 = table(ec, Q.F32, Q.F32, [np.inf], 1)
    assert f32["n_reached"] == 1 and Q.from_key(Q.F32, f32["thr"][:1]).view(np.uint32)[0] == 0x7F800001
    f32 = table(ec, Q.F32, Q.F64, [-np.inf], 0)
    assert Q.from_key(Q.F32, f32["thr"][:1]).view(np.uint32)[0] == 0xFF800000
    # u64 2^53 + 1 against u64 breaks is exact; against f64 it is 2^53
    exact = table(ec, Q.U64, Q.U64, np.array([2**53 + 1], np.uint64), 0)
    assert Q.from_key(Q.U64, exact["thr"][:1])[0] == 2**53 + 1
    rounded = table(ec, Q.U64, Q.F64, [2.0**53], 1)
    assert Q.from_key(Q.U64, rounded["thr"][:1])[0] == 2**53 + 2                     # 2^53 + 1 rounds to the break: not past it


def test_every_refusal_of_ec_reclass_in_order(ec):
    L = ec.lib()
    text = lambda: L.ec_last_error_string().decode()
    cases = [(dict(t=10, dt=10, src=None, table=TAB + 8, n=2**62), UNSUPPORTED, "bad dtype"),
             (dict(dt=10, src=None, table=TAB + 8, n=2**62), UNSUPPORTED, "bad dtype"),
             (dict(src=None, table=TAB + 8, n=2**62), ARG, "null pointer"),
             (dict(table=None, n=2**62), ARG, "null pointer"),
             (dict(dst=None, table=TAB + 8, n=2**62), ARG, "null pointer"),
             (dict(table=TAB + 8, n=2**62, dst=SRC), ARG, "not 16-byte aligned"),
             (dict(n=2**62, dst=SRC), ARG, "2^31 - 1 tiles"),
             (dict(dst=SRC + 1999), ARG, "dst overlaps an input"),
             (dict(dst=SRC - 999), ARG, "dst overlaps an input"),
             (dict(mask=M, dst=M + 999), ARG, "dst overlaps an input"),
             (dict(dst=TAB + Q.TABLE_BYTES - 1), ARG, "dst overlaps an input"),
             (dict(dmask=SRC), ARG, "dst_mask overlaps an input"),
             (dict(mask=M, dmask=M), ARG, "dst_mask overlaps an input"),
             (dict(dmask=TAB - 999), ARG, "dst_mask overlaps an input"),
             (dict(dmask=DST + 999), ARG, "dst_mask overlaps dst")]
    for kw, status, why in cases:
        assert L.ec_tune_set(b"no such knob", 0) == ARG
        assert reclass(L, **kw) == status, kw
        assert text().startswith("ec_reclass: ") and why in text(), (kw, text())
    assert reclass(L, n=0) == OK and reclass(L, n=0, src=None, table=None, dst=None) == OK and reclass(L, n=0, table=TAB + 1) == OK   # nothing to do
    assert reclass(L, n=0, t=10) == UNSUPPORTED                                                                                    # the types come first
    for t in range(Q.NT):
        for dt in (Q.U8, Q.I16, Q.F32, Q.F64):
            most = (2**31 - 1) * Q.tile(t, dt) + Q.cpl(t, dt) - 1
            assert reclass(L, t=t, dt=dt, n=most + 1) == ARG and "2^31 - 1 tiles" in text(), (t, dt)
            assert reclass(L, t=t, dt=dt, n=most, dst=SRC) == ARG and "dst overlaps" in text(), (t, dt)


def test_symbols_and_the_sharded_form_without_a_group(ec):
    L = ec.lib()
    raw = C.CDLL(ec._ffi.SO_PATH)
    for name in ("ec_reclass_table_build", "ec_reclass", "ec_sharded_reclass"):
        assert hasattr(raw, name) and name in ec._ffi.SIGNATURES
    assert L.ec_abi_version() == 1
    assert L.ec_sharded_reclass(None, Q.U16, None, None, None, Q.U8, None, None, None) == ARG
    assert C.sizeof(ec._ffi.EcReclassTable) == ec.EC_RECLASS_TABLE_BYTES == Q.TABLE_BYTES and ec.EC_RECLASS_MAX_BREAKS == Q.MAX_BREAKS
    header = open(os.path.join(ROOT, "include", "erased_cells.h")).read()
    assert re.search(r"EC_RECLASS_MAX_BREAKS\s*=\s*255\b", header) and re.search(r"EC_RECLASS_TABLE_BYTES\s*=\s*4384\b", header)


def test_the_python_spellings(ec):
    T = ec.ReclassTable
    assert T(ec.UInt16, [10, 20], [0, 1, 2]).bt == ec.UInt16            # integral and they fit: the raster's type
    assert T(ec.UInt16, [10, 20.5], [0, 1, 2]).bt == ec.Float64
    assert T(ec.UInt8, [10, 300], [0, 1, 2]).bt == ec.Float64            # 300 is no u8
    assert T(ec.Float32, [0.2, 0.4], [0, 1, 2]).bt == ec.Float64 and T(ec.Float32, [1, 2], [0, 1, 2]).bt == ec.Float32
    assert T(ec.Float32, [1, 2], [0, 1, 2], breaks_dtype=ec.Int16).bt == ec.Int16
    assert T(ec.Float32, np.array([1, 2], np.int8), [0, 1, 2]).bt == ec.Int8
    assert T(ec.UInt8, [1], [0, 255]).dt == ec.UInt8 and T(ec.UInt8, [1], [0, 256]).dt == ec.Int32 and T(ec.UInt8, [1], [0, 0.5]).dt == ec.Float64
    assert T(ec.UInt8, [1], np.array([0, 1], np.int16)).dt == ec.Int16 and T(ec.UInt8, [1], [0, 1], dtype=ec.Float32).dt == ec.Float32
    t = T(ec.UInt8, [1, 2], [5, 6, 7], valid=[1, 0, 1], nodata=9)
    assert t.drops and t.has_nodata and t.n_breaks == 2 and not T(ec.UInt8, [1], [0, 1]).drops
    for bad in (dict(breaks=[], values=[0]), dict(breaks=list(range(256)), values=list(range(257)), dtype=ec.Int32),
                dict(breaks=[1, 2], values=[0, 1]), dict(breaks=[1, 2], values=[0, 1, 2], valid=[1, 1]), dict(breaks=[2, 1], values=[0, 1, 2]),
                dict(breaks=[1.0, float("nan")], values=[0, 1, 2]), dict(breaks=[True, 2], values=[0, 1, 2])):
        with pytest.raises(ec.EcError):
            T(ec.UInt16, **bad)
    from erased_cells_hip import buffer as B
    from erased_cells_hip import sharded

    class Fake(B.CellBuffer):   # no device memory: refused before the library is asked to launch
        def __init__(self, ct, n):
            self.ct, self.n, self.mem = ct, n, None
    with pytest.raises(ec.EcError):
        Fake(ec.UInt8, 10).reclassify(T(ec.UInt16, [1], [0, 1]))                  # a table for another cell type
    with pytest.raises(ec.EcError):
        Fake(ec.UInt16, 10).reclassify(T(ec.UInt16, [1], [0, 1], nodata=0))       # a masked table for an unmasked raster
    with pytest.raises(ec.EcError):
        Fake(ec.UInt16, 10).reclassify(T(ec.UInt16, [1], [0, 1]), values=[0, 1])  # the table has its own
    with pytest.raises(ec.EcError):
        Fake(ec.UInt16, 10).reclassify([1, 2])                                    # breaks without values
    for cls in (ec.CellBuffer, ec.MaskedCellBuffer, sharded.ShardGroup):
        assert callable(getattr(cls, "reclassify")) and callable(getattr(cls, "classify"))


def test_the_shape_the_tests_restate_is_the_kernels():
    plan = open(os.path.join(ROOT, "erased-cells_amd", "csrc", "ec_reclass_plan.hpp")).read()

    def const(name):
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(\d+)\s*;", plan)
        assert m, name
        return int(m.group(1))
    assert (const("kBlock"), const("kU"), const("kMaxBreaks"), const("kSlots")) == (Q.BLOCK, Q.U, Q.MAX_BREAKS, 256)
    assert not re.search(r'#include\s+"(?!ec_lattice\.hpp|ec_order_key\.hpp|ec_compare_cell\.hpp)', plan)   # HIP-free, three headers of the library
    kernels = open(os.path.join(ROOT, "erased-cells_amd", "csrc", "ec_reclass_kernels.hpp")).read()
    assert "__launch_bounds__(kBlock) void k_reclass(" in kernels and "constexpr int CPL = 16 / max_of<sizeof(T), sizeof(W)>::value;" in kernels
    assert "ec_reclass.hip" in open(os.path.join(ROOT, "erased-cells_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("target", ["test_reclass_plan", "test_reclass_plan_san"])
def test_the_plan_header_alone_and_under_sanitizers(target):
    """erased-cells_amd/host/test_reclass_plan.cpp: csrc/ec_reclass_plan.hpp's thresholds against the predicate for every narrow
    cell, the refusals and the record — a stand-alone program, built plainly and with -fsanitize=address,undefined"""
    run_host_program(target)
