"""The host side of the band statistics without a GPU: ec_stats_fold through ctypes against tests/stats_ref.py bit for bit on
hand-made records, the layout of ec_moments / ec_stats against the C compiler, the refusals of every stats entry point with no
device present, and csrc/ec_stats_fold.hpp run alone by erased-cells_amd/host/test_stats_fold.cpp — plain and under the
address and undefined-behaviour sanitizers, as a stand-alone program (nothing of it is loaded into Python)."""
import ctypes as C
import math
import os
import struct
import subprocess

import pytest

import stats_ref as R
from host_program import run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    return ec


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def to_moments(E, r):
    """A stats_ref record as the ec_moments the device would have written."""
    m = E.EcMoments()
    m.count = r["count"]
    m.keys2[0] = ~R.order_key(r["dtype"], r["min"])
    m.keys2[1] = R.order_key(r["dtype"], r["max"])
    m.kind, m.dtype = r["kind"], r["dtype"]
    if r["kind"] == 0:
        m.u.i.sum = r["sum"]
        m.u.i.sq_lo, m.u.i.sq_hi = r["sq"] & (2**64 - 1), r["sq"] >> 64
    else:
        m.u.f.pivot, m.u.f.s1, m.u.f.s2 = r["pivot"], r["s1"], r["s2"]
    return m


def fold_through_the_library(ec, records):
    E = ec._ffi
    arr = (E.EcMoments * len(records))(*[to_moments(E, r) for r in records])
    out = E.EcStats()
    st = ec.lib().ec_stats_fold(arr, len(records), C.byref(out))
    assert st == E.EC_OK, ec.lib().ec_last_error_string()
    return out


def assert_same(ec, out, exp, dtype):
    assert out.count == exp["count"]
    for name in ("sum", "mean", "stddev"):
        got, want = getattr(out, name), exp[name]
        assert bits(got) == bits(want) or (math.isnan(got) and math.isnan(want)), (name, got, want)
    mn, mx = ec.CellValue.from_ec(out.min), ec.CellValue.from_ec(out.max)
    assert (mn.ct, mx.ct) == (dtype, dtype)
    as_py = float if dtype in (R.F32, R.F64) else int
    got = [R.order_key(dtype, as_py(v.value)) for v in (mn, mx)]  # by key: equal keys are equal bits, NaN included
    assert got == [R.order_key(dtype, exp["min"]), R.order_key(dtype, exp["max"])], (mn.value, mx.value, exp["min"], exp["max"])


def int_record(dtype, count, total, sq, mn, mx):
    return {"count": count, "kind": 0, "dtype": dtype, "sum": total, "sq": sq, "min": mn, "max": mx}


def f64_record(dtype, count, pivot, s1, s2, mn, mx):
    return {"count": count, "kind": 1, "dtype": dtype, "pivot": pivot, "s1": s1, "s2": s2, "min": mn, "max": mx}


def _empty(dtype):
    return R.record(dtype, [])


def _hex_record(count, pivot, s1, s2, mn, mx):
    f = float.fromhex
    return f64_record(R.F64, count, f(pivot), f(s1), f(s2), f(mn), f(mx))


# Three f64 records found by search: folding them A, B, C and C, B, A differs in the last bit of mean and of stddev.
ORDERED = [_hex_record(4, "0x1.98a94cf1c320fp+13", "-0x1.fb503fcab3af0p+9", "0x1.5cb852abb5b5ap+19", "0x1.7ecabdbaab444p+13", "0x1.98a94cf1c320fp+13"),
           _hex_record(7, "0x1.874394cd8f635p+13", "-0x1.f7ad86e073a40p+10", "0x1.05ace8bb19565p+21", "0x1.686f663880c53p+13", "0x1.941d0dd057ee7p+13"),
           _hex_record(1, "0x1.84388527b6df8p+13", "0x0.0p+0", "0x0.0p+0", "0x1.84388527b6df8p+13", "0x1.84388527b6df8p+13")]
# Three u16 records whose Chan merge would depend on the order: integer records are added exactly first, so theirs does not.
INTEGERS = [int_record(R.U16, 7, 203374, 6236826672, 21821, 41110), int_record(R.U16, 4, 143712, 6740226378, 2827, 54382),
            int_record(R.U16, 2, 53675, 1560333493, 19097, 34578)]

CASES = {
    # 2^31 - 5 cells of i32 near MIN with a few at MAX: the sum of squares needs its high word, the sum is negative
    "i32 sq_hi and a negative sum": [int_record(R.I32, 2**31 - 5, -(2**31) * (2**31 - 8) + 3 * (2**31 - 1),
                                                2**62 * (2**31 - 8) + 3 * (2**31 - 1) ** 2, -2**31, 2**31 - 1)],
    "u32 sq_hi, 2^31 cells": [int_record(R.U32, 2**31, 2**30 * (2**32 - 1) + 2**30 * 7, 2**30 * (2**32 - 1) ** 2 + 2**30 * 49, 7, 2**32 - 1)],
    "i8 negative sum": [R.record(R.I8, [-128, -127, 5, -1, 0, 127])],
    "count 0 alone": [_empty(R.U8)],
    "count 0 alone, f32": [_empty(R.F32)],
    "count 0 between others": [_empty(R.I16), R.record(R.I16, [-300, 7, 9]), _empty(R.I16), R.record(R.I16, [32767, -32768]), _empty(R.I16)],
    "merge order A, B, C": ORDERED,
    "merge order C, B, A": ORDERED[::-1],
    "integer records add exactly": INTEGERS,
    "integer records add exactly, reversed": INTEGERS[::-1],
    # 2^31 + 5 cells: past what one exact u32 record may cover, so the run closes and the two enter the Chan merge
    "u32 run closed at the limit": [int_record(R.U32, 2**31, 2**31 * 1000, 2**31 * 10**6, 1000, 1000), int_record(R.U32, 5, 45, 445, 7, 11),
                                    int_record(R.U32, 3, 6, 14, 1, 3)],
    # s2 - s1 * (s1 / n) < 0: rounding over a near-constant band; the fold sets M2 to 0
    "f32 negative raw M2": [f64_record(R.F32, 3, 0.0, 0.3, 0.03 - 1e-17, 0.1, 0.1)],
    "f64 negative raw M2 inside a merge": [f64_record(R.F64, 3, 1e9, 0.3, 0.03 - 1e-17, 1e9, 1e9 + 0.1), R.record(R.F64, [1e9 + 1, 1e9 + 3])],
    "f64 NaN": [f64_record(R.F64, 4, 2.0, math.nan, math.nan, -1.0, math.nan)],
    "f64 NaN then finite": [f64_record(R.F64, 4, 2.0, math.nan, math.nan, -1.0, 5.0), R.record(R.F64, [1.5, 2.5, -7.0])],
    "f64 pivot 1e9": [R.record(R.F64, [1e9 + k for k in (0, 3, -5, 1024, -1024)])],
    "u64 above 2^63 and i64": [R.record(R.U64, [2**63 + 5, 2**63 + 9, 2**63 - 1000])],
    "i64 negative": [R.record(R.I64, [-(10**9) - 3, -(10**9) + 900, -(10**9)]), R.record(R.I64, [7, 8])],
}


@pytest.mark.parametrize("name", list(CASES))
def test_fold_matches_the_python_restatement_bit_for_bit(ec, name):
    records = CASES[name]
    out = fold_through_the_library(ec, records)
    assert_same(ec, out, R.fold(records), records[0]["dtype"])


def test_the_hand_made_records_are_what_they_claim():
    """The cases above exercise what their names say — in the reference itself, so a fold that ignored sq_hi, the order of the
    records or the clamp could not pass."""
    assert CASES["i32 sq_hi and a negative sum"][0]["sq"] >> 64 and CASES["i32 sq_hi and a negative sum"][0]["sum"] < 0
    assert CASES["u32 sq_hi, 2^31 cells"][0]["sq"] >> 64
    abc, cba = R.fold(ORDERED), R.fold(ORDERED[::-1])
    assert bits(abc["mean"]) != bits(cba["mean"]) and bits(abc["stddev"]) != bits(cba["stddev"])
    assert abs(abc["mean"] - cba["mean"]) < 1e-10 and abc["count"] == cba["count"]
    whole = int_record(R.U16, 13, sum(r["sum"] for r in INTEGERS), sum(r["sq"] for r in INTEGERS), 2827, 54382)
    assert R.fold(INTEGERS) == R.fold(INTEGERS[::-1]) == R.fold([whole])
    closed = CASES["u32 run closed at the limit"]
    assert R.fold(closed)["count"] == 2**31 + 8 and len(R._runs(closed)) == 2 and R._runs(closed)[1]["count"] == 8
    r = CASES["f32 negative raw M2"][0]
    assert r["s2"] - r["s1"] * (r["s1"] / 3.0) < 0.0 and R.fold([r])["stddev"] == 0.0
    assert math.isnan(R.fold(CASES["f64 NaN then finite"])["stddev"])
    e = R.fold([_empty(R.F32)])
    assert e["count"] == 0 and e["sum"] == 0.0 and math.isnan(e["mean"]) and (e["min"], e["max"]) == R.sentinels(R.F32)


def test_small_known_answers(ec):
    """Figures one can check by hand: 2 4 4 4 5 5 7 9 has mean 5 and population stddev 2."""
    out = fold_through_the_library(ec, [R.record(R.U8, [2, 4, 4, 4]), R.record(R.U8, [5, 5, 7, 9])])
    assert (out.count, out.sum, out.mean, out.stddev) == (8, 40.0, 5.0, 2.0)
    assert (ec.CellValue.from_ec(out.min).value, ec.CellValue.from_ec(out.max).value) == (2, 9)
    out = fold_through_the_library(ec, [R.record(R.F64, [1e9 + 1, 1e9 + 2, 1e9 + 3, 1e9 + 4])])
    assert (out.count, out.mean, out.stddev, out.sum) == (4, 1e9 + 2.5, math.sqrt(1.25), 4e9 + 10)


def test_struct_layouts_are_what_the_c_compiler_says(ec, tmp_path):
    E = ec._ffi
    prog = tmp_path / "layout.c"
    fields_m = ["count", "keys2", "kind", "dtype", "u", "u.i.sum", "u.i.sq_lo", "u.i.sq_hi", "u.f.pivot", "u.f.s1", "u.f.s2", "reserved"]
    fields_s = ["count", "min", "max", "sum", "mean", "stddev"]
    fmt = " ".join(["%zu"] * (2 + len(fields_m) + len(fields_s)))
    args = ", ".join(["sizeof(ec_moments)"] + [f"offsetof(ec_moments, {f})" for f in fields_m] +
                     ["sizeof(ec_stats)"] + [f"offsetof(ec_stats, {f})" for f in fields_s])
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "erased_cells.h"\n'
                    f'int main(void) {{ printf("{fmt}\\n", {args}); return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(prog), "-o", str(exe)],
                   check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[:1 + len(fields_m)] == [64, 0, 8, 24, 28, 32, 32, 40, 48, 32, 40, 48, 56]
    assert out[1 + len(fields_m):] == [64, 0, 8, 24, 40, 48, 56]
    # and the ctypes mirror agrees with both
    M, S = E.EcMoments, E.EcStats
    assert C.sizeof(M) == 64 and [getattr(M, f).offset for f in ("count", "keys2", "kind", "dtype", "u", "reserved")] == [0, 8, 24, 28, 32, 56]
    assert [getattr(E._MomentsInt, f).offset for f in ("sum", "sq_lo", "sq_hi")] == [0, 8, 16]
    assert [getattr(E._MomentsF64, f).offset for f in ("pivot", "s1", "s2")] == [0, 8, 16]
    assert C.sizeof(S) == 64 and [getattr(S, f).offset for f in fields_s] == [0, 8, 24, 40, 48, 56]


def test_bad_arguments_are_refused_without_a_device(ec):
    """EC_ERR_ARG comes before anything looks for a device — the cell-count limits of ec_stats_device among them — and a
    well-formed compute call fails loudly (no CPU fallback) where there is none."""
    L, E = ec.lib(), ec._ffi
    rec, out = E.EcMoments(), E.EcStats()
    rec.kind, rec.dtype = 0, R.U8
    # the fold
    assert L.ec_stats_fold(None, 1, C.byref(out)) == E.EC_ERR_ARG and b"ec_stats_fold" in L.ec_last_error_string()
    assert L.ec_stats_fold(C.byref(rec), 1, None) == E.EC_ERR_ARG
    assert L.ec_stats_fold(C.byref(rec), 0, C.byref(out)) == E.EC_ERR_ARG
    assert L.ec_stats_fold(C.byref(rec), -1, C.byref(out)) == E.EC_ERR_ARG
    two = (E.EcMoments * 2)()
    two[0].dtype, two[1].dtype = R.U8, R.I8
    assert L.ec_stats_fold(two, 2, C.byref(out)) == E.EC_ERR_ARG and b"different dtype" in L.ec_last_error_string()
    two[1].dtype, two[1].kind = R.U8, 1
    assert L.ec_stats_fold(two, 2, C.byref(out)) == E.EC_ERR_ARG and b"kind" in L.ec_last_error_string()
    two[0].dtype = two[1].dtype = R.F64  # kind 0 is not f64's
    two[1].kind = 0
    assert L.ec_stats_fold(two, 2, C.byref(out)) == E.EC_ERR_ARG
    two[0].dtype = two[1].dtype = 10
    assert L.ec_stats_fold(two, 2, C.byref(out)) == E.EC_ERR_ARG
    assert L.ec_stats_fold(C.byref(rec), 1, C.byref(out)) == E.EC_OK and out.count == 0
    # a record no launch can have written: more cells than one exact record may cover (its sums could leave their words)
    for dtype, limit in ((R.U8, 2**32), (R.I16, 2**32), (R.U32, 2**31), (R.I32, 2**31)):
        big = E.EcMoments()
        big.kind, big.dtype, big.count = 0, dtype, limit + 1
        assert L.ec_stats_fold(C.byref(big), 1, C.byref(out)) == E.EC_ERR_ARG and b"more cells" in L.ec_last_error_string()
        big.count = limit
        assert L.ec_stats_fold(C.byref(big), 1, C.byref(out)) == E.EC_OK and out.count == limit
    # the device entry points: a fake non-null address is never dereferenced, the refusal comes first
    p = C.c_void_p(0x1000)
    for fn in (L.ec_stats_device, L.ec_stats_compute):
        assert fn(R.U8, None, None, 4, p, None) == E.EC_ERR_ARG and b"null pointer" in L.ec_last_error_string()
        assert fn(R.U8, p, None, 4, None, None) == E.EC_ERR_ARG
        for dtype, limit in ((R.U8, 2**32), (R.I8, 2**32), (R.U16, 2**32), (R.I16, 2**32), (R.U32, 2**31), (R.I32, 2**31)):
            assert fn(dtype, p, None, limit + 1, p, None) == E.EC_ERR_ARG, dtype
            assert b"shard it" in L.ec_last_error_string()
        assert fn(10, p, None, 4, p, None) == E.EC_ERR_UNSUPPORTED_TYPE
    import torch
    if not torch.cuda.is_available():
        for fn in (L.ec_stats_device, L.ec_stats_compute):
            # at the limit, and any size for the f64 kind, the arguments are fine: what is missing is the device
            assert fn(R.U8, p, None, 2**32, p, None) == E.EC_ERR_NOT_INITIALIZED
            assert fn(R.F64, p, None, 2**40, p, None) == E.EC_ERR_NOT_INITIALIZED
            assert fn(R.U8, None, None, 0, p, None) == E.EC_ERR_NOT_INITIALIZED  # n == 0 needs no cells
    n1, p1 = (C.c_size_t * 1)(4), (C.c_void_p * 1)()
    assert L.ec_sharded_stats(None, R.U8, p1, None, n1, C.byref(out)) == E.EC_ERR_ARG and b"null shard group" in L.ec_last_error_string()


def test_fold_header_alone():
    run_host_program("test_stats_fold", passed="all checks passed")


def test_fold_header_under_the_address_and_undefined_behaviour_sanitizers():
    run_host_program("test_stats_fold_san", passed="all checks passed")


def test_offset_data_loses_its_variance_without_the_pivot():
    """Why the pivot is not optional, shown in plain floats: the raw f64 sums of 1e9-offset cells give a variance that is wrong
    in its third digit, the pivoted sums give it to the last."""
    from fractions import Fraction
    cells = [1e9 + r for r in (1.0, -3.0, 5.0, -7.0, 2.0, 400.0, -512.0, 3.0)]
    n = float(len(cells))
    s1 = s2 = 0.0
    for x in cells:
        s1, s2 = s1 + x, s2 + x * x
    raw = (s2 - s1 * (s1 / n)) / n
    true = float(sum(Fraction(x) ** 2 for x in cells) / 8 - (sum(Fraction(x) for x in cells) / 8) ** 2)
    pivoted = R.fold([R.record(R.F64, cells)])["stddev"] ** 2
    assert abs(pivoted - true) <= 1e-12 * true and abs(raw - true) > 1e-4 * true


def test_rust_records_have_the_layout_the_c_compiler_gives(tmp_path):
    """`#[repr(C)]` ec_moments and ec_stats of ffi.rs, field by field, against sizeof / offsetof from gcc: repr(C) lays fields
    out in order at their natural alignment, which is worked out here from the field types."""
    import re
    rs = open(os.path.join(ROOT, "erased-cells_amd", "rust", "erased-cells-hip", "src", "ffi.rs")).read()
    size_align = {"u64": (8, 8), "i64": (8, 8), "f64": (8, 8), "i32": (4, 4), "u32": (4, 4), "ec_value": (16, 8),
                  "[i64;2]": (16, 8), "[u64;3]": (24, 8)}

    def layout(name):
        m = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct %s\s*\{([^}]*)\}" % name, rs)
        assert m, f"ffi.rs lacks #[repr(C)] {name}"
        fields = [(n, re.sub(r"\s+", "", t)) for n, t in re.findall(r"pub (\w+)\s*:\s*([^,\n]+)", re.sub(r"//[^\n]*", "", m.group(1)))]
        at, offsets, align = 0, {}, 1
        for n, t in fields:
            size, al = size_align[t]
            at = (at + al - 1) // al * al
            offsets[n] = at
            at += size
            align = max(align, al)
        return [n for n, _ in fields], offsets, (at + align - 1) // align * align

    c_names = {"ec_moments": {"count": "count", "keys2": "keys2", "kind": "kind", "dtype": "dtype", "moments": "u", "reserved": "reserved"},
               "ec_stats": {k: k for k in ("count", "min", "max", "sum", "mean", "stddev")}}
    prog = tmp_path / "rs_layout.c"
    exprs = []
    for name, fields in c_names.items():
        exprs += [f"sizeof({name})"] + [f"offsetof({name}, {c})" for c in fields.values()]
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "erased_cells.h"\n'
                    'int main(void) { printf("%s\\n", %s); return 0; }\n' % (" ".join(["%zu"] * len(exprs)), ", ".join(exprs)))
    exe = tmp_path / "rs_layout"
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for name, fields in c_names.items():
        order, offsets, size = layout(name)
        assert order == list(fields), (name, order)
        want += [size] + [offsets[f] for f in fields]
    assert got == want, (got, want)
