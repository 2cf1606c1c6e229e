"""tests/reclass_ref.py is the reference the GPU tests of ec_reclass compare against; this file holds IT to three things that do
not share its code: a scalar transcription of the header's rule (Python integers and struct-packed floats, one cell and one
break at a time), compare_ref.relation — the predicate the oracle holds — for all 100 pairs of types, and numpy.digitize.  Then
the cells worked out by hand in include/erased_cells.h.  Needs no device and not the library."""
import struct

import numpy as np
import pytest

import compare_ref as R
import reclass_ref as Q
from vectors import rand_cells

INF = float("inf")


def scalar_key(u, v):
    """the order key of Python value v as a cell of union type u: integers themselves, floats the total_cmp key of their bits"""
    if Q.NP[u].kind != "f":
        return int(v)
    fmt, n = ("<f", 32) if u == Q.F32 else ("<d", 64)
    b = int.from_bytes(struct.pack(fmt, v), "little")
    s = b - (1 << n) if b >> (n - 1) else b                   # the bits as a signed integer
    return s ^ ((1 << (n - 1)) - 1) if s < 0 else s           # negatives: magnitude reversed (total_cmp)


def scalar_class(t, x, bt, breaks, right):
    """the header's rule for one cell: both sides converted to the union type (numpy scalar casts are the `as` of every widening), compared there"""
    u = Q.union(t, bt)
    with np.errstate(all="ignore"):
        kx = scalar_key(u, Q.NP[u].type(Q.NP[t].type(x)).item())
        c = 0
        for b in breaks:
            kb = scalar_key(u, Q.NP[u].type(Q.NP[bt].type(b)).item())
            c += (kb < kx) if right else (kb <= kx)
    return c


@pytest.mark.parametrize("t", range(Q.NT), ids=Q.NAMES)
def test_against_the_scalar_rule_and_the_oracle_held_predicate(t):
    for bt in range(Q.NT):
        breaks = Q.gpu_tables(t, bt, 9, seed=t)
        with np.errstate(all="ignore"):
            x = np.concatenate([Q.special_cells(t), rand_cells(t, 40, 77 + bt, specials=False), breaks.astype(Q.NP[t])])
        for right in (False, True):
            got = Q.classes(t, x, bt, breaks, right)
            assert got.tolist() == [scalar_class(t, v, bt, breaks, right) for v in x], (Q.NAMES[t], Q.NAMES[bt], right)
            rel = R.GT if right else R.GE
            by_relation = sum(R.relation(rel, t, x, bt, b).astype(np.int32) for b in breaks)
            assert np.array_equal(got, by_relation), (Q.NAMES[t], Q.NAMES[bt], right)
            assert got.min() >= 0 and got.max() <= breaks.size


@pytest.mark.parametrize("t", range(Q.NT), ids=Q.NAMES)
def test_against_numpy_digitize(t):
    """same-type breaks, cells without NaN and without -0.0 (digitize orders by IEEE <)"""
    x = rand_cells(t, 3000, 5, specials=False)
    breaks = np.unique(rand_cells(t, 40, 6, specials=False))
    if Q.NP[t].kind == "f":
        x, breaks = x[~np.isnan(x)] + 0.0, breaks[~np.isnan(breaks)] + 0.0   # + 0.0: no negative zero
        x[::5] = breaks[np.arange(x[::5].size) % breaks.size]
    else:
        x[::5] = breaks[np.arange(x[::5].size) % breaks.size]
    for right in (False, True):
        assert np.array_equal(Q.classes(t, x, t, breaks, right), np.digitize(x, breaks, right=right))


def test_cells_worked_out_by_hand():
    f32 = lambda bits: np.array([bits], np.uint32).view(np.float32)[0]
    pnan, nnan, pz, nz = f32(0x7FC00000), f32(0xFFC00000), np.float32(0.0), np.float32(-0.0)
    # -0.0 < +0.0: a break at +0.0 has -0.0 below it, a break at -0.0 has it at (right: not past) it
    assert Q.classes(Q.F32, [nz, pz], Q.F32, [pz], False).tolist() == [0, 1]
    assert Q.classes(Q.F32, [nz, pz], Q.F32, [nz], False).tolist() == [1, 1]
    assert Q.classes(Q.F32, [nz, pz], Q.F32, [nz], True).tolist() == [0, 1]
    assert Q.classes(Q.F32, [nz, pz], Q.F32, [nz, pz], False).tolist() == [1, 2]
    # +-inf breaks isolate the NaNs: the top class with right = 1, class 0 with right = 0
    x = [nnan, -INF, -1.0, 0.0, INF, pnan]
    assert Q.classes(Q.F32, x, Q.F64, [0.5, INF], True).tolist() == [0, 0, 0, 0, 1, 2]
    assert Q.classes(Q.F32, x, Q.F64, [-INF, 0.5], False).tolist() == [0, 1, 1, 1, 2, 2]
    # u64 2^53 + 1: exact against u64 breaks, Float64 (where it IS 2^53) against f64 and i64 breaks
    big = np.array([2**53, 2**53 + 1, 2**53 + 2], np.uint64)
    assert Q.classes(Q.U64, big, Q.U64, np.array([2**53 + 1], np.uint64), False).tolist() == [0, 1, 1]
    assert Q.classes(Q.U64, big, Q.U64, np.array([2**53 + 1], np.uint64), True).tolist() == [0, 0, 1]
    assert Q.classes(Q.U64, big, Q.F64, [2.0**53], True).tolist() == [0, 0, 1]
    assert Q.classes(Q.U64, big, Q.I64, np.array([2**53 + 1], np.int64), False).tolist() == [1, 1, 1]   # the break is 2^53 too
    # a u8 raster with breaks -1.5, 0.2, 0.7, 255.0, 300.0: an empty class between 0.2 and 0.7, none above 255.0 reached
    b = [-1.5, 0.2, 0.7, 255.0, 300.0]
    assert Q.classes(Q.U8, [0, 1, 2, 254, 255], Q.F64, b, False).tolist() == [1, 3, 3, 3, 4]
    assert Q.classes(Q.U8, [0, 1, 2, 254, 255], Q.F64, b, True).tolist() == [1, 3, 3, 3, 3]
    assert Q.breaks_refusal(Q.U8, Q.F64, b) is None
    assert Q.breaks_refusal(Q.F32, Q.F64, [0.0, float("nan")]) == "NaN"
    assert Q.breaks_refusal(Q.F32, Q.F64, [0.0, 0.0]) == "ascending" and Q.breaks_refusal(Q.F32, Q.F64, [-0.0, 0.0]) is None
    assert Q.breaks_refusal(Q.F32, Q.I64, np.array([2**53, 2**53 + 1], np.int64)) == "ascending"   # equal in Float64
    assert Q.breaks_refusal(Q.I64, Q.I64, np.array([2**53, 2**53 + 1], np.int64)) is None


def test_reclass_output_rule():
    x = np.array([0.1, 0.3, 0.5, 0.9, np.nan], np.float32)
    mask = np.array([1, 0, 1, 1, 0], np.uint8)
    dst, ok = Q.reclass(Q.F32, x, None, Q.F64, [0.2, 0.4], False, Q.I16, [10, -20, 30], valid=[1, 0, 1])
    assert dst.dtype == np.int16 and dst.tolist() == [10, -20, 30, 30, 30] and ok.tolist() == [1, 0, 1, 1, 1]
    dst, ok = Q.reclass(Q.F32, x, mask, Q.F64, [0.2, 0.4], False, Q.I16, [10, -20, 30], valid=[1, 1, 0], nodata=-1)
    assert dst.tolist() == [10, -1, 30, 30, -1] and ok.tolist() == [1, 0, 0, 0, 0]
    assert Q.tile(Q.U8, Q.U8) == 8192 and Q.tile(Q.U16, Q.U8) == 4096 and Q.tile(Q.U8, Q.F64) == 1024
    assert [Q.search_steps(n) for n in (0, 1, 2, 3, 4, 7, 8, 127, 128, 255)] == [0, 1, 2, 2, 3, 3, 4, 7, 8, 8]
