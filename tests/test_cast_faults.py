"""The inputs of tests/test_gpu_cast.py can tell a right cast kernel from a wrong one — checked here without a GPU.

For each mistake a kernel of this family can make, `cast_ref` holds a numpy model of the kernel that makes it; the inputs the GPU
file uses (`gpu_inputs`, `scaled_inputs`, `SCALED_PARAMS`) must contain a cell where the wrong kernel's answer differs from the
right one, for every type pair and mode the mistake applies to.  An input set that passed a faulty model would show nothing on
the GPU either.
"""
import numpy as np
import pytest

import cast_ref as R

FLOATS = (R.F32, R.F64)
ALL_PAIRS = [(st, dt) for st in range(R.NT) for dt in range(R.NT)]
NARROWING = [p for p in ALL_PAIRS if not R.can_fit_into(*p)]


def _applies(kind, st, dt):
    """(pairs, modes) the fault can touch"""
    int_dst = R.is_int(dt)
    if kind == "wrap_where_clamp_is_due":
        return R.is_int(st) and int_dst, (R.ROUND,)
    if kind == "clamp_where_wrap_is_due":
        return R.is_int(st) and int_dst, (R.AS,)
    if kind in ("truncate_where_rounding_is_due", "round_half_even"):
        return st in FLOATS and int_dst, (R.ROUND,)
    if kind == "nan_not_zero":
        return st in FLOATS and int_dst, R.MODES
    if kind == "upper_bound_rounds_up":      # 2^63, 2^64 through f64; 2^31 - 1 (and 2^32 - 1) through f32
        return (st, dt) in ((R.F64, R.I64), (R.F64, R.U64), (R.F32, R.I64), (R.F32, R.U64), (R.F32, R.I32), (R.F32, R.U32)), R.MODES
    if kind == "int64_pair_through_f64":
        return (st, dt) in ((R.I64, R.U64), (R.U64, R.I64)), (R.ROUND,)
    raise KeyError(kind)


@pytest.mark.parametrize("kind", R.CAST_FAULTS)
def test_cast_faults_change_an_answer(kind):
    seen = 0
    for st, dt in NARROWING:
        applies, modes = _applies(kind, st, dt)
        if not applies:
            continue
        x = R.gpu_inputs(st, dt)
        for mode in modes:
            good, bad = R.cast(mode, st, x, dt), R.cast_faulty(kind, mode, st, x, dt)
            assert not R.same_cells(bad, good).all(), (kind, R.NAMES[st], R.NAMES[dt], mode)
            seen += 1
    assert seen


def test_the_two_modes_differ_on_every_narrowing_pair_with_an_integer_destination():
    for st, dt in NARROWING:
        x = R.gpu_inputs(st, dt)
        differ = R.cast(R.AS, st, x, dt).tobytes() != R.cast(R.ROUND, st, x, dt).tobytes()
        assert differ == R.is_int(dt), (R.NAMES[st], R.NAMES[dt])


def test_the_lengths_cover_the_three_paths():
    """n = 2 T + 16 / widest + 1: one unguarded tile at least, a guarded last tile that is not full, and a cell tail."""
    for st, dt in ALL_PAIRS:
        cpl = 16 // R.widest(st, dt)
        tile, n = 256 * 2 * cpl, R.gpu_len(st, dt)
        assert n == R.gpu_inputs(st, dt).size <= 16409
        assert n // tile >= 2 and 0 < (n // cpl) % (256 * 2) and n % cpl == 1


@pytest.mark.parametrize("kind", R.SCALED_FAULTS)
def test_scaled_faults_change_an_answer(kind):
    seen = 0
    for st in R.SCALED_SOURCES:
        for dt in range(R.NT):
            if kind == "widen_through_f32" and st != R.I32:          # the one source whose cells an f32 cannot hold
                continue
            if kind == "fma" and (st, dt) != (R.F64, R.F64):         # the stated case: 0.1 * 10.0 + -1.0 is 0.0, 2^-54 fused
                continue
            x, m = R.scaled_inputs(st, dt)
            nd = R.nodata_of(dt)
            changed = []
            for scale, offset in R.SCALED_PARAMS:
                good = R.scaled(st, x, m, scale, offset, dt, nd)
                bad = R.scaled_faulty(kind, st, x, m, scale, offset, dt, nd)
                changed.append(not R.same_cells(bad, good).all())
            assert any(changed), (kind, R.NAMES[st], R.NAMES[dt])
            if kind == "fma":
                assert changed[0] and 0.1 in x[m == 1]
                good = R.scaled(st, x, m, 10.0, -1.0, dt, nd)
                assert (good[(x == 0.1) & (m == 1)] == 0.0).all()
            seen += 1
    assert seen


def test_a_nan_under_a_cleared_mask_byte_is_among_the_inputs():
    for st in FLOATS:
        for dt in range(R.NT):
            x, m = R.scaled_inputs(st, dt)
            assert (np.isnan(x) & (m == 0)).any() and (np.isnan(x) & (m == 1)).any(), (R.NAMES[st], R.NAMES[dt])
            nd = R.nodata_of(dt)
            out = R.scaled(st, x, m, 10000.0, 0.0, dt, nd)
            assert (out[np.isnan(x) & (m == 0)] == nd).all()
