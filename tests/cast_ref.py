"""A vectorised numpy restatement of ec_cast / ec_cast_scaled (include/erased_cells.h): a cell of one type as a cell of another,
for all 100 ordered pairs.

numpy's float-to-integer `astype` is not defined outside the destination's range, so every such `astype` here comes after a
clamp.  tests/test_cast_ref.py holds `cast` to things it shares no code with (the oracle's convert for the 41 fitting pairs,
resample_ref.to_cell, `cast_scalar` below in Python's exact integers, the whole value space of the small types); the GPU tests
and the stand-alone host program are then held to `cast` and `scaled`.  Also here: the special-values table, the inputs the GPU
tests use, and numpy models of the mistakes a cast kernel can make (tests/test_cast_faults.py).
"""
import math
import struct
from fractions import Fraction

import numpy as np

from compare_ref import F32, F64, I8, I16, I32, I64, NAMES, NP, NT, U8, U16, U32, U64, union

AS, ROUND = 0, 1   # ec_cast_mode
MODES = (AS, ROUND)
CAST_MODE = {"as": AS, "round": ROUND}   # the Python mirror's spellings
FLT_MAX = float(np.finfo(np.float32).max)


def can_fit_into(st: int, dt: int) -> bool:
    """CellType::can_fit_into (src/ctype.rs:129-131)."""
    return union(st, dt) == dt


def is_int(ct: int) -> bool:
    return NP[ct].kind in "ui"


def limits(ct: int):
    info = np.iinfo(NP[ct])
    return int(info.min), int(info.max)


def _saturate(v: np.ndarray, dt: np.dtype) -> np.ndarray:
    """f64 cells as integer cells of dtype dt: truncated toward zero, saturated, NaN -> 0; clamped before the astype.  The 64-bit
    limits are compared in f64 (2^63, 2^64)."""
    info = np.iinfo(dt)
    nan = np.isnan(v)
    if dt.itemsize < 8:
        c = np.clip(np.where(nan, 0.0, v), float(info.min), float(info.max))
        return c.astype(np.int64).astype(dt)
    out = np.zeros(v.shape, dt)
    if dt.kind == "i":
        top, bot = v >= 2.0**63, v <= -2.0**63
        mid = ~(top | bot | nan)
        out[mid] = v[mid].astype(np.int64)
        out[top], out[bot] = info.max, info.min
        return out
    top, pos = v >= 2.0**64, v > 0.0
    mid = pos & ~top
    big = mid & (v >= 2.0**63)              # above the i64 range: moved down by 2^63 (exact), cast, moved up again
    small = mid & ~big
    out[small] = v[small].astype(np.int64).astype(np.uint64)
    out[big] = (v[big] - 2.0**63).astype(np.int64).astype(np.uint64) + np.uint64(2**63)
    out[top] = info.max
    return out


def cast(mode: int, st: int, x, dt: int) -> np.ndarray:
    """dst of ec_cast(mode, st, x, dt)."""
    x = np.asarray(x, dtype=NP[st])
    d = NP[dt]
    with np.errstate(all="ignore"):
        if d.kind == "f" or can_fit_into(st, dt):
            return x.astype(d)                              # a widening, or into f32: round to nearest even, overflow to inf
        if is_int(st):
            if mode == AS:
                return x.astype(d)                          # integer to integer: numpy wraps, as C and Rust `as` do
            (slo, shi), (dlo, dhi) = limits(st), limits(dt)
            return np.clip(x, NP[st].type(max(slo, dlo)), NP[st].type(min(shi, dhi))).astype(d)   # clamped in the source's own integers
        v = x.astype(np.float64)
        if mode == ROUND:
            v = np.trunc(v + np.copysign(0.5, v))           # ONE f64 add, then the truncation
        return _saturate(v, d)


def scaled(st: int, x, mask, scale: float, offset: float, dt: int, nodata=None) -> np.ndarray:
    """dst of ec_cast_scaled: two individually rounded f64 operations (numpy never fuses them), then ROUND; nodata under a cleared mask byte."""
    with np.errstate(all="ignore"):
        y = np.asarray(x, dtype=NP[st]).astype(np.float64) * np.float64(scale)
        y = y + np.float64(offset)
    out = y if dt == F64 else cast(ROUND, F64, y, dt)
    if mask is not None:
        out = np.where(np.asarray(mask).astype(bool), out, NP[dt].type(nodata))
    return out


# ---------------------------------------------------------------- one cell in Python's exact integers
def _f32_of_int(v: int) -> float:
    """v rounded to nearest even at 24 significant bits (no integer cell reaches FLT_MAX)."""
    a = abs(v)
    e = max(a.bit_length() - 24, 0)
    q, r = divmod(a, 1 << e)
    half = (1 << e) >> 1
    if e and (r > half or (r == half and q & 1)):
        q += 1
    return math.copysign(float(q << e), -1.0 if v < 0 else 1.0)


def _f32_of_f64(v: float) -> float:
    if v != v or math.isinf(v):
        return v
    if abs(v) >= 2.0**128 - 2.0**103:       # FLT_MAX plus half its last place, a tie that rounds to even = up: overflow
        return math.copysign(math.inf, v)
    if abs(v) > FLT_MAX:
        return math.copysign(FLT_MAX, v)
    return struct.unpack("<f", struct.pack("<f", v))[0]   # the C conversion of an in-range double


def cast_scalar(mode: int, st: int, v, dt: int):
    """One cell, written for a reader: Python integers and Fractions, no numpy arithmetic.  Returns a numpy scalar of type dt."""
    d = NP[dt]
    if dt == F64:
        return d.type(float(v)) if not is_int(st) else d.type(_f64_of_int(int(v)))
    if dt == F32:
        if is_int(st):
            return d.type(_f32_of_int(int(v)))
        f = float(v)
        if f != f:
            return np.asarray(v).astype(d)[()]    # a NaN stays a NaN of its sign (compared by class and sign)
        return d.type(_f32_of_f64(f))
    lo, hi = limits(dt)
    if is_int(st):
        i = int(v)
        if mode == ROUND or can_fit_into(st, dt):
            return d.type(min(max(i, lo), hi))
        bits = 8 * d.itemsize
        w = i & ((1 << bits) - 1)
        return d.type(w - (1 << bits) if lo < 0 and w >> (bits - 1) else w)
    f = float(v)
    if f != f:
        return d.type(0)
    if math.isinf(f):
        return d.type(hi if f > 0 else lo)
    if mode == ROUND:
        f = f + math.copysign(0.5, f)             # one f64 add, correctly rounded
    return d.type(min(max(math.trunc(Fraction(f)), lo), hi))


def _f64_of_int(v: int) -> float:
    return float(v)   # Python rounds an int to the nearest f64, ties to even


# ---------------------------------------------------------------- the special-values table
def special_reals():
    """The values of the issue's table as exact Python numbers (floats and ints), before they are narrowed to a source type."""
    vals = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999999999999994, -0.49999999999999994, 0.0, -0.0, math.inf, -math.inf,
            5e-324, -5e-324, 2**24 - 1, 2**24 + 1, 2**53 - 1, 2**53 + 1, 2**31, -2**31, 2**63, -2**63, 2**64,
            FLT_MAX, float(np.nextafter(np.float64(FLT_MAX), np.inf)), 0.1, 1, -1, 2**24, 2**53]
    for ct in range(8):
        lo, hi = limits(ct)
        vals += [lo - 1, lo, hi, hi + 1]
        for mid in (Fraction(2 * lo - 1, 2), Fraction(2 * hi + 1, 2)):     # lo - 0.5, hi + 0.5 and their two f64 neighbours
            f = np.float64(float(mid))
            vals += [float(np.nextafter(f, -np.inf)), float(f), float(np.nextafter(f, np.inf))]
    return vals


def specials(st: int) -> np.ndarray:
    """The table as cells of type st: integers keep the values their range holds; floats take every value rounded to the type, the
    two neighbours IN THAT TYPE of every half-way limit, and quiet NaNs of both signs."""
    dt = NP[st]
    if is_int(st):
        lo, hi = limits(st)
        keep = sorted({int(v) for v in special_reals() if isinstance(v, int) or (math.isfinite(v) and float(v).is_integer()) if lo <= int(v) <= hi})
        return np.array(keep, dtype=object).astype(dt)
    with np.errstate(all="ignore"):
        a = np.array([float(v) for v in special_reals()], dtype=np.float64).astype(dt)
        a = np.concatenate([a, np.nextafter(a, dt.type(np.inf)), np.nextafter(a, dt.type(-np.inf))])
    ut = np.uint32 if st == F32 else np.uint64
    nans = [0x7FC00000, 0xFFC00000, 0x7FC12345] if st == F32 else [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000012345678]
    a = np.concatenate([a, np.array(nans, dtype=ut).view(dt)])
    _, first = np.unique(a.view(ut), return_index=True)
    return a[np.sort(first)]


def widest(st: int, dt: int) -> int:
    return max(NP[st].itemsize, NP[dt].itemsize)


def gpu_len(st: int, dt: int) -> int:
    """n = 2 T + 16 / widest + 1 with T = 256 * 2 * (16 / widest): an unguarded tile, the guarded last tile and the cell tail."""
    cpl = 16 // widest(st, dt)
    return 2 * (256 * 2 * cpl) + cpl + 1


def gpu_inputs(st: int, dt: int, seed: int = 0) -> np.ndarray:
    """What tests/test_gpu_cast.py casts: random cells of the whole range with the special values tiled through every other cell,
    and special values in the last cells (the guarded tile's last group and the cell tail)."""
    from vectors import rand_cells
    n = gpu_len(st, dt)
    x = rand_cells(st, n, 9600 + seed, specials=False)
    sp = specials(st)
    x[::2] = sp[np.arange(x[::2].size) % sp.size]
    x[-sp.size:] = sp[:min(sp.size, n)][-n:]
    return x


SCALED_SOURCES = (U8, I16, I32, F32, F64)           # one per byte width, and both float types (a NaN under a cleared mask byte)
# 0.1 * 10.0 + -1.0 is 0.0 in two roundings and 2^-54 fused; (2^24 + 1) * 0.5 - 2^23 is 0.5 -> 1, and 0 when the cell went through f32
SCALED_PARAMS = ((10.0, -1.0), (10000.0, 0.0), (-0.37, 100.25), (0.5, -8388608.0))


def scaled_inputs(st: int, dt: int):
    """(x, mask): gpu_inputs with small magnitudes mixed in (so that the products land inside narrow destinations), a mask that
    clears every NaN among other cells and is set over the last cells."""
    from vectors import rand_mask
    x = gpu_inputs(st, dt, seed=1)
    rng = np.random.default_rng(9700 + st)
    k = np.arange(1, x.size, 4)
    if is_int(st):
        lo, hi = limits(st)
        x[k] = rng.integers(max(lo, -40000), min(hi, 40000), k.size, endpoint=True).astype(NP[st])
    else:
        x[k] = (rng.random(k.size) * 8.0 - 4.0).astype(NP[st])
    m = rand_mask(x.size, 9701)
    if not is_int(st):
        m[np.isnan(x)] = 0
        m[np.flatnonzero(np.isnan(x))[::3]] = 1     # and some NaNs stay valid: they become 0
    m[-5:] = 1
    return x, m


def nodata_of(dt: int):
    """a nodata value no rounding is likely to give: -9999 where the type holds it, else -99 / 255 / 65535"""
    return NP[dt].type(-99 if dt == I8 else -9999 if NP[dt].kind != "u" else 255 if dt == U8 else 65535)


# ---------------------------------------------------------------- fault models: the mistakes a kernel can make
CAST_FAULTS = ("wrap_where_clamp_is_due", "clamp_where_wrap_is_due", "truncate_where_rounding_is_due", "round_half_even",
               "nan_not_zero", "upper_bound_rounds_up", "int64_pair_through_f64")
SCALED_FAULTS = ("widen_through_f32", "fma", "mask_ignored", "nodata_over_valid")


def cast_faulty(kind: str, mode: int, st: int, x, dt: int) -> np.ndarray:
    """`cast` as a kernel with the fault `kind` would compute it (for the pairs and modes the fault can touch)."""
    x = np.asarray(x, dtype=NP[st])
    d = NP[dt]
    right = cast(mode, st, x, dt)
    with np.errstate(all="ignore"):
        if kind == "wrap_where_clamp_is_due":
            return cast(AS, st, x, dt) if mode == ROUND and is_int(st) else right
        if kind == "clamp_where_wrap_is_due":
            return cast(ROUND, st, x, dt) if mode == AS and is_int(st) else right
        if kind == "truncate_where_rounding_is_due":
            return cast(AS, st, x, dt) if mode == ROUND else right
        if is_int(st) and kind == "int64_pair_through_f64":
            return _saturate(x.astype(np.float64), d) if mode == ROUND and is_int(dt) else right
        if is_int(st) or not is_int(dt):
            return right
        v = x.astype(np.float64)
        if kind == "round_half_even":
            return _saturate(np.rint(v), d) if mode == ROUND else right
        r = np.trunc(v + np.copysign(0.5, v)) if mode == ROUND else v
        lo, hi = limits(dt)
        if kind == "nan_not_zero":
            out = right.copy()
            out[np.isnan(v)] = lo if lo < 0 else hi           # what a clamp by fmax / fmin leaves of a NaN
            return out
        if kind == "upper_bound_rounds_up":
            # the upper bound held as a float that rounds up (hi as f64 is 2^63 / 2^64; hi of Int32 as f32 is 2^31): a cell equal
            # to it passes the clamp and overflows the cast, which leaves the "indefinite" value lo (0 for unsigned types)
            bound = float(np.float32(hi)) if st == F32 else float(hi)
            out = right.copy()
            if bound > hi:
                out[r == bound] = lo
            return out
    raise KeyError(kind)


def scaled_faulty(kind: str, st: int, x, mask, scale, offset, dt: int, nodata=None) -> np.ndarray:
    x = np.asarray(x, dtype=NP[st])
    if kind == "mask_ignored":
        return scaled(st, x, None, scale, offset, dt)
    if kind == "nodata_over_valid":
        return scaled(st, x, 1 - np.asarray(mask), scale, offset, dt, nodata)
    with np.errstate(all="ignore"):
        if kind == "widen_through_f32":
            y = x.astype(np.float32).astype(np.float64) * np.float64(scale) + np.float64(offset)
        elif kind == "fma":   # one rounding of the exact a * b + c, cell by cell in Fractions (finite cells only)
            wide = x.astype(np.float64)
            y = wide * np.float64(scale) + np.float64(offset)
            for i in np.flatnonzero(np.isfinite(wide) & np.isfinite(y)):
                exact = Fraction(float(wide[i])) * Fraction(scale) + Fraction(offset)
                y[i] = float(exact) if exact != 0 else y[i]
        else:
            raise KeyError(kind)
    out = y if dt == F64 else cast(ROUND, F64, y, dt)
    if mask is not None:
        out = np.where(np.asarray(mask).astype(bool), out, NP[dt].type(nodata))
    return out


def same_cells(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """Per cell: bit-equal, or — for a float destination where the restatement itself is a NaN — a NaN of the same sign."""
    ut = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    g, w = np.ascontiguousarray(got).view(ut), np.ascontiguousarray(want).view(ut)
    ok = g == w
    if want.dtype.kind == "f":
        sign = ut(1) << ut(8 * want.dtype.itemsize - 1)
        ok |= np.isnan(want) & np.isnan(got.view(want.dtype)) & ((g & sign) == (w & sign))
    return ok
