"""An independent reference for the arithmetic cell rule: `out = f64(l) op f64(r)`, one correctly rounded IEEE 754 operation per
step, with the NaN results of the reference on x86-64.  Plain Python and numpy: neither the library nor the oracle is imported.

The rule (src/value.rs:199-217, `cv_bin_op!`: `(l as f64) op (r as f64)`, compiled to addsd / subsd / mulsd / divsd):
  * widening: integers by `as f64` (round to nearest, ties to even), f32 exactly; an f32 NaN as cvtss2sd does: the sign, the
    payload shifted left by 29 bits, the quiet bit set;
  * a NaN result takes the first NaN operand, quieted; when neither operand is a NaN (an invalid operation) it is the x86 default
    NaN 0xFFF8000000000000;
  * both operands NaN under `+` or `*`: the compiler may swap the operands of a commutative instruction, so either operand,
    quieted, is allowed.  That is the only cell with two answers.

Two forms: `binop_exact` on bit patterns, one cell at a time, in exact rational arithmetic rounded once; `binop_vec` over numpy
arrays, numpy doing the arithmetic of the non-NaN cells.  tests/test_special_cases.py holds the two to each other and the
oracle to both."""
import struct
from fractions import Fraction

import numpy as np

U8, U16, U32, U64, I8, I16, I32, I64, F32, F64 = range(10)
ADD, SUB, MUL, DIV = range(4)
NP_DTYPES = [np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]

SIGN = 1 << 63
QUIET = 1 << 51
EXP = 0x7FF << 52
INF = EXP
DEFAULT_NAN = 0xFFF8000000000000     # what addsd & co. make of an invalid operation
GPU_DEFAULT_NAN = 0x7FF8000000000000  # what the GPU's own instructions make of one


def f64_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def bits_f64(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def is_nan(b: int) -> bool:
    return (b & ~SIGN) > EXP


def quiet(b: int) -> int:
    return b | QUIET


# ---------------------------------------------------------------- widening
def widen_f32_bits(b: int) -> int:
    """The f64 bits of an f32 given by its bits (cvtss2sd)."""
    sign, rest = (b >> 31) << 63, b & 0x7FFFFFFF
    if rest > 0x7F800000:  # NaN: payload << 29, quieted
        return sign | EXP | QUIET | ((rest & 0x7FFFFF) << 29)
    return f64_bits(struct.unpack("<f", struct.pack("<I", b))[0])  # exact: every f32 is an f64


def widen_bits(ct: int, raw: int) -> int:
    """The f64 bits of one cell of type `ct` given by its raw little-endian bits."""
    if ct == F64:
        return raw
    if ct == F32:
        return widen_f32_bits(raw)
    width = 8 * np.dtype(NP_DTYPES[ct]).itemsize
    if ct in (I8, I16, I32, I64) and raw >> (width - 1):
        raw -= 1 << width
    return f64_bits(float(raw))  # int -> float: nearest, ties to even


def widen_vec(a: np.ndarray) -> np.ndarray:
    """The f64 bits (uint64) of an array of any of the ten cell types."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return a.view(np.uint64).copy()
    if a.dtype == np.float32:
        b = a.view(np.uint32).astype(np.uint64)
        nan = (b & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
        with np.errstate(all="ignore"):
            plain = a.astype(np.float64).view(np.uint64)
        made = ((b >> np.uint64(31)) << np.uint64(63)) | np.uint64(EXP | QUIET) | ((b & np.uint64(0x7FFFFF)) << np.uint64(29))
        return np.where(nan, made, plain)
    return a.astype(np.float64).view(np.uint64)


# ---------------------------------------------------------------- one cell, exactly
def _round(q: Fraction) -> int:
    """A non-zero rational rounded once to f64 (nearest, ties to even; int / int is correctly rounded, subnormals included)."""
    try:
        r = float(q)
    except OverflowError:
        return INF | (SIGN if q < 0 else 0)
    if r == 0.0:  # underflow to zero keeps the exact sign
        return SIGN if q < 0 else 0
    return f64_bits(r)


def _invalid(op: int, a: int, b: int) -> bool:
    """IEEE 754-2019 7.2 for operands that are not NaNs."""
    ainf, binf = (a & ~SIGN) == INF, (b & ~SIGN) == INF
    azero, bzero = (a & ~SIGN) == 0, (b & ~SIGN) == 0
    if op == ADD:
        return ainf and binf and (a ^ b) & SIGN != 0      # inf + -inf
    if op == SUB:
        return ainf and binf and (a ^ b) & SIGN == 0      # inf - inf
    if op == MUL:
        return (ainf and bzero) or (azero and binf)        # 0 * inf
    return (ainf and binf) or (azero and bzero)            # inf / inf, 0 / 0


def binop_exact(op: int, a: int, b: int) -> set:
    """The allowed f64 result bits of `a op b` for f64 operand bits."""
    na, nb = is_nan(a), is_nan(b)
    if na and nb and op in (ADD, MUL):
        return {quiet(a), quiet(b)}   # a commutative instruction: the compiler picks the first operand
    if na:
        return {quiet(a)}             # value.rs:199-217 on x86-64: the first NaN operand, quieted
    if nb:
        return {quiet(b)}
    if _invalid(op, a, b):
        return {DEFAULT_NAN}
    if op == SUB:                     # a - b is a + (-b) for everything that is left (IEEE 754 6.3)
        op, b = ADD, b ^ SIGN
    sa, sb = a & SIGN, b & SIGN
    ma, mb = a & ~SIGN, b & ~SIGN
    if op == ADD:
        if ma == INF:
            return {a}
        if mb == INF:
            return {b}
        if ma == 0 and mb == 0:
            return {a if sa == sb else 0}   # like signs keep the sign; +0 + -0 is +0 under round to nearest
        if ma == 0:
            return {b}
        if mb == 0:
            return {a}
        q = Fraction(bits_f64(a)) + Fraction(bits_f64(b))
        return {0} if q == 0 else {_round(q)}  # x + -x is +0 under round to nearest
    sign = sa ^ sb
    if op == MUL:
        if ma == INF or mb == INF:
            return {sign | INF}
        if ma == 0 or mb == 0:
            return {sign}
        return {_round(Fraction(bits_f64(a)) * Fraction(bits_f64(b)))}
    if ma == INF:                     # inf / finite (inf / inf was invalid)
        return {sign | INF}
    if mb == INF:                     # finite / inf
        return {sign}
    if mb == 0:                       # division by zero of a non-zero finite value
        return {sign | INF}
    if ma == 0:
        return {sign}
    return {_round(Fraction(bits_f64(a)) / Fraction(bits_f64(b)))}


# ---------------------------------------------------------------- arrays
def _u64(x) -> np.ndarray:
    return np.asarray(x, dtype=np.uint64)


def nan_vec(b: np.ndarray) -> np.ndarray:
    return (b & np.uint64(~SIGN & (2**64 - 1))) > np.uint64(EXP)


def arith_vec(op: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """numpy's own f64 arithmetic on bit arrays; NaN cells are whatever the host makes of them."""
    x, y = a.view(np.float64), b.view(np.float64)
    with np.errstate(all="ignore"):
        r = x + y if op == ADD else x - y if op == SUB else x * y if op == MUL else x / y
    return r.view(np.uint64)


def binop_vec(op: int, a, b):
    """`binop_exact` over arrays of f64 bits: `(first, second)`, two uint64 arrays; a cell's allowed set is {first, second}, and
    the two differ only where both operands are NaNs of different quieted bits under `+` or `*`."""
    a, b = np.ascontiguousarray(_u64(a)), np.ascontiguousarray(_u64(b))
    a, b = np.broadcast_arrays(a, b)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    r = arith_vec(op, a, b)
    na, nb = nan_vec(a), nan_vec(b)
    q = np.uint64(QUIET)
    first = np.where(nan_vec(r), np.where(na, a | q, np.where(nb, b | q, np.uint64(DEFAULT_NAN))), r)
    second = np.where(na & nb, b | q, first) if op in (ADD, MUL) else first
    return first, second


# ---------------------------------------------------------------- programs
def compress(rows) -> np.ndarray:
    """A stack of alternative results (k, n) with the same per-cell sets in as few rows as the largest set needs."""
    s = np.sort(np.stack(rows), axis=0)
    if len(s) > 1:
        s[1:] = np.where(s[1:] == s[:-1], s[0], s[1:])
        s = np.sort(s, axis=0)
        keep = [0] + [i for i in range(1, len(s)) if (s[i] != s[0]).any()]
        s = s[keep]
    return s


def allowed(alts: np.ndarray, got_bits: np.ndarray) -> np.ndarray:
    """Per cell: is the bit pattern one of the allowed ones?"""
    return (np.atleast_2d(alts) == got_bits).any(axis=0)


def program(streams, scalars, steps):
    """An expression program evaluated step by step.  `streams`: f64 bits per stream, as numpy uint64 arrays (the vector form: the
    result is a (k, n) stack whose columns are the allowed sets) or as lists of ints (the exact form: a list of sets).
    `scalars`: f64 bits; `steps`: `(op, a, b, dst)` with operand references 0.. streams, 4.. registers, 8.. scalars; the value is
    what the last step computed."""
    vector = isinstance(streams[0], np.ndarray)
    n = min(len(s) for s in streams)
    val = {}
    if vector:
        for k, s in enumerate(streams):
            val[k] = np.ascontiguousarray(s[:n], dtype=np.uint64)[None, :]
        for k, c in enumerate(scalars):
            val[8 + k] = np.full((1, n), c, dtype=np.uint64)
    else:
        for k, s in enumerate(streams):
            val[k] = [{int(x)} for x in s[:n]]
        for k, c in enumerate(scalars):
            val[8 + k] = [{int(c)}] * n
    last = None
    for op, ra, rb, dst in steps:
        xa, xb = val[ra], val[rb]
        if vector:
            rows = []
            for pa in xa:
                for pb in xb:
                    rows.extend(binop_vec(op, pa, pb))
            out = compress(rows)
        else:
            out = [set().union(*[binop_exact(op, p, q) for p in sa for q in sb]) for sa, sb in zip(xa, xb)]
        val[4 + dst] = out
        last = 4 + dst
    return val[last]
