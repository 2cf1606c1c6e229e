"""Python host mirror of the reference's buffer API over the C ABI.

Same names, argument meaning and error behaviour as `CellBuffer` /
`MaskedCellBuffer` / `Mask` / `NoData` / `CellValue` / `CellType`
(src/buffer.rs, src/masked/*.rs, src/value.rs, src/ctype.rs), so that the parity
tests read like the reference's own tests.  Buffers live in HBM between
operations (`from_vec` uploads once, `to_vec` downloads); every operator body is
one call into liberased_cells_hip.so.  The host keeps what the reference's host
code keeps: the dtype-erased dispatch tag, zip truncation (src/buffer.rs:327),
the empty-result-is-UInt8 rule (src/buffer.rs:233-234) and the length asserts.

This module is test/bench plumbing; the compiled host mirror is
erased-cells_amd/host/erased_cells.hpp and the Rust binding is in INTEGRATION.md.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import fractions
from typing import Callable, Optional, Sequence

import numpy as np

from ._ffi import EC_CAST_AS, EC_CAST_ROUND, EC_COMPOSITE_MAX_LAYERS, EC_DISTANCE_UNLIMITED, EC_REGIONS_DENSE, EC_REGIONS_ROOT, EC_RANK_LOWER, EC_RANK_MAX_DEN, EC_RANK_UPPER, EC_CMP_EQ, EC_CMP_GE, EC_CMP_GT, EC_CMP_LE, EC_CMP_LT, EC_CMP_NE, EC_ERR_ARG, EC_FOCAL_MAX, EC_FOCAL_MEAN, EC_FOCAL_MIN, EC_FOCAL_NORMALIZE, EC_FOCAL_RADIUS_CAP, EC_FOCAL_SUM, EC_FOCAL_WHOLE, EC_RESAMPLE_AVERAGE, EC_ZONAL_MAX_ZONES, EC_ZONAL_TABLE_MAX_ZONES, EC_RECLASS_DROPS, EC_RECLASS_HAS_NODATA, EC_RECLASS_MAX_BREAKS, EC_RECLASS_TABLE_BYTES, EC_RESAMPLE_BILINEAR, EcError, EcReclassTable, EcStats, EcValue, check, lib

# CellType (src/ctype.rs:11-20; order of with_ct!, src/lib.rs:89-98)
UInt8, UInt16, UInt32, UInt64, Int8, Int16, Int32, Int64, Float32, Float64 = range(10)
CELL_TYPES = list(range(10))
CT_NAMES = ["UInt8", "UInt16", "UInt32", "UInt64", "Int8", "Int16", "Int32", "Int64", "Float32", "Float64"]
NP_DTYPES = [np.dtype(d) for d in (np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16, np.int32,
                                   np.int64, np.float32, np.float64)]
ADD, SUB, MUL, DIV = range(4)

_stream: Optional[int] = None  # hipStream_t handle; None = default stream


def init(device: int = 0) -> None:
    check(lib().ec_init(device))


def set_stream(handle: Optional[int]) -> None:
    """Route subsequent launches to `handle` (e.g. torch.cuda.current_stream().cuda_stream)."""
    global _stream
    _stream = handle


def stream() -> Optional[int]:
    return _stream


def synchronize() -> None:
    check(lib().ec_stream_sync(_stream))


def cell_type_of(dtype) -> int:
    dt = np.dtype(dtype)
    for i, d in enumerate(NP_DTYPES):
        if d == dt:
            return i
    raise TypeError(f"no CellType for dtype {dt}")  # e.g. isize is not CellEncoding (encoding.rs:5-8)


def union(a: int, b: int) -> int:
    return lib().ec_union(a, b)


def can_fit_into(a: int, b: int) -> bool:
    return bool(lib().ec_can_fit_into(a, b))


class ParseError(ValueError):
    """Error::ParseError (src/error.rs, raised by `CellType::from_str`, src/ctype.rs:29-44)."""


def cell_type_to_string(ct: int) -> str:  # Display == Debug (ctype.rs:22-27)
    return CT_NAMES[ct]


def cell_type_from_str(s: str) -> int:  # ctype.rs:29-44
    for ct in CELL_TYPES:
        if CT_NAMES[ct] == s:
            return ct
    raise ParseError(f"Unable to parse '{s}' as CellType")


def is_integral(ct: int) -> bool:  # ctype.rs:55-69
    return NP_DTYPES[ct].kind in "ui"


def is_signed(ct: int) -> bool:  # ctype.rs:71-85
    return NP_DTYPES[ct].kind in "if"


def size_of(ct: int) -> int:  # ctype.rs:87-96
    return lib().ec_size_of(ct)


def min_value(ct: int) -> "CellValue":  # ctype.rs:158-167
    out = EcValue()
    check(lib().ec_min_value(ct, C.byref(out)))
    return CellValue.from_ec(out)


def max_value(ct: int) -> "CellValue":  # ctype.rs:170-179
    out = EcValue()
    check(lib().ec_max_value(ct, C.byref(out)))
    return CellValue.from_ec(out)


def zero(ct: int) -> "CellValue":  # ctype.rs:134-144
    return CellValue(ct, 0)


def one(ct: int) -> "CellValue":  # ctype.rs:146-156
    return CellValue(ct, 1)


# --------------------------------------------------------------------------- CellValue
def rust_debug(x) -> str:
    """`format!("{:?}", x)` of a Rust primitive: integers plain; floats as the shortest digits that round-trip
    for their width, decimal with at least one fractional digit for 1e-4 <= |x| < 1e16 (and zero), scientific
    (`1e16`, `1.5e-7`) outside, `NaN` / `inf` / `-inf`; bools `true` / `false`."""
    if isinstance(x, (bool, np.bool_)):
        return "true" if x else "false"
    if isinstance(x, (int, np.integer)):
        return str(int(x))
    x = x if isinstance(x, np.floating) else np.float64(x)
    if np.isnan(x):
        return "NaN"
    if np.isinf(x):
        return "inf" if x > 0 else "-inf"
    ax = abs(float(x))
    if ax == 0.0 or 1e-4 <= ax < 1e16:
        return np.format_float_positional(x, unique=True, trim="0")
    mant, exp = np.format_float_scientific(x, unique=True, trim="-").split("e")
    return f"{mant}e{int(exp)}"


def elided(values) -> str:
    """`Elided` (src/lib.rs:165-192): more than 10 items render as the first five, `, ... `, the last five."""
    items = [rust_debug(v) for v in values]
    if len(items) > 10:
        return ", ".join(items[:5]) + ", ... " + ", ".join(items[-5:])
    return ", ".join(items)


def _ends(n: int, fetch):
    """The cells a Debug rendering shows: all of them up to 10, else only the first and last five are downloaded."""
    if n <= 10:
        return list(fetch(0, n))
    return list(fetch(0, 5)) + [None] + list(fetch(n - 5, 5))


def _elided_ends(n: int, fetch) -> str:
    vals = _ends(n, fetch)
    if n > 10:
        return elided(vals[:5]) + ", ... " + elided(vals[6:])
    return elided(vals)


class CellValue:
    """Scalar with a run-time cell type (src/value.rs:12-20)."""

    __slots__ = ("ct", "value")

    def __init__(self, ct: int, value):
        self.ct = ct
        self.value = value if isinstance(value, np.generic) and value.dtype == NP_DTYPES[ct] else \
            np.array([value]).astype(NP_DTYPES[ct])[0]

    @staticmethod
    def new(x, ct: Optional[int] = None) -> "CellValue":
        """`x.into()`: numpy scalars keep their type; Python ints are i32, floats f64 (Rust literal defaults)."""
        if isinstance(x, CellValue):
            return x
        if ct is not None:
            return CellValue(ct, x)
        if isinstance(x, np.generic):
            return CellValue(cell_type_of(x.dtype), x)
        if isinstance(x, bool):
            raise TypeError("bool is not a CellEncoding")
        if isinstance(x, int):
            if not -2**31 <= x < 2**31:  # a Rust integer literal defaults to i32 and does not compile out of range
                raise OverflowError(f"literal out of range for `i32`: {x} (pass a numpy scalar of the intended type)")
            return CellValue(Int32, x)
        if isinstance(x, float):
            return CellValue(Float64, x)
        raise TypeError(f"cannot convert {type(x)} into CellValue")

    def cell_type(self) -> int:
        return self.ct

    def bits(self) -> int:
        return int.from_bytes(np.array([self.value], dtype=NP_DTYPES[self.ct]).tobytes(), "little")

    def to_ec(self) -> EcValue:
        v = EcValue()
        v.dtype = self.ct
        v.v.bits = self.bits()
        return v

    @staticmethod
    def from_ec(v: EcValue) -> "CellValue":
        n = NP_DTYPES[v.dtype].itemsize
        raw = int(v.v.bits & ((1 << (8 * n)) - 1)).to_bytes(n, "little")
        return CellValue(v.dtype, np.frombuffer(raw, dtype=NP_DTYPES[v.dtype])[0])

    def convert(self, ct: int) -> "CellValue":
        """CellValue::convert (value.rs:74-98): NarrowingError unless can_fit_into."""
        out = EcValue()
        src = self.to_ec()
        check(lib().ec_value_convert(C.byref(src), ct, C.byref(out)))
        return CellValue.from_ec(out)

    def get(self, ct: int):
        return self.convert(ct).value

    def to_f64(self) -> float:
        src = self.to_ec()
        return lib().ec_value_to_f64(C.byref(src))

    def _key(self, ct: int) -> int:
        c = self.convert(ct)
        if NP_DTYPES[ct].kind != "f":
            return int(c.value)
        n = NP_DTYPES[ct].itemsize * 8
        b = c.bits()
        if b >> (n - 1):
            b = b - (1 << n)  # as signed
            b ^= (1 << (n - 1)) - 1
        return b

    def cmp(self, other: "CellValue") -> int:
        """impl Ord for CellValue (value.rs:248-265): unify, ints natural, floats total_cmp."""
        ct = union(self.ct, other.ct)
        a, b = self._key(ct), other._key(ct)
        return (a > b) - (a < b)

    def __eq__(self, other):
        return self.cmp(CellValue.new(other)) == 0

    def __lt__(self, other):
        return self.cmp(CellValue.new(other)) < 0

    def __hash__(self):
        return hash((self.ct, self.bits()))

    def __gt__(self, other):
        return self.cmp(CellValue.new(other)) > 0

    def unify(self, other: "CellValue") -> tuple["CellValue", "CellValue"]:
        """value.rs:103-107: both converted to the union of their cell types."""
        ct = union(self.ct, other.ct)
        return self.convert(ct), other.convert(ct)

    @staticmethod
    def zero() -> "CellValue":  # num_traits::Zero (value.rs:166-170)
        return CellValue(UInt8, 0)

    @staticmethod
    def one() -> "CellValue":  # num_traits::One (value.rs:159-164)
        return CellValue(UInt8, 1)

    def is_zero(self) -> bool:  # value.rs:172-174
        return self.to_f64() == 0.0

    def _scalar_op(self, other, fn) -> "CellValue":
        """cv_bin_op! (value.rs:199-217): both sides as f64, result always Float64.  Scalar arithmetic stays on the
        host as in the reference (IEEE double arithmetic of the host CPU; the buffers' per-cell form runs on the GPU)."""
        a, b = np.float64(self.to_f64()), np.float64(CellValue.new(other).to_f64())
        with np.errstate(all="ignore"):
            return CellValue(Float64, fn(a, b))

    def __add__(self, other): return self._scalar_op(other, lambda a, b: a + b)
    def __sub__(self, other): return self._scalar_op(other, lambda a, b: a - b)
    def __mul__(self, other): return self._scalar_op(other, lambda a, b: a * b)
    def __truediv__(self, other): return self._scalar_op(other, lambda a, b: a / b)

    def __neg__(self) -> "CellValue":
        """impl Neg for CellValue (value.rs:224-240): u8 -> i16, u16 -> i32, u32/u64 -> f64, signed wrap, floats flip."""
        out_ct = lib().ec_neg_result_type(self.ct)
        dt = NP_DTYPES[out_ct]
        with np.errstate(all="ignore"):
            if dt.kind == "f":
                return CellValue(out_ct, -dt.type(self.value))
            return CellValue(out_ct, (np.array([self.value]).astype(dt) * dt.type(-1))[0])  # wrapping at MIN

    def __repr__(self):  # derived Debug: `Int32(37)`
        return f"{CT_NAMES[self.ct]}({rust_debug(self.value)})"


# --------------------------------------------------------------------------- device memory
class DeviceMem:
    """An HBM allocation (ec_alloc/ec_free), or a window into one (shards)."""

    _GLOBAL = object()

    def __init__(self, nbytes: int, _parent: "DeviceMem" = None, _offset: int = 0, stream=_GLOBAL):
        """`stream`: allocate (and later free) on this explicit stream — for callers that drive the ABI themselves on
        their own stream (e.g. one stream per host thread); default: the module's current stream (set_stream)."""
        self.nbytes = nbytes
        self._parent = _parent
        if _parent is not None:
            self.ptr = (_parent.ptr or 0) + _offset if nbytes else None
            self._owned = False
        else:
            p = C.c_void_p()
            self._explicit = stream is not DeviceMem._GLOBAL
            self._alloc_stream = stream if self._explicit else _stream  # the block goes back to the pool on this stream
            check(lib().ec_alloc_async(C.byref(p), nbytes, self._alloc_stream))  # stream-ordered pool: no per-op hipMalloc
            self.ptr = p.value
            self._owned = True

    def window(self, offset: int, nbytes: int) -> "DeviceMem":
        assert 0 <= offset and offset + nbytes <= self.nbytes
        return DeviceMem(nbytes, _parent=self, _offset=offset)

    def __del__(self):
        # The free is queued on the ALLOCATING stream, ordered (event + wait, inside ec_free_ordered) after everything
        # enqueued so far on the stream that is current now — the stream this buffer's last operator ran on when
        # the caller switched streams with set_stream() in between.  Freeing on "whatever stream is current" alone
        # would let the pool hand the block out again while kernels on the other stream still use it.
        if getattr(self, "_owned", False) and self.ptr:
            try:
                lib().ec_free_ordered(self.ptr, self._alloc_stream, self._alloc_stream if self._explicit else _stream)
            except Exception:
                pass
            self.ptr = None


def _upload(a: np.ndarray) -> DeviceMem:
    a = np.ascontiguousarray(a)
    mem = DeviceMem(a.nbytes)
    if a.nbytes:
        check(lib().ec_upload(mem.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, _stream))
    return mem


def _download(mem: DeviceMem, dtype, n: int) -> np.ndarray:
    out = np.empty(n, dtype=dtype)
    if out.nbytes:
        check(lib().ec_download(out.ctypes.data_as(C.c_void_p), mem.ptr, out.nbytes, _stream))
    return out


def _window_args(n: int, cols: int, window, window_size, size):
    """(rows, x, y, w, h, out_w, out_h) of a window call on a buffer of n cells read as rows of `cols` cells."""
    if cols < 0 or (cols == 0 and n != 0) or (cols and n % cols):
        raise AssertionError(f"a buffer of {n} cells is not a raster of rows of {cols} cells")
    (x, y), (w, h) = window, window_size
    out_w, out_h = (w, h) if size is None else size
    if min(x, y, w, h, out_w, out_h) < 0:
        raise EcError(EC_ERR_ARG, f"negative window: offset {(x, y)}, size {(w, h)}, output {(out_w, out_h)}")
    return (n // cols if cols else 0), x, y, w, h, out_w, out_h


# the names gdal::raster::ResampleAlg gives the algorithms ec_window_resample has (None: GDAL's default, nearest neighbour)
RESAMPLE_ALGS = {"Bilinear": EC_RESAMPLE_BILINEAR, "Average": EC_RESAMPLE_AVERAGE}


def _resample_alg(resample):
    """None for `resample` None / "NearestNeighbour" (ec_window), the ec_resample number of "Bilinear" / "Average"; any other name is refused"""
    if resample is None or resample == "NearestNeighbour":
        return None
    if resample not in RESAMPLE_ALGS:
        raise EcError(EC_ERR_ARG, f"window: resampling algorithm {resample!r} is not one of NearestNeighbour, Bilinear, Average")
    return RESAMPLE_ALGS[resample]


def _cut(alg, *args) -> None:
    """ec_window(*args), or ec_window_resample(alg, *args) when `alg` (_resample_alg) names an algorithm"""
    check(lib().ec_window(*args, _stream) if alg is None else lib().ec_window_resample(alg, *args, _stream))


def _scalar(x) -> CellValue:
    return CellValue.new(x)


# the spellings of an ec_cmp relation: the truth table over Ordering (bit 0 Less, bit 1 Equal, bit 2 Greater)
RELATIONS = {"<": EC_CMP_LT, "==": EC_CMP_EQ, "<=": EC_CMP_LE, ">": EC_CMP_GT, "!=": EC_CMP_NE, ">=": EC_CMP_GE}


def _relation(rel) -> int:
    """the ec_cmp number of "<" "<=" ">" ">=" "==" "!=" or of an ec_cmp value; anything else is refused"""
    r = RELATIONS.get(rel, rel) if isinstance(rel, str) else rel
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 1 <= int(r) <= 6:
        raise EcError(EC_ERR_ARG, f"compare: relation {rel!r} is not one of {sorted(RELATIONS)} or an ec_cmp value 1..6")
    return int(r)


def _compare(rel, lhs: "CellBuffer", lmask, rhs, rmask=None) -> "Mask":
    """ec_compare / ec_compare_scalar of `lhs` against a buffer or a scalar, ANDed with the masks given, into a new Mask"""
    r = _relation(rel)
    if isinstance(rhs, CellBuffer):
        n = min(lhs.n, rhs.n)  # zip (buffer.rs:327)
        out = Mask.empty(n)
        check(lib().ec_compare(r, lhs.ct, lhs.mem.ptr, lmask.mem.ptr if lmask else None, rhs.ct, rhs.mem.ptr,
                               rmask.mem.ptr if rmask else None, n, out.mem.ptr, _stream))
        return out
    v = _scalar(rhs).to_ec()
    out = Mask.empty(lhs.n)
    check(lib().ec_compare_scalar(r, lhs.ct, lhs.mem.ptr, lmask.mem.ptr if lmask else None, lhs.n, C.byref(v), out.mem.ptr, _stream))
    return out


# the spellings of an ec_cast_mode
CAST_MODES = {"as": EC_CAST_AS, "round": EC_CAST_ROUND}


def _cast_mode(mode) -> int:
    """the ec_cast_mode number of "as" / "round" or of an ec_cast_mode value; anything else is refused"""
    m = CAST_MODES.get(mode, mode) if isinstance(mode, str) else mode
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or int(m) not in (EC_CAST_AS, EC_CAST_ROUND):
        raise EcError(EC_ERR_ARG, f"cast: mode {mode!r} is not one of {sorted(CAST_MODES)} or an ec_cast_mode value")
    return int(m)


def _to_scaled(buf: "CellBuffer", mask, ct: int, scale, offset, nd) -> "CellBuffer":
    """ec_cast_scaled of `buf` (with `mask` and the nodata CellValue `nd`, or neither) into a new buffer of type ct"""
    out = CellBuffer.empty(buf.n, ct)
    ev = nd.to_ec() if nd is not None else None
    check(lib().ec_cast_scaled(buf.ct, buf.mem.ptr, mask.mem.ptr if ev is not None else None, buf.n, float(scale), float(offset), ct,
                               C.byref(ev) if ev is not None else None, out.mem.ptr, _stream))
    return out


# the spellings of an ec_focal_op
FOCAL_OPS = {"sum": EC_FOCAL_SUM, "mean": EC_FOCAL_MEAN, "min": EC_FOCAL_MIN, "max": EC_FOCAL_MAX}


def _focal_op(op) -> int:
    """the ec_focal_op number of "sum" "mean" "min" "max" or of an ec_focal_op value; anything else is refused"""
    o = FOCAL_OPS.get(op, op) if isinstance(op, str) else op
    if isinstance(o, bool) or not isinstance(o, (int, np.integer)) or not 0 <= int(o) <= 3:
        raise EcError(EC_ERR_ARG, f"focal: operation {op!r} is not one of {sorted(FOCAL_OPS)} or an ec_focal_op value 0..3")
    return int(o)


def _raster_rows(n: int, cols: int) -> int:
    if cols < 0 or (cols == 0 and n != 0) or (cols and n % cols):
        raise AssertionError(f"a buffer of {n} cells is not a raster of rows of {cols} cells")
    return n // cols if cols else 0


def _max_sq(max_distance) -> int:
    """ec_distance's max_sq of a greatest distance: floor(max_distance^2), exact through Fraction (an int, a float or a Fraction);
    None, infinity and everything from 2^16 cells on — beyond any raster's diagonal — is EC_DISTANCE_UNLIMITED"""
    if max_distance is None or max_distance == float("inf"):
        return EC_DISTANCE_UNLIMITED
    if isinstance(max_distance, bool) or max_distance != max_distance or max_distance < 0:
        raise EcError(EC_ERR_ARG, f"distance: the greatest distance {max_distance!r} is not a number >= 0")
    sq = fractions.Fraction(max_distance) ** 2
    return min(sq.numerator // sq.denominator, EC_DISTANCE_UNLIMITED)


def _regions(buf, mask, n: int, cols: int, connectivity: int, min_cells: int, numbering, labels: bool):
    """ec_regions of `buf` (or None: the mask form) under `mask` (or None) read as rows of `cols` cells, with the workspace from the
    library's pool -> (MaskedCellBuffer of Int32 labels, K), or with `labels` False — the sieve-only form — the Mask of the kept cells."""
    if isinstance(numbering, str):
        if numbering not in ("root", "dense"):
            raise EcError(EC_ERR_ARG, f"regions: the numbering {numbering!r} is neither 'root' nor 'dense'")
        numbering = EC_REGIONS_DENSE if numbering == "dense" else EC_REGIONS_ROOT
    if isinstance(min_cells, bool) or int(min_cells) != min_cells or not 0 <= min_cells < 1 << 64:
        raise EcError(EC_ERR_ARG, f"regions: min_cells {min_cells!r} is not an integer within 0 .. 2^64 - 1")
    rows = _raster_rows(n, cols)
    out = CellBuffer.empty(n, Int32) if labels else None
    om = Mask.empty(n)
    k = CellBuffer.empty(1, UInt64) if labels else None
    if n:  # an empty raster has no memory to point at, and no region
        check(lib().ec_regions(buf.ct if buf is not None else UInt8, buf.mem.ptr if buf is not None else None, mask.mem.ptr if mask is not None else None,
                               cols, rows, int(connectivity), int(numbering), int(min_cells), out.mem.ptr if labels else None, om.mem.ptr,
                               k.mem.ptr if labels else None, None, _stream))
    if not labels:
        return om
    return MaskedCellBuffer(out, om), (int(k.to_numpy()[0]) if n else 0)


def _radius(radius):
    rx, ry = radius
    if not 0 <= min(rx, ry) <= max(rx, ry) <= EC_FOCAL_RADIUS_CAP:  # here, not in C: a radius of 2^32 + 1 would arrive there as 1
        raise EcError(EC_ERR_ARG, f"focal: radius {(rx, ry)} is not within 0 .. EC_FOCAL_RADIUS_CAP ({EC_FOCAL_RADIUS_CAP})")
    return int(rx), int(ry)


def _focal(buf: "CellBuffer", mask, cols: int, op, radius, whole: bool):
    """ec_focal of `buf` (under `mask`, or None) read as rows of `cols` cells -> (result buffer, result Mask or None).  A mask comes back
    when there is a source mask or `whole` is set: only then can a cell be invalid."""
    o, (rx, ry), rows = _focal_op(op), _radius(radius), _raster_rows(buf.n, cols)
    out = CellBuffer.empty(buf.n, lib().ec_focal_result_type(o, buf.ct))
    om = Mask.empty(buf.n) if (mask is not None or whole) else None
    if buf.n:  # an empty buffer has no memory to point at
        check(lib().ec_focal(o, buf.ct, buf.mem.ptr, mask.mem.ptr if mask is not None else None, cols, rows, rx, ry, EC_FOCAL_WHOLE if whole else 0,
                             out.mem.ptr, om.mem.ptr if om is not None else None, _stream))
    return out, om


def _convolve(buf: "CellBuffer", mask, cols: int, weights, normalize: bool, whole: bool):
    """ec_focal_convolve with the 2-D `weights` (odd shape (2 ry + 1, 2 rx + 1)) -> (Float64 buffer, Mask or None).  With `normalize`
    and no mask back, a cell whose counted weights sum to 0.0 holds zero bits (include/erased_cells.h)."""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.ndim != 2 or w.shape[0] % 2 == 0 or w.shape[1] % 2 == 0:
        raise EcError(EC_ERR_ARG, f"convolve: weights of shape {w.shape} are not a 2-D array of odd shape")
    rx, ry = _radius((w.shape[1] // 2, w.shape[0] // 2))
    rows = _raster_rows(buf.n, cols)
    out = CellBuffer.empty(buf.n, Float64)
    om = Mask.empty(buf.n) if (mask is not None or whole) else None
    flags = (EC_FOCAL_WHOLE if whole else 0) | (EC_FOCAL_NORMALIZE if normalize else 0)
    if buf.n:
        check(lib().ec_focal_convolve(buf.ct, buf.mem.ptr, mask.mem.ptr if mask is not None else None, cols, rows, w.ctypes.data_as(C.POINTER(C.c_double)),
                                      rx, ry, flags, out.mem.ptr, om.mem.ptr if om is not None else None, _stream))
    return out, om


def _focal_rank(buf: "CellBuffer", mask, cols: int, q, method, radius, whole: bool):
    """ec_focal_rank, or ec_focal_majority when `q` is None, of `buf` (under `mask`, or None) read as rows of `cols` cells ->
    (result buffer of the same cell type, result Mask or None), as `_focal` gives them for "min"."""
    num, den, m = _rank_args(q, method, "focal_rank") if q is not None else (0, 1, 0)
    (rx, ry), rows = _radius(radius), _raster_rows(buf.n, cols)
    out = CellBuffer.empty(buf.n, buf.ct)
    om = Mask.empty(buf.n) if (mask is not None or whole) else None
    flags = EC_FOCAL_WHOLE if whole else 0
    if buf.n:  # an empty buffer has no memory to point at
        sm, dm = (mask.mem.ptr if mask is not None else None), (om.mem.ptr if om is not None else None)
        if q is not None:
            check(lib().ec_focal_rank(buf.ct, buf.mem.ptr, sm, cols, rows, rx, ry, num, den, m, flags, out.mem.ptr, dm, _stream))
        else:
            check(lib().ec_focal_majority(buf.ct, buf.mem.ptr, sm, cols, rows, rx, ry, flags, out.mem.ptr, dm, _stream))
    return out, om


# --------------------------------------------------------------------------- CellBuffer
@dataclasses.dataclass(frozen=True)
class Stats:
    """Band statistics of one pass over a resident buffer (`ec_stats_compute`): `min` / `max` as `min_max()` gives them, `stddev` the
    population one (divided by `count`), as GDAL's STATISTICS_STDDEV (src/gdal/rasterband.rs:151-156).  With `count == 0`: the
    sentinels, `sum == 0.0`, `mean` and `stddev` NaN."""
    count: int
    min: "CellValue"
    max: "CellValue"
    sum: float
    mean: float
    stddev: float

    @staticmethod
    def from_ec(s: EcStats) -> "Stats":
        return Stats(int(s.count), CellValue.from_ec(s.min), CellValue.from_ec(s.max), float(s.sum), float(s.mean), float(s.stddev))


class CellBuffer:
    """Device-resident `CellBuffer` (src/buffer.rs:12-55): a cell type tag + n cells in HBM."""

    def __init__(self, ct: int, n: int, mem: DeviceMem):
        self.ct, self.n, self.mem = ct, n, mem

    # ---- constructors (BufferOps, src/lib.rs:104-163)
    @staticmethod
    def from_vec(data) -> "CellBuffer":
        a = np.ascontiguousarray(data)
        if a.dtype == np.dtype(np.int64) and not isinstance(data, np.ndarray):
            if a.size and (a.min() < -2**31 or a.max() >= 2**31):
                raise OverflowError("literal out of range for `i32` (pass a numpy array of the intended type)")
            a = a.astype(np.int32)  # Rust integer literals default to i32
        return CellBuffer(cell_type_of(a.dtype), a.size, _upload(a.ravel()))

    new = from_vec

    @staticmethod
    def from_values(values) -> "CellBuffer":
        """impl FromIterator<CellValue> for CellBuffer (src/buffer.rs:229-250): empty -> UInt8; otherwise the
        FIRST value's cell type, every value through `get::<T>().unwrap()` (a value that does not fit panics)."""
        vals = [CellValue.new(v) for v in values]
        if not vals:
            return CellBuffer.with_defaults(0, UInt8)
        ct = vals[0].ct
        return CellBuffer.from_vec(np.array([v.get(ct) for v in vals], dtype=NP_DTYPES[ct]))

    def __iter__(self):
        """impl IntoIterator for &CellBuffer (src/buffer.rs:278-305): yields CellValue; one download for the walk."""
        return (CellValue(self.ct, v) for v in self.to_numpy())

    @staticmethod
    def with_defaults(length: int, ct: int) -> "CellBuffer":
        return CellBuffer.fill(length, CellValue(ct, 0))

    @staticmethod
    def fill(length: int, value) -> "CellBuffer":
        v = _scalar(value)
        mem = DeviceMem(length * NP_DTYPES[v.ct].itemsize)
        ev = v.to_ec()
        check(lib().ec_fill(v.ct, mem.ptr, length, C.byref(ev), _stream))
        return CellBuffer(v.ct, length, mem)

    @staticmethod
    def fill_via(length: int, f: Callable[[int], object], dtype) -> "CellBuffer":
        return CellBuffer.from_vec(np.array([f(i) for i in range(length)], dtype=dtype))

    @staticmethod
    def empty(length: int, ct: int) -> "CellBuffer":
        return CellBuffer(ct, length, DeviceMem(length * NP_DTYPES[ct].itemsize))

    # ---- accessors
    def len(self) -> int:
        return self.n

    __len__ = len

    def is_empty(self) -> bool:
        return self.n == 0

    def cell_type(self) -> int:
        return self.ct

    def shard(self, cell_offset: int, cell_len: int) -> "CellBuffer":
        """Contiguous window (row-block shard) of this buffer; no copy."""
        sz = NP_DTYPES[self.ct].itemsize
        return CellBuffer(self.ct, cell_len, self.mem.window(cell_offset * sz, cell_len * sz))

    def window(self, cols: int, window=(0, 0), window_size=(0, 0), size=None, resample=None) -> "CellBuffer":
        """The `window_size` = (w, h) cells at `window` = (x, y) of this buffer read as a raster of rows of `cols` cells, delivered as
        `size` = (out_w, out_h) cells (default: as they are; another size resamples by `resample`: None or "NearestNeighbour",
        "Bilinear", "Average" — the rule of each is in include/erased_cells.h) — the device part of
        read_cells(window, window_size, size, e_resample_alg) (src/gdal/rasterband.rs:82-103).  One launch, no download."""
        alg = _resample_alg(resample)
        rows, x, y, w, h, ow, oh = _window_args(self.n, cols, window, window_size, size)
        out = CellBuffer.empty(ow * oh, self.ct)
        _cut(alg, self.ct, self.mem.ptr, None, cols, rows, x, y, w, h, ow, oh, out.mem.ptr, None)
        return out

    def focal(self, cols: int, op, radius=(1, 1), whole: bool = False):
        """The moving-window `op` ("sum" "mean" "min" "max" or an ec_focal_op) over the (2 ry + 1) x (2 rx + 1) footprint of every cell of
        this buffer read as rows of `cols` cells, `radius` = (rx, ry), clipped at the raster's edges — the rule is at ec_focal in
        include/erased_cells.h.  A CellBuffer of ec_focal_result_type (Float64 for sum / mean); with `whole` only cells whose whole
        footprint exists are valid and a MaskedCellBuffer says which.  One launch, no download."""
        out, om = _focal(self, None, cols, op, radius, whole)
        return out if om is None else MaskedCellBuffer(out, om)

    def convolve(self, cols: int, weights, normalize: bool = False, whole: bool = False):
        """The weighted moving-window sum (a correlation) with the 2-D `weights` of odd shape (2 ry + 1, 2 rx + 1), as Float64 cells;
        `normalize` divides by the sum of the weights counted.  A MaskedCellBuffer with `whole`, as `focal`."""
        out, om = _convolve(self, None, cols, weights, normalize, whole)
        return out if om is None else MaskedCellBuffer(out, om)

    def focal_rank(self, cols: int, q=(1, 2), method="lower", radius=(1, 1), whole: bool = False):
        """The moving-window order statistic (ec_focal_rank; the rule is in include/erased_cells.h): the taps of every cell's footprint
        in the reference's total order and the one at position q * (count - 1) kept — rounded down ("lower") or up ("upper"),
        q = (num, den) an exact fraction as `composite_rank` takes it, `radius` = (rx, ry) as `focal` takes it, at most 64 cells in the
        footprint.  (0, 1) is `focal(cols, "min")`, (1, 1) `focal(cols, "max")`.  Returns what `focal(cols, "min", ...)` returns."""
        out, om = _focal_rank(self, None, cols, q, method, radius, whole)
        return out if om is None else MaskedCellBuffer(out, om)

    def focal_median(self, cols: int, radius=(1, 1), method="lower", whole: bool = False):
        """`focal_rank` at q = 1/2: the median filter.  The lower and the upper median agree where the tap count is odd."""
        return self.focal_rank(cols, (1, 2), method, radius, whole)

    def focal_majority(self, cols: int, radius=(1, 1), whole: bool = False):
        """The majority (mode) filter (ec_focal_majority): every cell takes the value most cells of its footprint hold, the least of
        those that tie under the total order; "equal" is equal bits.  Returns what `focal(cols, "min", ...)` returns."""
        out, om = _focal_rank(self, None, cols, None, None, radius, whole)
        return out if om is None else MaskedCellBuffer(out, om)

    def regions(self, cols: int, connectivity: int = 4, min_cells: int = 0, numbering="dense"):
        """The connected regions of equal cells of this buffer read as rows of `cols` cells (ec_regions; the rule is in
        include/erased_cells.h) -> (MaskedCellBuffer of Int32 labels, K): "equal" is equal bits, `connectivity` 4 or 8, regions of
        fewer than `min_cells` cells are invalidated, and the K kept ones are numbered 1 .. K in raster order of their first cell
        ("dense") or by that cell's index plus one ("root").  The labels are a zone raster: `zonal_stats(labels, K + 1)`."""
        return _regions(self, None, self.n, cols, connectivity, min_cells, numbering, True)

    def put_window(self, cols: int, window, tile: "CellBuffer", window_size) -> None:
        """Writes `tile` (`window_size` = (w, h) contiguous cells of this buffer's type) into the window at `window` = (x, y) of this
        buffer read as rows of `cols` cells.  Nothing outside the window changes."""
        if tile.ct != self.ct:
            raise EcError(EC_ERR_ARG, f"put_window: a {CT_NAMES[tile.ct]} tile into a {CT_NAMES[self.ct]} buffer")
        w, h = window_size
        rows, x, y, w, h, _, _ = _window_args(self.n, cols, window, (w, h), None)
        if w * h != tile.n:
            raise AssertionError(f"a tile of {tile.n} cells is not {w} x {h}")
        check(lib().ec_window_put(self.ct, tile.mem.ptr, None, w, h, self.mem.ptr, None, cols, rows, x, y, _stream))

    def get(self, index: int) -> CellValue:
        if not 0 <= index < self.n:
            raise IndexError(f"index out of bounds: the len is {self.n} but the index is {index}")  # Rust panics
        sz = NP_DTYPES[self.ct].itemsize
        return CellValue(self.ct, _download(self.mem.window(index * sz, sz), NP_DTYPES[self.ct], 1)[0])

    def put(self, index: int, value) -> None:
        v = _scalar(value).convert(self.ct)  # NarrowingError like buffer.rs:137
        if not 0 <= index < self.n:
            raise IndexError(f"index out of bounds: the len is {self.n} but the index is {index}")
        sz = NP_DTYPES[self.ct].itemsize
        a = np.array([v.value], dtype=NP_DTYPES[self.ct])
        check(lib().ec_upload(self.mem.window(index * sz, sz).ptr, a.ctypes.data_as(C.c_void_p), sz, _stream))

    def to_numpy(self) -> np.ndarray:
        return _download(self.mem, NP_DTYPES[self.ct], self.n)

    def extend(self, values) -> None:
        """impl Extend<C> for CellBuffer (src/buffer.rs:205-221): each item goes through num-traits'
        range-checked `to_<p>()` (value-based, unlike `convert`) and panics when it does not fit."""
        items = [_scalar(v) for v in values]
        dt = NP_DTYPES[self.ct]
        new = np.empty(len(items), dtype=dt)
        for i, v in enumerate(items):
            x = v.value
            if dt.kind in "ui":
                info = np.iinfo(dt)
                f = float(x)
                if f != f or not (info.min - 1 < f < info.max + 1):
                    raise OverflowError(f"called `Option::unwrap()` on a `None` value: {v!r} does not fit {CT_NAMES[self.ct]}")
                new[i] = int(x)  # truncation toward zero for float sources
            else:
                new[i] = dt.type(x)
        grown = DeviceMem((self.n + new.size) * dt.itemsize)
        if self.n:
            check(lib().ec_copy(grown.ptr, self.mem.ptr, self.n * dt.itemsize, _stream))
        if new.size:
            check(lib().ec_upload(grown.window(self.n * dt.itemsize, new.nbytes).ptr, new.ctypes.data_as(C.c_void_p), new.nbytes, _stream))
        self.mem, self.n = grown, self.n + new.size

    def clone(self) -> "CellBuffer":
        out = CellBuffer.empty(self.n, self.ct)
        check(lib().ec_copy(out.mem.ptr, self.mem.ptr, self.mem.nbytes, _stream))
        return out

    # ---- convert / to_vec / min_max (src/buffer.rs:150-185)
    def convert(self, ct: int) -> "CellBuffer":
        if ct == self.ct:
            return self.clone()
        if not can_fit_into(self.ct, ct):
            check(lib().ec_convert(self.ct, None, ct, None, 0, _stream))  # raises NarrowingError{src,dst}
        if self.n == 0:
            return CellBuffer.empty(0, UInt8)  # collect() of nothing (buffer.rs:233-234)
        out = CellBuffer.empty(self.n, ct)
        check(lib().ec_convert(self.ct, self.mem.ptr, ct, out.mem.ptr, self.n, _stream))
        return out

    def cast(self, ct: int, mode="round") -> "CellBuffer":
        """The cells as type `ct`, for every pair of types (ec_cast) — where `convert` refuses a narrowing.  mode "round": the
        storing rule (integers clamped to the range, floats rounded half away from zero, then saturated, NaN -> 0); mode "as":
        Rust's `as` (integers wrap, floats truncate toward zero and saturate).  A pair that fits is `convert` in either mode."""
        m = _cast_mode(mode)
        out = CellBuffer.empty(self.n, ct)
        check(lib().ec_cast(m, self.ct, self.mem.ptr, ct, out.mem.ptr, self.n, _stream))
        return out

    def to_scaled(self, ct: int, scale: float, offset: float) -> "CellBuffer":
        """`self * scale + offset` (two rounded f64 steps) stored as type `ct` by the "round" rule, in one launch (ec_cast_scaled):
        `ndvi.to_scaled(Int16, 10000.0, 0.0)`."""
        return _to_scaled(self, None, ct, scale, offset, None)

    def to_vec(self, ct: Optional[int] = None) -> np.ndarray:
        ct = self.ct if ct is None else ct
        r = self.convert(ct)
        if r.ct != ct:
            raise AssertionError("danger::cast: cell types differ (empty convert yields UInt8, buffer.rs:443-444)")
        return r.to_numpy()

    def min_max(self) -> tuple[CellValue, CellValue]:
        mn, mx = EcValue(), EcValue()
        check(lib().ec_min_max(self.ct, self.mem.ptr, None, self.n, C.byref(mn), C.byref(mx), _stream))
        return CellValue.from_ec(mn), CellValue.from_ec(mx)

    def stats(self) -> Stats:
        """count, min, max, sum, mean and population stddev in one pass over the cells where they are."""
        out = EcStats()
        check(lib().ec_stats_compute(self.ct, self.mem.ptr, None, self.n, C.byref(out), _stream))
        return Stats.from_ec(out)

    def zonal_stats(self, zones: "CellBuffer", n_zones: int) -> list:
        """`stats()` per zone of the zone raster `zones` (UInt8, UInt16 or Int32, one id per cell) in one pass: a list of `n_zones`
        Stats, entry z over the cells whose id is z.  An id outside 0 .. n_zones - 1 belongs to no zone (ec_zonal_stats_compute;
        the rule is in include/erased_cells.h).  `mean NDVI per region`: `[s.mean for s in ndvi.zonal_stats(regions, 200)]`."""
        return _zonal_stats(self, None, zones, n_zones)

    def broadcast(self, table, cell_type: Optional[int] = None) -> "MaskedCellBuffer":
        """This buffer as a zone raster, each cell replaced by `table[id]`: the way back from per-zone figures into the raster
        (ec_zonal_broadcast).  `table`: a CellBuffer of n_zones cells, or a sequence / array that `cell_type` (default: its own
        numpy type) is stored as.  A cell whose id is outside 0 .. len(table) - 1 is zero and not valid in the result."""
        return _table_gather("broadcast", "EC_ZONAL_MAX_ZONES", EC_ZONAL_MAX_ZONES, "ec_zonal_broadcast", self, table, cell_type)

    def zonal_table(self, zones: "CellBuffer", n_zones: int) -> np.ndarray:
        """`zonal_stats` for up to EC_ZONAL_TABLE_MAX_ZONES (2^24) zones — the K + 1 labels of `regions`, a UInt16 parcel raster — as
        ONE numpy structured array of `n_zones` rows with the fields count, min, max, sum, mean and stddev (ec_zonal_table_compute;
        the rule, whose Float and 64-bit sums are truncated fixed-point sums independent of any order, is in include/erased_cells.h).
        `per_patch = ndvi.zonal_table(labels, K + 1); per_patch["mean"]`."""
        return _zonal_table(self, None, zones, n_zones)

    def lookup(self, table, cell_type: Optional[int] = None) -> "MaskedCellBuffer":
        """`broadcast` for a table of up to EC_ZONAL_TABLE_MAX_ZONES cells, read from device memory (ec_zonal_lookup): each cell
        replaced by `table[id]`; a cell whose id is outside 0 .. len(table) - 1 is zero and not valid in the result.
        `anomaly = ndvi - labels.lookup(per_patch["mean"])`."""
        return _table_gather("lookup", "EC_ZONAL_TABLE_MAX_ZONES", EC_ZONAL_TABLE_MAX_ZONES, "ec_zonal_lookup", self, table, cell_type)

    def reclassify(self, table_or_breaks, values=None, right: bool = False, dtype: Optional[int] = None, valid=None, breaks_dtype: Optional[int] = None):
        """Each cell replaced by the value of its class among the breaks, in one pass (ec_reclass; the rule is in
        include/erased_cells.h): class c = the number of breaks <= the cell (`right`: < the cell), result `values[c]`.  Pass a
        ReclassTable to reuse one across calls, or breaks and `len(breaks) + 1` values.  A CellBuffer comes back — or, when `valid`
        drops a class, a MaskedCellBuffer whose mask is 0 in the dropped classes."""
        table = _reclass_table(self.ct, table_or_breaks, values, right, dtype, valid, None, breaks_dtype)
        out, om = _reclass(self, None, table, table.drops)
        return MaskedCellBuffer(out, om) if om is not None else out

    def classify(self, breaks, right: bool = False, breaks_dtype: Optional[int] = None) -> "CellBuffer":
        """A UInt8 class raster with values 0 .. len(breaks): numpy.digitize(cells, breaks, right) under the reference's total order,
        fit for `zonal_stats` — `[s.count for s in x.zonal_stats(x.classify(edges), len(edges) + 1)]` is a histogram."""
        return self.reclassify(breaks, np.arange(len(breaks) + 1, dtype=np.uint8), right=right, breaks_dtype=breaks_dtype)

    # ---- arithmetic (src/buffer.rs:321-371)
    def _binop(self, op: int, rhs) -> "CellBuffer":
        if isinstance(rhs, CellBuffer):
            n = min(self.n, rhs.n)  # zip (buffer.rs:327)
            if n == 0:
                return CellBuffer.empty(0, UInt8)
            out = CellBuffer.empty(n, Float64)
            check(lib().ec_binop(op, self.ct, self.mem.ptr, rhs.ct, rhs.mem.ptr, n, out.mem.ptr, _stream))
            return out
        v = _scalar(rhs).to_ec()  # RHS scalar (buffer.rs:346-352)
        if self.n == 0:
            return CellBuffer.empty(0, UInt8)
        out = CellBuffer.empty(self.n, Float64)
        check(lib().ec_binop_scalar(op, self.ct, self.mem.ptr, self.n, C.byref(v), out.mem.ptr, _stream))
        return out

    def __add__(self, rhs): return self._binop(ADD, rhs)
    def __sub__(self, rhs): return self._binop(SUB, rhs)
    def __mul__(self, rhs): return self._binop(MUL, rhs)
    def __truediv__(self, rhs): return self._binop(DIV, rhs)

    def __neg__(self) -> "CellBuffer":
        if self.n == 0:
            return CellBuffer.empty(0, UInt8)
        out = CellBuffer.empty(self.n, lib().ec_neg_result_type(self.ct))
        check(lib().ec_neg(self.ct, self.mem.ptr, self.n, out.mem.ptr, _stream))
        return out

    # ---- per-cell order predicates (impl Ord for CellValue, src/value.rs:248-271, cell by cell)
    def compare(self, rel, rhs) -> "Mask":
        """The Mask of the cells for which `self[i] rel rhs[i]` holds under the reference's per-cell order (both cells unified to
        CellType::union, ints natural, floats total_cmp).  `rel`: one of "<" "<=" ">" ">=" "==" "!=" or an ec_cmp value; `rhs`: a
        CellBuffer (zip-truncated) or a scalar.  One launch, nothing downloaded.  The operators `==` `<` `>` of a buffer are NOT
        this: they stay the reference's whole-buffer Ord (`cmp`)."""
        return _compare(rel, self, None, rhs)

    def lt(self, rhs) -> "Mask": return self.compare(EC_CMP_LT, rhs)
    def le(self, rhs) -> "Mask": return self.compare(EC_CMP_LE, rhs)
    def gt(self, rhs) -> "Mask": return self.compare(EC_CMP_GT, rhs)
    def ge(self, rhs) -> "Mask": return self.compare(EC_CMP_GE, rhs)
    def eq(self, rhs) -> "Mask": return self.compare(EC_CMP_EQ, rhs)
    def ne(self, rhs) -> "Mask": return self.compare(EC_CMP_NE, rhs)

    # ---- Ord / Eq (src/buffer.rs:373-436), decided on the device: first differing cell, no download.  `==` `<` `>` are the
    # reference's WHOLE-BUFFER order; the per-cell predicates are compare() and lt() .. ne() above.
    def cmp(self, other: "CellBuffer") -> int:
        res = C.c_int32()
        check(lib().ec_buffer_cmp(self.ct, self.mem.ptr, self.n, other.ct, other.mem.ptr, other.n, C.byref(res), _stream))
        return res.value

    def __eq__(self, other):
        return isinstance(other, CellBuffer) and self.cmp(other) == 0

    def __lt__(self, other):
        return self.cmp(other) < 0

    def __gt__(self, other):
        return self.cmp(other) > 0

    __hash__ = None

    def __repr__(self):  # impl Debug for CellBuffer (src/buffer.rs:188-203)
        return f"{CT_NAMES[self.ct]}CellBuffer({_elided_ends(self.n, lambda o, k: self.shard(o, k).to_numpy())})"


# --------------------------------------------------------------------------- NoData
class NoData:
    """NoData<T> (src/masked/nodata.rs:7-17)."""

    NONE, DEFAULT, VALUE = range(3)

    def __init__(self, kind: int, value=None):
        self.kind, self._value = kind, value

    @staticmethod
    def none() -> "NoData":
        return NoData(NoData.NONE)

    @staticmethod
    def default() -> "NoData":
        return NoData(NoData.DEFAULT)

    @staticmethod
    def new(value) -> "NoData":
        return NoData(NoData.VALUE, value)

    def value(self, ct: int) -> Optional[CellValue]:
        """NoData::value (nodata.rs:23-40) for T = ct."""
        if self.kind == NoData.NONE:
            return None
        if self.kind == NoData.VALUE:
            v = self._value
            return v if isinstance(v, CellValue) and v.ct == ct else CellValue(ct, v.value if isinstance(v, CellValue) else v)
        out = EcValue()
        check(lib().ec_nodata_default(ct, C.byref(out)))
        return CellValue.from_ec(out)


# --------------------------------------------------------------------------- Mask
class Mask:
    """`Mask(Vec<bool>)` (src/masked/mask.rs:10-12): one byte per cell, 0 or 1, in HBM."""

    def __init__(self, n: int, mem: DeviceMem):
        self.n, self.mem = n, mem

    @staticmethod
    def new(values: Sequence[bool]) -> "Mask":
        a = np.ascontiguousarray(np.asarray(values).astype(bool).astype(np.uint8))
        return Mask(a.size, _upload(a))

    @staticmethod
    def fill(length: int, value: bool) -> "Mask":
        mem = DeviceMem(length)
        ev = CellValue(UInt8, 1 if value else 0).to_ec()
        check(lib().ec_fill(UInt8, mem.ptr, length, C.byref(ev), _stream))
        return Mask(length, mem)

    @staticmethod
    def fill_via(length: int, f: Callable[[int], bool]) -> "Mask":
        return Mask.new([bool(f(i)) for i in range(length)])

    @staticmethod
    def empty(length: int) -> "Mask":
        return Mask(length, DeviceMem(length))

    def len(self) -> int:
        return self.n

    __len__ = len

    def is_empty(self) -> bool:
        return self.n == 0

    def shard(self, cell_offset: int, cell_len: int) -> "Mask":
        return Mask(cell_len, self.mem.window(cell_offset, cell_len))

    def to_numpy(self) -> np.ndarray:
        return _download(self.mem, np.uint8, self.n)

    def get(self, index: int) -> bool:
        if not 0 <= index < self.n:
            raise IndexError(index)
        return bool(_download(self.mem.window(index, 1), np.uint8, 1)[0])

    def put(self, index: int, value: bool) -> None:
        if not 0 <= index < self.n:
            raise IndexError(index)
        a = np.array([1 if value else 0], dtype=np.uint8)
        check(lib().ec_upload(self.mem.window(index, 1).ptr, a.ctypes.data_as(C.c_void_p), 1, _stream))

    def __iter__(self):  # impl IntoIterator for Mask (mask.rs:171-178)
        return (bool(b) for b in self.to_numpy())

    def __getitem__(self, index: int) -> bool:  # impl Index<usize> for Mask (mask.rs:89-94)
        return self.get(index)

    def __setitem__(self, index: int, value: bool) -> None:  # impl IndexMut (mask.rs:96-100)
        self.put(index, value)

    def extend(self, values) -> None:  # impl Extend<bool> for Mask (mask.rs:83-87)
        new = np.asarray([bool(v) for v in values], dtype=np.uint8)
        grown = DeviceMem(self.n + new.size)
        if self.n:
            check(lib().ec_copy(grown.ptr, self.mem.ptr, self.n, _stream))
        if new.size:
            check(lib().ec_upload(grown.window(self.n, new.size).ptr, new.ctypes.data_as(C.c_void_p), new.size, _stream))
        self.mem, self.n = grown, self.n + new.size

    def clone(self) -> "Mask":
        out = Mask.empty(self.n)
        check(lib().ec_copy(out.mem.ptr, self.mem.ptr, self.n, _stream))
        return out

    def _morph(self, cols: int, op: int, radius) -> "Mask":
        (rx, ry), rows = _radius(radius), _raster_rows(self.n, cols)
        out = Mask.empty(self.n)
        if self.n:
            check(lib().ec_focal(op, UInt8, self.mem.ptr, None, cols, rows, rx, ry, 0, out.mem.ptr, None, _stream))
        return out

    def dilate(self, cols: int, radius=(1, 1)) -> "Mask":
        """A byte of the result is set iff ANY byte of its footprint — `radius` = (rx, ry), clipped at the raster's edges — is: the
        cloud-mask buffer.  ec_focal MAX over the mask's bytes as UInt8 cells."""
        return self._morph(cols, EC_FOCAL_MAX, radius)

    def erode(self, cols: int, radius=(1, 1)) -> "Mask":
        """A byte of the result is set iff ALL bytes of its clipped footprint are (ec_focal MIN)."""
        return self._morph(cols, EC_FOCAL_MIN, radius)

    def _distance(self, cols: int, max_sq: int, ct, want_mask: bool = True):
        """ec_distance of the mask read as rows of `cols` bytes, with the workspace from the library's pool -> (CellBuffer of type
        `ct` or None for the mask-only form, Mask or None)."""
        rows = _raster_rows(self.n, cols)
        out = CellBuffer.empty(self.n, ct) if ct is not None else None
        om = Mask.empty(self.n) if want_mask else None
        if self.n:  # an empty mask has no memory to point at
            check(lib().ec_distance(self.mem.ptr, cols, rows, max_sq, ct if ct is not None else UInt32, out.mem.ptr if out is not None else None,
                                    om.mem.ptr if om is not None else None, None, _stream))
        return out, om

    def distance(self, cols: int, max_distance=None, squared: bool = False) -> "MaskedCellBuffer":
        """The exact Euclidean distance, in cells, of every cell of the mask read as rows of `cols` bytes to the nearest SET byte
        (ec_distance; the rule is in include/erased_cells.h): Float64 distances, or with `squared` the UInt32 squared distances.  A
        cell is valid iff the mask has a set byte and its distance is at most `max_distance` (None: no limit; an int, a float or a
        Fraction, compared exactly); an invalid cell holds zero bits."""
        return MaskedCellBuffer(*self._distance(cols, _max_sq(max_distance), UInt32 if squared else Float64))

    def within(self, cols: int, distance) -> "Mask":
        """A byte of the result is set iff a set byte of the mask lies within `distance` cells of it, Euclidean: the round buffer
        (`dilate` is the rectangle).  ec_distance's mask-only form: no distance is ever written."""
        return self._distance(cols, _max_sq(distance), None)[1]

    def regions(self, cols: int, connectivity: int = 4, min_cells: int = 0, numbering="dense"):
        """The connected regions of the SET bytes of the mask read as rows of `cols` bytes (ec_regions without cells: every set
        byte equals every other) -> (MaskedCellBuffer of Int32 labels, K), as `CellBuffer.regions`; with "dense" this is
        scipy.ndimage.label's numbering."""
        return _regions(None, self, self.n, cols, connectivity, min_cells, numbering, True)

    def sieve(self, cols: int, min_cells: int, connectivity: int = 4) -> "Mask":
        """The mask without its regions of fewer than `min_cells` set bytes (ec_regions' sieve-only form)."""
        return _regions(None, self, self.n, cols, connectivity, min_cells, EC_REGIONS_ROOT, False)

    def counts(self) -> tuple[int, int]:
        """(data, nodata) — mask.rs:72-80."""
        a, b = C.c_uint64(), C.c_uint64()
        check(lib().ec_mask_counts(self.mem.ptr, self.n, C.byref(a), C.byref(b), _stream))
        return a.value, b.value

    def all(self, value: bool) -> bool:
        t, f = self.counts()
        return (f == 0) if value else (t == 0)

    def __invert__(self) -> "Mask":  # Not for &Mask (mask.rs:111-116)
        out = Mask.empty(self.n)
        check(lib().ec_mask_not(self.mem.ptr, self.n, out.mem.ptr, _stream))
        return out

    def __and__(self, rhs: "Mask") -> "Mask":  # BitAnd for &Mask: zip -> shorter (mask.rs:129-140)
        n = min(self.n, rhs.n)
        out = Mask.empty(n)
        check(lib().ec_mask_and(self.mem.ptr, rhs.mem.ptr, n, out.mem.ptr, _stream))
        return out

    def __or__(self, rhs: "Mask") -> "Mask":  # BitOr for &Mask (mask.rs:153-163)
        n = min(self.n, rhs.n)
        out = Mask.empty(n)
        check(lib().ec_mask_or(self.mem.ptr, rhs.mem.ptr, n, out.mem.ptr, _stream))
        return out

    def __iand__(self, rhs: "Mask") -> "Mask":  # BitAnd for Mask (owned, in place; lhs length kept — mask.rs:118-127)
        check(lib().ec_mask_and(self.mem.ptr, rhs.mem.ptr, min(self.n, rhs.n), self.mem.ptr, _stream))
        return self

    def __ior__(self, rhs: "Mask") -> "Mask":  # mask.rs:142-151
        check(lib().ec_mask_or(self.mem.ptr, rhs.mem.ptr, min(self.n, rhs.n), self.mem.ptr, _stream))
        return self

    def cmp(self, other: "Mask") -> int:  # derived Ord on Vec<bool> (mask.rs:10)
        res = C.c_int32()
        check(lib().ec_buffer_cmp(UInt8, self.mem.ptr, self.n, UInt8, other.mem.ptr, other.n, C.byref(res), _stream))
        return res.value

    def __eq__(self, other):
        return isinstance(other, Mask) and self.cmp(other) == 0

    __hash__ = None

    def __repr__(self):  # impl Debug for Mask (src/masked/mask.rs:165-169)
        return f"Mask({_elided_ends(self.n, lambda o, k: self.shard(o, k).to_numpy().astype(bool))})"


# --------------------------------------------------------------------------- MaskedCellBuffer
class MaskedCellBuffer:
    """`MaskedCellBuffer(CellBuffer, Mask)` (src/masked/masked_buffer.rs:39-41)."""

    def __init__(self, buffer: CellBuffer, mask: Mask):
        if buffer.len() != mask.len():
            raise AssertionError("Mask and buffer must have the same length.")  # masked_buffer.rs:48-53
        self._buf, self._mask = buffer, mask

    new = None  # set below (classmethod-style alias needs the class)

    @staticmethod
    def from_vec(data) -> "MaskedCellBuffer":
        b = CellBuffer.from_vec(data)
        return MaskedCellBuffer(b, Mask.fill(b.len(), True))

    @staticmethod
    def from_iter(items, dtype=None) -> "MaskedCellBuffer":
        """FromIterator<C> (all valid) and FromIterator<(C, bool)> for MaskedCellBuffer (masked_buffer.rs:257-278)."""
        items = list(items)
        if items and isinstance(items[0], tuple):
            vals = np.array([p[0] for p in items]) if dtype is None else np.array([p[0] for p in items], dtype=dtype)
            if vals.dtype == np.dtype(np.int64) and dtype is None:
                vals = vals.astype(np.int32)
            return MaskedCellBuffer(CellBuffer.from_vec(vals), Mask.new([bool(p[1]) for p in items]))
        return MaskedCellBuffer.from_vec(items if dtype is None else np.array(items, dtype=dtype))

    def __iter__(self):
        """impl IntoIterator for &MaskedCellBuffer (masked_buffer.rs:289-318): yields (CellValue, bool)."""
        return ((CellValue(self.cell_type(), v), bool(m)) for v, m in zip(self._buf.to_numpy(), self._mask.to_numpy()))

    @staticmethod
    def from_buffer(b: CellBuffer) -> "MaskedCellBuffer":  # From<CellBuffer> (masked_buffer.rs:250-255)
        return MaskedCellBuffer(b, Mask.fill(b.len(), True))

    @staticmethod
    def from_vec_with_nodata(data, nodata: NoData) -> "MaskedCellBuffer":
        """masked_buffer.rs:62-71: mask[i] = !(data[i] == nodata) under total-order equality."""
        b = CellBuffer.from_vec(data)
        return MaskedCellBuffer(b, mask_from_nodata(b, nodata))

    @staticmethod
    def with_defaults(length: int, ct: int) -> "MaskedCellBuffer":
        return MaskedCellBuffer(CellBuffer.with_defaults(length, ct), Mask.fill(length, True))

    @staticmethod
    def fill(length: int, value) -> "MaskedCellBuffer":
        return MaskedCellBuffer(CellBuffer.fill(length, value), Mask.fill(length, True))

    @staticmethod
    def fill_via(length: int, f, dtype) -> "MaskedCellBuffer":
        return MaskedCellBuffer(CellBuffer.fill_via(length, f, dtype), Mask.fill(length, True))

    @staticmethod
    def fill_with_mask_via(length: int, mv: Callable[[int], tuple], dtype) -> "MaskedCellBuffer":
        pairs = [mv(i) for i in range(length)]
        return MaskedCellBuffer(CellBuffer.from_vec(np.array([p[0] for p in pairs], dtype=dtype)),
                                Mask.new([p[1] for p in pairs]))

    def buffer(self) -> CellBuffer:
        return self._buf

    def mask(self) -> Mask:
        return self._mask

    def len(self) -> int:
        return self._buf.len()

    __len__ = len

    def cell_type(self) -> int:
        return self._buf.cell_type()

    def shard(self, cell_offset: int, cell_len: int) -> "MaskedCellBuffer":
        return MaskedCellBuffer(self._buf.shard(cell_offset, cell_len), self._mask.shard(cell_offset, cell_len))

    def window(self, cols: int, window=(0, 0), window_size=(0, 0), size=None, resample=None) -> "MaskedCellBuffer":
        """CellBuffer.window for values and mask in ONE launch (read_cells_masked, src/gdal/rasterband.rs:104-125).  "Bilinear" and
        "Average" weigh the valid cells of a footprint only; an output cell without one is invalid and holds 0."""
        alg = _resample_alg(resample)
        rows, x, y, w, h, ow, oh = _window_args(self.len(), cols, window, window_size, size)
        out, om = CellBuffer.empty(ow * oh, self.cell_type()), Mask.empty(ow * oh)
        _cut(alg, self.cell_type(), self._buf.mem.ptr, self._mask.mem.ptr, cols, rows, x, y, w, h, ow, oh, out.mem.ptr, om.mem.ptr)
        return MaskedCellBuffer(out, om)

    def focal(self, cols: int, op, radius=(1, 1), whole: bool = False) -> "MaskedCellBuffer":
        """`CellBuffer.focal` over the cells whose mask byte is set: a masked-out cell contributes nothing, and one with a valid
        neighbour is filled from it (AND the result's mask with this one to keep the holes)."""
        return MaskedCellBuffer(*_focal(self._buf, self._mask, cols, op, radius, whole))

    def convolve(self, cols: int, weights, normalize: bool = False, whole: bool = False) -> "MaskedCellBuffer":
        """`CellBuffer.convolve` over the cells whose mask byte is set."""
        return MaskedCellBuffer(*_convolve(self._buf, self._mask, cols, weights, normalize, whole))

    def focal_rank(self, cols: int, q=(1, 2), method="lower", radius=(1, 1), whole: bool = False) -> "MaskedCellBuffer":
        """`CellBuffer.focal_rank` over the cells whose mask byte is set: the position follows the count of those."""
        return MaskedCellBuffer(*_focal_rank(self._buf, self._mask, cols, q, method, radius, whole))

    def focal_median(self, cols: int, radius=(1, 1), method="lower", whole: bool = False) -> "MaskedCellBuffer":
        """`focal_rank` at q = 1/2 over the cells whose mask byte is set."""
        return self.focal_rank(cols, (1, 2), method, radius, whole)

    def focal_majority(self, cols: int, radius=(1, 1), whole: bool = False) -> "MaskedCellBuffer":
        """`CellBuffer.focal_majority` over the cells whose mask byte is set."""
        return MaskedCellBuffer(*_focal_rank(self._buf, self._mask, cols, None, None, radius, whole))

    def regions(self, cols: int, connectivity: int = 4, min_cells: int = 0, numbering="dense"):
        """`CellBuffer.regions` over the cells whose mask byte is set: an invalid cell belongs to no region and joins none."""
        return _regions(self._buf, self._mask, self.len(), cols, connectivity, min_cells, numbering, True)

    def sieve(self, cols: int, min_cells: int, connectivity: int = 4) -> "MaskedCellBuffer":
        """The same cells with every region of fewer than `min_cells` cells invalidated (ec_regions' sieve-only form: no label is
        ever written).  GDAL's sieve merges such a patch into its largest neighbour; this one drops it."""
        return MaskedCellBuffer(self._buf, _regions(self._buf, self._mask, self.len(), cols, connectivity, min_cells, EC_REGIONS_ROOT, False))

    def put_window(self, cols: int, window, tile: "MaskedCellBuffer", window_size) -> None:
        """CellBuffer.put_window for values and mask in one launch."""
        if tile.cell_type() != self.cell_type():
            raise EcError(EC_ERR_ARG, f"put_window: a {CT_NAMES[tile.cell_type()]} tile into a {CT_NAMES[self.cell_type()]} buffer")
        w, h = window_size
        rows, x, y, w, h, _, _ = _window_args(self.len(), cols, window, (w, h), None)
        if w * h != tile.len():
            raise AssertionError(f"a tile of {tile.len()} cells is not {w} x {h}")
        check(lib().ec_window_put(self.cell_type(), tile._buf.mem.ptr, tile._mask.mem.ptr, w, h, self._buf.mem.ptr, self._mask.mem.ptr,
                                  cols, rows, x, y, _stream))

    def get(self, index: int) -> CellValue:
        return self._buf.get(index)

    def put(self, index: int, value) -> None:
        self._buf.put(index, value)

    def get_masked(self, index: int) -> Optional[CellValue]:
        return self._buf.get(index) if self._mask.get(index) else None

    def get_with_mask(self, index: int) -> tuple[CellValue, bool]:
        return self._buf.get(index), self._mask.get(index)

    def put_with_mask(self, index: int, value, mask: bool) -> None:
        self.put(index, value)
        self._mask.put(index, mask)

    def counts(self) -> tuple[int, int]:
        return self._mask.counts()

    def extend(self, pairs) -> None:  # impl Extend<(C, bool)> for MaskedCellBuffer (masked_buffer.rs:280-287)
        pairs = list(pairs)
        self._buf.extend([p[0] for p in pairs])
        self._mask.extend([p[1] for p in pairs])

    def convert(self, ct: int) -> "MaskedCellBuffer":
        return MaskedCellBuffer(self._buf.convert(ct), self._mask.clone())

    def to_vec(self, ct: Optional[int] = None) -> np.ndarray:
        return self._buf.to_vec(ct)

    def cast(self, ct: int, mode="round") -> "MaskedCellBuffer":
        """`CellBuffer.cast` of the cells; the mask travels unchanged."""
        return MaskedCellBuffer(self._buf.cast(ct, mode), self._mask.clone())

    def to_scaled(self, ct: int, scale: float, offset: float, no_data: NoData) -> CellBuffer:
        """`CellBuffer.to_scaled` where a cell that is not valid receives `no_data.value()` whatever it holds, in one launch:
        to_vec_with_nodata (masked_buffer.rs:137-152) for a type the buffer does not fit into, the result left on the device.
        NoData.none() stores every cell."""
        nd = no_data.value(ct)
        return _to_scaled(self._buf, self._mask if nd is not None else None, ct, scale, offset, nd)

    def to_vec_with_nodata(self, ct: int, no_data: NoData) -> np.ndarray:
        """masked_buffer.rs:137-152: convert to T, then masked cells become no_data.value()."""
        conv = self._buf.convert(ct)
        if conv.ct != ct:
            raise AssertionError("danger::cast: cell types differ")
        nd = no_data.value(ct)
        if nd is None:
            return conv.to_numpy()
        out = CellBuffer.empty(conv.n, ct)
        ev = nd.to_ec()
        check(lib().ec_mask_select(ct, conv.mem.ptr, self._mask.mem.ptr, conv.n, C.byref(ev), out.mem.ptr, _stream))
        return out.to_numpy()

    def min_max(self) -> tuple[CellValue, CellValue]:
        mn, mx = EcValue(), EcValue()
        check(lib().ec_min_max(self.cell_type(), self._buf.mem.ptr, self._mask.mem.ptr, self.len(),
                               C.byref(mn), C.byref(mx), _stream))
        return CellValue.from_ec(mn), CellValue.from_ec(mx)

    def stats(self) -> Stats:
        """`CellBuffer.stats` over the valid cells: a masked-out cell contributes nothing, whatever it holds."""
        out = EcStats()
        check(lib().ec_stats_compute(self.cell_type(), self._buf.mem.ptr, self._mask.mem.ptr, self.len(), C.byref(out), _stream))
        return Stats.from_ec(out)

    def zonal_stats(self, zones: "CellBuffer", n_zones: int) -> list:
        """`CellBuffer.zonal_stats` over the valid cells: a masked-out cell belongs to no zone, whatever it holds."""
        return _zonal_stats(self._buf, self._mask, zones, n_zones)

    def zonal_table(self, zones: "CellBuffer", n_zones: int) -> np.ndarray:
        """`CellBuffer.zonal_table` over the valid cells: a masked-out cell belongs to no zone, whatever it holds."""
        return _zonal_table(self._buf, self._mask, zones, n_zones)

    def reclassify(self, table_or_breaks, values=None, right: bool = False, dtype: Optional[int] = None, valid=None, nodata=None,
                   breaks_dtype: Optional[int] = None) -> "MaskedCellBuffer":
        """`CellBuffer.reclassify` of the valid cells: a cell that is not valid receives `nodata` (default: 0) whatever it holds and stays
        invalid; a cell of a class that `valid` drops becomes invalid.  A ReclassTable must have been built with a nodata value."""
        table = _reclass_table(self.cell_type(), table_or_breaks, values, right, dtype, valid, 0 if nodata is None else nodata, breaks_dtype)
        out, om = _reclass(self._buf, self._mask, table, True)
        return MaskedCellBuffer(out, om)

    def classify(self, breaks, right: bool = False, breaks_dtype: Optional[int] = None) -> "MaskedCellBuffer":
        """`CellBuffer.classify` of the valid cells; a cell that is not valid holds 255 (0 with 255 breaks) and stays invalid."""
        return self.reclassify(breaks, np.arange(len(breaks) + 1, dtype=np.uint8), right=right, nodata=255 if len(breaks) < 255 else 0,
                               breaks_dtype=breaks_dtype)

    # ---- arithmetic (src/masked/masked_buffer.rs:323-383)
    def _binop(self, op: int, rhs) -> "MaskedCellBuffer":
        if isinstance(rhs, MaskedCellBuffer):
            n = min(self.len(), rhs.len())
            if n == 0:
                return MaskedCellBuffer(CellBuffer.empty(0, UInt8), Mask.empty(0))
            out, om = CellBuffer.empty(n, Float64), Mask.empty(n)
            check(lib().ec_masked_binop(op, self._buf.ct, self._buf.mem.ptr, self._mask.mem.ptr,
                                        rhs._buf.ct, rhs._buf.mem.ptr, rhs._mask.mem.ptr, n,
                                        out.mem.ptr, om.mem.ptr, _stream))
            return MaskedCellBuffer(out, om)
        return MaskedCellBuffer(self._buf._binop(op, rhs), self._mask.clone())  # scalar: mask carried over (:353-364)

    def __add__(self, rhs): return self._binop(ADD, rhs)
    def __sub__(self, rhs): return self._binop(SUB, rhs)
    def __mul__(self, rhs): return self._binop(MUL, rhs)
    def __truediv__(self, rhs): return self._binop(DIV, rhs)

    def __neg__(self) -> "MaskedCellBuffer":
        return MaskedCellBuffer(-self._buf, self._mask.clone())

    # ---- per-cell order predicates: the predicate ANDed with the masks (a cell that is not valid satisfies none)
    def compare(self, rel, rhs) -> Mask:
        """CellBuffer.compare ANDed, in the same launch, with this buffer's mask and — when `rhs` is a MaskedCellBuffer — with its
        mask too: the masked-operator rule (src/masked/masked_buffer.rs:326-335).  `rhs` may also be a CellBuffer or a scalar.
        `==` `<` `>` of a MaskedCellBuffer stay the reference's whole-buffer order."""
        if isinstance(rhs, MaskedCellBuffer):
            return _compare(rel, self._buf, self._mask, rhs._buf, rhs._mask)
        return _compare(rel, self._buf, self._mask, rhs)

    def lt(self, rhs) -> Mask: return self.compare(EC_CMP_LT, rhs)
    def le(self, rhs) -> Mask: return self.compare(EC_CMP_LE, rhs)
    def gt(self, rhs) -> Mask: return self.compare(EC_CMP_GT, rhs)
    def ge(self, rhs) -> Mask: return self.compare(EC_CMP_GE, rhs)
    def eq(self, rhs) -> Mask: return self.compare(EC_CMP_EQ, rhs)
    def ne(self, rhs) -> Mask: return self.compare(EC_CMP_NE, rhs)

    def or_else(self, other: "MaskedCellBuffer") -> "MaskedCellBuffer":
        """This buffer's cell where it is valid, else `other`'s cell with `other`'s validity (cloud fill): ec_masked_select with
        sel == this mask.  Operands of different cell types are converted to their union first."""
        return select(self._mask, self, other)

    def __eq__(self, other):  # derived PartialEq (masked_buffer.rs:39): buffer (all cells) and mask
        return isinstance(other, MaskedCellBuffer) and self._buf == other._buf and self._mask == other._mask

    def cmp(self, other: "MaskedCellBuffer") -> int:
        """derived PartialOrd (masked_buffer.rs:39): the buffer decides, the mask breaks ties; both on the device."""
        c = self._buf.cmp(other._buf)
        return c if c != 0 else self._mask.cmp(other._mask)

    def __lt__(self, other):
        return self.cmp(other) < 0

    def __gt__(self, other):
        return self.cmp(other) > 0

    __hash__ = None

    def __repr__(self):  # debug_tuple(buffer, mask) (src/masked/masked_buffer.rs:227-235)
        return f"{CT_NAMES[self.cell_type()]}MaskedCellBuffer({self._buf!r}, {self._mask!r})"


MaskedCellBuffer.new = staticmethod(lambda buffer, mask: MaskedCellBuffer(buffer, mask))


def mask_from_nodata(b: CellBuffer, nodata: NoData) -> Mask:
    m = Mask.empty(b.len())
    nd = nodata.value(b.ct)
    ev = nd.to_ec() if nd is not None else None
    check(lib().ec_mask_from_nodata(b.ct, b.mem.ptr, b.len(), C.byref(ev) if ev is not None else None,
                                    m.mem.ptr, _stream))
    return m


def select(mask: Mask, a, b):
    """out[i] = mask[i] ? a[i] : b[i] (ec_select), zip-truncated to the shortest of the three.  `a` and `b` are both CellBuffers or both
    MaskedCellBuffers — then the result's mask is picked the same way (ec_masked_select); operands of different cell types are
    converted to their CellType::union with `convert` first."""
    masked = isinstance(a, MaskedCellBuffer)
    if masked != isinstance(b, MaskedCellBuffer):
        raise EcError(EC_ERR_ARG, "select: a and b must both be CellBuffers or both MaskedCellBuffers")
    if a.cell_type() != b.cell_type():
        ct = union(a.cell_type(), b.cell_type())
        a = a if a.cell_type() == ct else a.convert(ct)
        b = b if b.cell_type() == ct else b.convert(ct)
    ct, n = a.cell_type(), min(mask.len(), a.len(), b.len())
    out = CellBuffer.empty(n, ct)
    if not masked:
        check(lib().ec_select(ct, a.mem.ptr, b.mem.ptr, mask.mem.ptr, n, out.mem.ptr, _stream))
        return out
    om = Mask.empty(n)
    check(lib().ec_masked_select(ct, a._buf.mem.ptr, a._mask.mem.ptr, b._buf.mem.ptr, b._mask.mem.ptr, mask.mem.ptr, n,
                                 out.mem.ptr, om.mem.ptr, _stream))
    return MaskedCellBuffer(out, om)


def _table_gather(what: str, cap_name: str, cap: int, fn: str, zones: "CellBuffer", table, cell_type: Optional[int]) -> "MaskedCellBuffer":
    """`table[id]` for each id of `zones` by the library's `fn` (ec_zonal_broadcast, ec_zonal_lookup), whose cap on the table is `cap`."""
    if not isinstance(table, CellBuffer):
        a = np.asarray(table)
        table = CellBuffer.from_vec(a.astype(NP_DTYPES[cell_type]) if cell_type is not None else a)
    elif cell_type is not None and table.ct != cell_type:
        raise EcError(EC_ERR_ARG, f"{what}: the table is {CT_NAMES[table.ct]}, not {CT_NAMES[cell_type]}")
    if not 1 <= table.n <= cap:
        raise EcError(EC_ERR_ARG, f"{what}: a table of {table.n} cells, not within 1 .. {cap_name} ({cap})")
    out, om = CellBuffer.empty(zones.n, table.ct), DeviceMem(zones.n)
    check(getattr(lib(), fn)(zones.ct, zones.mem.ptr, zones.n, table.n, table.ct, table.mem.ptr, out.mem.ptr, om.ptr, _stream))
    return MaskedCellBuffer(out, Mask(zones.n, om))


def _check_n_zones(what: str, cap_name: str, cap: int, n_zones, advice: str = "") -> int:
    """`n_zones` as an int, refused unless it is an integer within 1 .. `cap` (the family's cap, named `cap_name`)."""
    if isinstance(n_zones, bool) or not isinstance(n_zones, (int, np.integer)) or not 1 <= n_zones <= cap:
        raise EcError(EC_ERR_ARG, f"{what}: n_zones {n_zones!r} is not within 1 .. {cap_name} ({cap}){advice}")
    return int(n_zones)


def _zonal_raw(what: str, cap_name: str, cap: int, advice: str, fn: str, buf: "CellBuffer", mask, zones, n_zones) -> np.ndarray:
    """The `n_zones` ec_stats of `buf` under `mask` (or None) per zone of the CellBuffer `zones`, as the library's `fn`
    (ec_zonal_stats_compute, ec_zonal_table_compute) leaves them."""
    if isinstance(zones, MaskedCellBuffer) or not isinstance(zones, CellBuffer):
        raise EcError(EC_ERR_ARG, f"{what}: the zone raster is a {type(zones).__name__}, not a CellBuffer")
    n_zones = _check_n_zones(what, cap_name, cap, n_zones, advice)
    if zones.n != buf.n:
        raise EcError(EC_ERR_ARG, f"{what}: the zone raster has {zones.n} cells, the values {buf.n}")
    raw = np.empty(n_zones, dtype=_EC_STATS_DTYPE)
    check(getattr(lib(), fn)(buf.ct, buf.mem.ptr, mask.mem.ptr if mask is not None else None, zones.ct, zones.mem.ptr, buf.n, n_zones, raw.ctypes.data,
                             _stream))
    return raw


def _stats_list(raw: np.ndarray) -> list:
    """An array of ec_stats as a list of Stats."""
    return [Stats.from_ec(s) for s in (EcStats * raw.size).from_buffer(raw)]


def _zonal_stats(buf: "CellBuffer", mask, zones, n_zones: int) -> list:
    """`n_zones` Stats of `buf` under `mask` (or None) per zone of the CellBuffer `zones` (ec_zonal_stats_compute)."""
    return _stats_list(_zonal_raw("zonal_stats", "EC_ZONAL_MAX_ZONES", EC_ZONAL_MAX_ZONES, "; relabel in chunks", "ec_zonal_stats_compute", buf, mask, zones,
                                 n_zones))


# ec_stats as numpy sees it: the u64, two 16-byte ec_value (a type byte, padding, the payload in 8 bytes), three doubles
_EC_STATS_DTYPE = np.dtype([("count", "<u8"), ("min_dtype", "u1"), ("min_pad", "V7"), ("min_bits", "<u8"), ("max_dtype", "u1"), ("max_pad", "V7"),
                            ("max_bits", "<u8"), ("sum", "<f8"), ("mean", "<f8"), ("stddev", "<f8")])
assert _EC_STATS_DTYPE.itemsize == C.sizeof(EcStats) == 64


def stats_table(raw, ct: int) -> np.ndarray:
    """An array of ec_stats (anything with their bytes) as a structured array with the fields count, min, max, sum, mean, stddev; min
    and max in the numpy type of cell type `ct`."""
    rows = np.frombuffer(raw, dtype=_EC_STATS_DTYPE)
    value = NP_DTYPES[ct]
    out = np.empty(rows.size, dtype=[("count", np.uint64), ("min", value), ("max", value), ("sum", np.float64), ("mean", np.float64), ("stddev", np.float64)])
    for name in ("count", "sum", "mean", "stddev"):
        out[name] = rows[name]
    for name in ("min", "max"):  # the payload's low bytes are the value (little-endian union)
        bits = np.ascontiguousarray(rows[name + "_bits"])
        out[name] = bits.view(np.uint8).reshape(-1, 8)[:, :value.itemsize].copy().view(value).reshape(-1)
    return out


def _zonal_table(buf: "CellBuffer", mask, zones, n_zones: int) -> np.ndarray:
    """`n_zones` rows of statistics of `buf` under `mask` (or None) per zone of the CellBuffer `zones` (ec_zonal_table_compute)."""
    return stats_table(_zonal_raw("zonal_table", "EC_ZONAL_TABLE_MAX_ZONES", EC_ZONAL_TABLE_MAX_ZONES, "", "ec_zonal_table_compute", buf, mask, zones,
                                  n_zones), buf.ct)


def _typed_array(what: str, xs, ct: Optional[int], default_for_numbers) -> np.ndarray:
    """`xs` as a 1-D array of a cell type: `ct` when given, else its own numpy type, else `default_for_numbers(list)` for Python numbers"""
    if ct is None and isinstance(xs, np.ndarray) and xs.dtype in NP_DTYPES:
        return np.ascontiguousarray(xs).reshape(-1)
    lst = [x.value if isinstance(x, CellValue) else x for x in (xs.tolist() if isinstance(xs, np.ndarray) else list(xs))]
    if any(isinstance(x, bool) for x in lst):
        raise EcError(EC_ERR_ARG, f"reclass: a bool among the {what}")
    ct = default_for_numbers(lst) if ct is None else ct
    with np.errstate(all="ignore"):
        return np.array(lst, dtype=NP_DTYPES[ct])


def _fits_exactly(lst, ct: int) -> bool:
    """every number is integral and a cell of type ct holds it exactly"""
    try:
        if not all(float(x).is_integer() for x in lst):
            return False
        with np.errstate(all="ignore"):
            a = np.array(lst, dtype=NP_DTYPES[ct])
        return all(int(a[i]) == int(x) for i, x in enumerate(lst))
    except (OverflowError, ValueError, TypeError):
        return False


class ReclassTable:
    """The table of `CellBuffer.reclassify` for rasters of type `cell_type`: built on the host (ec_reclass_table_build), uploaded
    once, reusable across calls on this device.  `breaks`: 1 .. 255 numbers, strictly ascending; Python numbers are cells of type
    `cell_type` when all are integral and fit it, else Float64 (`breaks_dtype` overrides; a numpy array keeps its type).
    `values`: len(breaks) + 1 cells of the output type `dtype` (default: a numpy array's own type; Python numbers UInt8 when they
    fit, else Int32, else Float64).  `valid`: len(breaks) + 1 flags, a false one drops its class.  `nodata`: given iff the table
    is for MaskedCellBuffers — what a cell that is not valid receives."""

    def __init__(self, cell_type: int, breaks, values, right: bool = False, dtype: Optional[int] = None, valid=None, nodata=None,
                 breaks_dtype: Optional[int] = None):
        b = _typed_array("breaks", breaks, breaks_dtype, lambda l: cell_type if _fits_exactly(l, cell_type) else Float64)
        v = _typed_array("values", values, dtype,
                         lambda l: UInt8 if _fits_exactly(l, UInt8) else Int32 if _fits_exactly(l, Int32) else Float64)
        bt, dt = cell_type_of(b.dtype), cell_type_of(v.dtype)
        if not 1 <= b.size <= EC_RECLASS_MAX_BREAKS:
            raise EcError(EC_ERR_ARG, f"reclass: {b.size} breaks, not within 1 .. EC_RECLASS_MAX_BREAKS ({EC_RECLASS_MAX_BREAKS})")
        if v.size != b.size + 1:
            raise EcError(EC_ERR_ARG, f"reclass: {v.size} class values for {b.size} breaks, not {b.size + 1}")
        if valid is not None and len(valid) != v.size:
            raise EcError(EC_ERR_ARG, f"reclass: {len(valid)} validity flags for {v.size} classes")
        if isinstance(right, (bool, np.bool_)):
            right = int(right)
        evs = (EcValue * v.size)(*[CellValue(dt, x).to_ec() for x in v])
        vb = (C.c_uint8 * v.size)(*[1 if x else 0 for x in valid]) if valid is not None else None
        nd = (nodata if isinstance(nodata, CellValue) else CellValue(dt, nodata)).to_ec() if nodata is not None else None
        self.host = EcReclassTable()
        check(lib().ec_reclass_table_build(cell_type, bt, b.ctypes.data_as(C.c_void_p), b.size, right, dt, evs, vb,
                                           C.byref(nd) if nd is not None else None, C.byref(self.host)))
        self.ct, self.bt, self.dt, self.n_breaks = cell_type, bt, dt, int(b.size)
        self.has_nodata = bool(self.host.flags & EC_RECLASS_HAS_NODATA)
        self.drops = bool(self.host.flags & EC_RECLASS_DROPS)
        self._mem = None

    def bytes(self) -> bytes:
        return C.string_at(C.byref(self.host), EC_RECLASS_TABLE_BYTES)

    @property
    def mem(self) -> DeviceMem:
        """the device copy (uploaded at first use: building a table needs no device)"""
        if self._mem is None:
            self._mem = _upload(np.frombuffer(self.bytes(), dtype=np.uint8))
        return self._mem


def _reclass_table(ct: int, table_or_breaks, values, right, dtype, valid, nodata, breaks_dtype) -> ReclassTable:
    """the ReclassTable of a reclassify call: the one given (checked against the call) or one built from the breaks"""
    if not isinstance(table_or_breaks, ReclassTable):
        if values is None:
            raise EcError(EC_ERR_ARG, "reclassify: breaks without class values")
        return ReclassTable(ct, table_or_breaks, values, right, dtype, valid, nodata, breaks_dtype)
    t = table_or_breaks
    if values is not None or valid is not None or dtype is not None or breaks_dtype is not None:
        raise EcError(EC_ERR_ARG, "reclassify: a ReclassTable carries its own values, validity and types")
    if t.ct != ct:
        raise EcError(EC_ERR_ARG, f"reclassify: the table is for {CT_NAMES[t.ct]} rasters, this one is {CT_NAMES[ct]}")
    if t.has_nodata != (nodata is not None):
        raise EcError(EC_ERR_ARG, "reclassify: a table built with a nodata value is for MaskedCellBuffers, one without for CellBuffers")
    return t


def _reclass(buf: "CellBuffer", mask, table: ReclassTable, want_mask: bool):
    """ec_reclass of `buf` under `mask` (or None) -> (result buffer, result Mask or None)"""
    out = CellBuffer.empty(buf.n, table.dt)
    om = Mask.empty(buf.n) if want_mask else None
    check(lib().ec_reclass(buf.ct, buf.mem.ptr, mask.mem.ptr if mask is not None else None, buf.n, table.dt, table.mem.ptr, out.mem.ptr,
                           om.mem.ptr if om is not None else None, _stream))
    return out, om


# the spellings of an ec_composite_op
COMPOSITE_OPS = {"first": 0, "last": 1, "min": 2, "max": 3, "sum": 4, "mean": 5}


def _composite_op(op) -> int:
    """the ec_composite_op number of "first" "last" "min" "max" "sum" "mean" or of an ec_composite_op value; anything else is refused"""
    o = COMPOSITE_OPS.get(op, op) if isinstance(op, str) else op
    if isinstance(o, bool) or not isinstance(o, (int, np.integer)) or not 0 <= int(o) <= 5:
        raise EcError(EC_ERR_ARG, f"composite: operation {op!r} is not one of {sorted(COMPOSITE_OPS)} or an ec_composite_op value 0..5")
    return int(o)


def _composite_stack(layers, min_count):
    """the checks Python makes itself on a stack -> ([(CellBuffer, Mask or None)] in stack order, cell type, length)"""
    layers = list(layers)
    if not 1 <= len(layers) <= EC_COMPOSITE_MAX_LAYERS:
        raise EcError(EC_ERR_ARG, f"composite: {len(layers)} layers, not within 1 .. EC_COMPOSITE_MAX_LAYERS ({EC_COMPOSITE_MAX_LAYERS}); "
                                  "compose two calls for a taller stack")
    pairs = []
    for k, layer in enumerate(layers):
        if isinstance(layer, MaskedCellBuffer):
            pairs.append((layer.buffer(), layer.mask()))
        elif isinstance(layer, CellBuffer):
            pairs.append((layer, None))
        else:
            raise EcError(EC_ERR_ARG, f"composite: layer {k} is a {type(layer).__name__}, not a CellBuffer or a MaskedCellBuffer")
    ct, n = pairs[0][0].cell_type(), pairs[0][0].len()
    for k, (b, _) in enumerate(pairs):
        if b.cell_type() != ct:
            raise EcError(EC_ERR_ARG, f"composite: layer {k} is {CT_NAMES[b.cell_type()]}, layer 0 {CT_NAMES[ct]}: cast the stack to one cell type first")
        if b.len() != n:
            raise EcError(EC_ERR_ARG, f"composite: layer {k} has {b.len()} cells, layer 0 {n}")
    if isinstance(min_count, bool) or not isinstance(min_count, (int, np.integer)) or not 1 <= int(min_count) <= len(pairs):
        raise EcError(EC_ERR_ARG, f"composite: min_count {min_count!r} is not within 1 .. {len(pairs)}, the number of layers")
    return pairs, ct, n


def _stack_call(layers, min_count, aux: bool, result_type, call):
    """What `composite` and `composite_rank` do but for their own arguments: the stack's checks, the result (cells of
    `result_type(cell type)`), its Mask when a layer is masked and the UInt8 `aux` buffer when asked for, and
    `call(cell type, layers, masks or None, K, n, dst, dst_mask or None, aux or None)`, which makes the library call.  A CellBuffer when
    no layer is masked, otherwise a MaskedCellBuffer; with `aux` a pair (result, aux buffer)."""
    pairs, ct, n = _composite_stack(layers, min_count)
    masked = any(m is not None for _, m in pairs)
    out = CellBuffer.empty(n, result_type(ct))
    om = Mask.empty(n) if masked else None
    ax = CellBuffer.empty(n, UInt8) if aux else None
    if n:  # an empty buffer has no memory to point at
        k = len(pairs)
        lp = (C.c_void_p * k)(*[b.mem.ptr for b, _ in pairs])
        mp = (C.c_void_p * k)(*[m.mem.ptr if m is not None else None for _, m in pairs])
        check(call(ct, lp, mp if masked else None, k, n, out.mem.ptr, om.mem.ptr if masked else None, ax.mem.ptr if aux else None))
    res = MaskedCellBuffer(out, om) if masked else out
    return (res, ax) if aux else res


def composite(layers, op="first", min_count: int = 1, aux: bool = False):
    """One buffer from a stack of co-registered `layers` (CellBuffers and MaskedCellBuffers, mixed allowed, one cell type and length), in
    one pass (ec_composite; the rule is in include/erased_cells.h).  `op`: "first" / "last" valid layer, "min" / "max" valid cell, "sum" /
    "mean" of the valid cells (Float64).  A cell is valid when at least `min_count` layers are.  A CellBuffer when no layer is masked,
    otherwise a MaskedCellBuffer; with `aux` a pair (result, UInt8 CellBuffer): the layer each cell came from (255: none), for sum / mean
    the number of valid layers."""
    o = _composite_op(op)
    return _stack_call(layers, min_count, aux, lambda ct: lib().ec_composite_result_type(o, ct),
                       lambda ct, lp, mp, k, n, dst, dm, ax: lib().ec_composite(o, ct, lp, mp, k, n, int(min_count), dst, dm, ax, _stream))


# the spellings of an ec_rank_method
RANK_METHODS = {"lower": EC_RANK_LOWER, "upper": EC_RANK_UPPER}


def _rank_args(q, method, what="composite_rank"):
    """(num, den, ec_rank_method) of `q`, a pair of integers (num, den) with 0 <= num <= den and 1 <= den <= EC_RANK_MAX_DEN, or 0 or 1,
    and of "lower" / "upper" or an ec_rank_method value; anything else is refused.  A float is no exact rational: it is refused."""
    if isinstance(q, (int, np.integer)) and not isinstance(q, bool) and int(q) in (0, 1):
        q = (int(q), 1)
    ok = isinstance(q, (tuple, list)) and len(q) == 2 and all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) for x in q)
    if not ok or not (1 <= int(q[1]) <= EC_RANK_MAX_DEN and 0 <= int(q[0]) <= int(q[1])):
        raise EcError(EC_ERR_ARG, f"{what}: q {q!r} is not a pair of integers (num, den) with 0 <= num <= den and "
                                  f"1 <= den <= EC_RANK_MAX_DEN ({EC_RANK_MAX_DEN})")
    m = RANK_METHODS.get(method, method) if isinstance(method, str) else method
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or int(m) not in (EC_RANK_LOWER, EC_RANK_UPPER):
        raise EcError(EC_ERR_ARG, f"{what}: method {method!r} is not one of {sorted(RANK_METHODS)} or an ec_rank_method value 0..1")
    return int(q[0]), int(q[1]), int(m)


def composite_rank(layers, q=(1, 2), method="lower", min_count: int = 1, aux: bool = False):
    """The per-cell order statistic of a stack of co-registered `layers` (the same kinds as `composite` takes) in one pass
    (ec_composite_rank; the rule is in include/erased_cells.h): the valid cells of each stack in the reference's total order, ties by
    layer index, and the one at position q * (count - 1) kept — rounded down ("lower") or up ("upper"), q = (num, den) an exact
    fraction.  (1, 2) is the median, (0, 1) the minimum, (1, 1) the maximum.  The result has the layers' cell type; a cell is valid
    when at least `min_count` layers are.  A CellBuffer when no layer is masked, otherwise a MaskedCellBuffer; with `aux` a pair
    (result, UInt8 CellBuffer): the layer each cell came from (255: none)."""
    num, den, m = _rank_args(q, method)
    return _stack_call(layers, min_count, aux, lambda ct: ct,
                       lambda ct, lp, mp, k, n, dst, dm, ax: lib().ec_composite_rank(ct, lp, mp, k, n, num, den, m, int(min_count), dst, dm, ax, _stream))


def composite_median(layers, method="lower", min_count: int = 1, aux: bool = False):
    """`composite_rank` at q = 1/2: the lower ("lower") or upper ("upper") median of the valid cells of each stack; they agree where the
    count is odd."""
    return composite_rank(layers, (1, 2), method, min_count, aux)
