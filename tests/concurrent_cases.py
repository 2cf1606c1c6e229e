"""One table of jobs for the concurrency tests (tests/test_gpu_concurrent_families.py): every job is one ABI entry point in one
form, with the inputs of worker k (0 .. 7), the bytes it must leave, and the call itself through a ctypes handle with an explicit
stream.  CPU only: nothing here imports the library — `call` is handed the handle — and every expected byte comes from the
references the families' own tests use (compare_ref, cast_ref, resample_ref, focal_ref, focal_rank_ref, composite_ref,
composite_rank_ref, reclass_ref, stats_ref, zonal_ref, distance_ref, regions_ref) and from the oracle (oracle.eco: min/max, mask
counts, the expression program).

Sizes are the smallest at which concurrency can matter.  Rasters are (96 + 16k) x (80 + 8k) cells, a few tiles of every family in
each direction, so no two workers share an output or a workspace size.  Reductions run over (k mod 4 + 1) T + 2k + 3 cells, T the
vector tile of tests/test_gpu_stats.py: grids of 2, 3, 4 and 5 workgroups, with the worker's minimum, its maximum and a block of
masked-out decoys in the last tile and the two extremes unique to the worker — a finalize step that folds another call's
partials, or too few of its own, is then wrong for certain (tests/test_concurrent_cases.py shows it on the CPU).

A job:
  make(k)                 the inputs of worker k: a dict of numpy arrays and plain parameters; deterministic
  want(inp)               name -> bytes of every output
  call(L, d, s)           the entry point on stream s; d.inp the inputs, d.ptr name -> device address of every array input,
                          every prepared input, every output and every scratch buffer; returns name -> bytes for the outputs
                          that come back on the host (`host`), which it first fills with d.fill
  prepare(L, inp)         name -> bytes of device inputs that only the library's host functions can build (the reclass record)
  scratch(L, inp)         name -> bytes of device workspace
  records                 outputs that are records of 8-byte fields
  reduction               (tile(inp), prefix(inp, n)): a two-launch reduction, its tile and its inputs cut to the first n cells
"""
import ctypes as C
import math
import struct

import numpy as np

import cast_ref
import compare_ref
import composite_rank_ref
import composite_ref
import distance_ref
import focal_rank_ref
import focal_ref
import reclass_ref
import regions_ref
import resample_ref
import stats_ref as R
import zonal_ref
from oracle import eco
from test_gpu_stats import BASE, random_cells
from test_gpu_window import resampled
from vectors import bits_of, rand_cells

U8, U16, U32, U64, I8, I16, I32, I64, F32, F64 = range(10)
NP = compare_ref.NP
WORKERS = 8
TYPES8 = (U8, I16, F64, U32, I8, U16, I64, F32)     # a 1-, 2-, 4- and 8-byte cell among any four workers in a row
M64 = (1 << 64) - 1


def ct_of(k, shift=0):
    return TYPES8[(k + shift) % 8]


def shape(k):
    """(rows, cols) of worker k's raster"""
    return 80 + 8 * k, 96 + 16 * k


def fill_byte(k):
    """the byte worker k's outputs hold before every call"""
    return 0xA1 + 11 * k


def size_of(ct):
    return NP[ct].itemsize


def tile(ct):
    """the reductions' vector tile in cells (tests/test_gpu_stats.py)"""
    return 512 * 8 * (16 // size_of(ct))


def reduction_len(ct, k):
    return (k % 4 + 1) * tile(ct) + 2 * k + 3


def cells(ct, n, seed):
    return rand_cells(ct, n, seed, specials=False)


def mask_bytes(n, seed):
    """about a third hidden"""
    return (np.random.default_rng(seed).integers(0, 100, size=n) >= 33).astype(np.uint8)


def classes(ct, n, seed, n_classes=3):
    return np.random.default_rng(seed).integers(1, n_classes, size=n, endpoint=True).astype(NP[ct])


def reduction_cells(ct, k, seed, masked):
    """(cells, mask or None) for a reduction of worker k: test_gpu_stats.random_cells (the integer kind over its range, the f64
    kind within 2^10 of its pivot, so that every sum is exact in any order), held inside a band; the worker's own minimum at the
    last cell and maximum at the one before, both outside the band and shared with no other worker; with a mask, the rest of the
    last tile hidden and holding values beyond both."""
    n, t = reduction_len(ct, k), tile(ct)
    a = random_cells(ct, n, seed)
    if R.KIND[ct] == 0:
        info = np.iinfo(NP[ct])
        a = np.clip(a, info.min + 16, info.max - 16)
        lo, hi, below, above = info.min + 1 + k, info.max - 1 - k, info.min, info.max
    else:
        lo, hi, below, above = BASE[ct] - 600 - k, BASE[ct] + 600 + k, BASE[ct] - 1000, BASE[ct] + 1000
    a[n - 1], a[n - 2] = lo, hi
    if not masked:
        return a, None
    m = mask_bytes(n, seed ^ 0x3A5C)
    last = (n - 1) // t * t
    assert last == (k % 4 + 1) * t and n - 2 - last == 2 * k + 1
    a[last:n - 2:2], a[last + 1:n - 2:2] = below, above
    m[last:n - 2] = 0
    m[n - 2:] = 1
    return a, m


# ---------------------------------------------------------------- bytes of records
def cell_bits(ct, v):
    return int.from_bytes(np.array([v]).astype(NP[ct]).tobytes(), "little")


def keys_of(ct, mn, mx):
    """{~key(min), key(max)} as ec_min_max_keys writes them"""
    plain = (lambda v: float(v)) if ct in (F32, F64) else (lambda v: int(v))
    return struct.pack("<qq", ~R.order_key(ct, plain(mn)), R.order_key(ct, plain(mx)))


def moments_bytes(r):
    """a stats_ref record as the 64 bytes of an ec_moments"""
    ct = r["dtype"]
    head = struct.pack("<Q", r["count"]) + keys_of(ct, r["min"], r["max"]) + struct.pack("<ii", r["kind"], ct)
    body = struct.pack("<qQQ", r["sum"], r["sq"] & M64, r["sq"] >> 64) if r["kind"] == 0 else struct.pack("<ddd", r["pivot"], r["s1"], r["s2"])
    return head + body + struct.pack("<Q", 0)


def _canonical(x):
    return math.nan if math.isnan(x) else x      # a NaN's sign is the host's choice (tests/test_gpu_stats.py)


def stats_bytes(ct, f):
    """a stats_ref.fold result in the canonical form stats_from_abi gives an ec_stats: the padding left out"""
    return struct.pack("<QBQBQddd", f["count"], ct, cell_bits(ct, f["min"]), ct, cell_bits(ct, f["max"]), _canonical(f["sum"]),
                       _canonical(f["mean"]), _canonical(f["stddev"]))


def stats_from_abi(raw):
    """the 64 bytes of an ec_stats in the same form"""
    count, t0, b0, t1, b1, s, m, d = struct.unpack("<QB7xQB7xQddd", raw)
    return struct.pack("<QBQBQddd", count, t0, b0, t1, b1, _canonical(s), _canonical(m), _canonical(d))


def values_from_abi(raw):
    """ec_value records, 16 bytes each, without their padding"""
    return b"".join(struct.pack("<BQ", *struct.unpack("<B7xQ", raw[i:i + 16])) for i in range(0, len(raw), 16))


# ---------------------------------------------------------------- ctypes helpers: no type of the binding is named here
def ok(L, status):
    if status != 0:
        raise RuntimeError(f"[ec_status {status}] {(L.ec_last_error_string() or b'').decode()}")


def value(ct, x):
    """an ec_value: tag, padding, the cell's bytes"""
    return C.create_string_buffer(struct.pack("<B7xQ", ct, cell_bits(ct, x)), 16)


def arg(fn, i, buf):
    """buf as argument i of fn, whatever pointer type the binding declares for it"""
    if buf is None:
        return None
    return C.cast(C.c_void_p(buf) if isinstance(buf, int) else buf, fn.argtypes[i])


def pointers(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def host_out(d, nbytes):
    buf = C.create_string_buffer(nbytes)
    C.memset(buf, d.fill, nbytes)
    return buf


class Job:
    def __init__(self, name, make, want, call, prepare=None, scratch=None, host=(), records=(), reduction=None):
        self.name, self.make, self._want, self.call = name, make, want, call
        self.prepare, self.scratch, self.host, self.records, self.reduction = prepare, scratch, tuple(host), tuple(records), reduction
        self._inputs, self._expected = {}, {}

    def want(self, inp):
        return self._want(inp)

    def inputs(self, k):
        if k not in self._inputs:
            self._inputs[k] = self.make(k)
        return self._inputs[k]

    def expected(self, k):
        """want(make(k)), computed once"""
        if k not in self._expected:
            self._expected[k] = self.want(self.inputs(k))
        return self._expected[k]


JOBS = []


def job(name, **kw):
    def add(make):
        JOBS.append(Job(name, make, **kw))
        return make
    return add


def opt(d, name):
    return d.ptr.get(name)


# ================================================================ compare / select
def _compare_want(inp):
    return {"out": compare_ref.masked_relation(inp["rel"], inp["lt"], inp["l"], inp.get("lm"), inp["rt"], inp["r"], inp.get("rm")).tobytes()}


def _compare_call(L, d, s):
    i, n = d.inp, d.inp["l"].size
    ok(L, L.ec_compare(i["rel"], i["lt"], d.ptr["l"], opt(d, "lm"), i["rt"], d.ptr["r"], opt(d, "rm"), n, d.ptr["out"], s))


@job("ec_compare", want=_compare_want, call=_compare_call)
def _compare_make(k):
    rows, cols = shape(k)
    n, lt, rt = rows * cols, ct_of(k), ct_of(k, 3)
    l = cells(lt, n, 1000 + k)
    with np.errstate(all="ignore"):
        r = np.where(np.arange(n) % 3 == 0, l.astype(NP[rt]), cells(rt, n, 1100 + k)).astype(NP[rt])   # every third cell a candidate tie
    inp = {"rel": compare_ref.RELS[k % 6], "lt": lt, "rt": rt, "l": l, "r": r}
    if k % 2:
        inp["lm"], inp["rm"] = mask_bytes(n, 1200 + k), mask_bytes(n, 1300 + k)
    return inp


def _compare_scalar_want(inp):
    return {"out": compare_ref.masked_relation(inp["rel"], inp["lt"], inp["l"], inp.get("lm"), inp["lt"], inp["rhs"], None).tobytes()}


def _compare_scalar_call(L, d, s):
    i = d.inp
    rhs = value(i["lt"], i["rhs"])
    ok(L, L.ec_compare_scalar(i["rel"], i["lt"], d.ptr["l"], opt(d, "lm"), i["l"].size, arg(L.ec_compare_scalar, 5, rhs), d.ptr["out"], s))


@job("ec_compare_scalar", want=_compare_scalar_want, call=_compare_scalar_call)
def _compare_scalar_make(k):
    rows, cols = shape(k)
    n, lt = rows * cols, ct_of(k, 1)
    l = cells(lt, n, 1400 + k)
    inp = {"rel": compare_ref.GE if k % 2 else compare_ref.LT, "lt": lt, "l": l, "rhs": np.sort(l)[n // 2 + k]}
    if k % 2 == 0:
        inp["lm"] = mask_bytes(n, 1500 + k)
    return inp


def _select_call(L, d, s):
    ok(L, L.ec_select(d.inp["t"], d.ptr["a"], d.ptr["b"], d.ptr["sel"], d.inp["a"].size, d.ptr["out"], s))


@job("ec_select", want=lambda inp: {"out": compare_ref.select(inp["sel"], inp["a"], inp["b"]).tobytes()}, call=_select_call)
def _select_make(k):
    rows, cols = shape(k)
    n, t = rows * cols, ct_of(k, 2)
    return {"t": t, "a": cells(t, n, 1600 + k), "b": cells(t, n, 1700 + k), "sel": mask_bytes(n, 1800 + k)}


def _masked_select_want(inp):
    out, om = compare_ref.masked_select(inp["sel"], inp["a"], inp["am"], inp["b"], inp["bm"])
    return {"out": out.tobytes(), "out_mask": om.tobytes()}


def _masked_select_call(L, d, s):
    p = d.ptr
    ok(L, L.ec_masked_select(d.inp["t"], p["a"], p["am"], p["b"], p["bm"], p["sel"], d.inp["a"].size, p["out"], p["out_mask"], s))


@job("ec_masked_select", want=_masked_select_want, call=_masked_select_call)
def _masked_select_make(k):
    rows, cols = shape(k)
    n, t = rows * cols, ct_of(k, 5)
    return {"t": t, "a": cells(t, n, 1900 + k), "am": mask_bytes(n, 1910 + k), "b": cells(t, n, 1920 + k), "bm": mask_bytes(n, 1930 + k),
            "sel": mask_bytes(n, 1940 + k)}


# ================================================================ cast
SATURATING = ((F64, I16), (I32, U8), (I64, I16), (F32, U8), (U32, I8), (I16, U8), (F64, I64), (U16, I8))


def _cast_call(L, d, s):
    ok(L, L.ec_cast(cast_ref.ROUND, d.inp["st"], d.ptr["x"], d.inp["dt"], d.ptr["dst"], d.inp["x"].size, s))


@job("ec_cast", want=lambda inp: {"dst": cast_ref.cast(cast_ref.ROUND, inp["st"], inp["x"], inp["dt"]).tobytes()}, call=_cast_call)
def _cast_make(k):
    rows, cols = shape(k)
    st, dt = SATURATING[k]
    x = cells(st, rows * cols, 2000 + k)
    if NP[st].kind == "f":       # half of the cells within the destination's range
        x[::2] = (np.random.default_rng(2050 + k).uniform(-300.0, 40000.0, size=x[::2].size)).astype(NP[st])
    return {"st": st, "dt": dt, "x": x}


SCALED_TARGETS = (I16, U8, F32, I32, F64, U16, I8, I64)


def _cast_scaled_want(inp):
    out = cast_ref.scaled(inp["st"], inp["x"], inp["mask"], inp["scale"], inp["offset"], inp["dt"], inp["nodata"])
    return {"dst": np.asarray(out, dtype=NP[inp["dt"]]).tobytes()}


def _cast_scaled_call(L, d, s):
    i = d.inp
    nd = value(i["dt"], i["nodata"])
    ok(L, L.ec_cast_scaled(i["st"], d.ptr["x"], d.ptr["mask"], i["x"].size, i["scale"], i["offset"], i["dt"], arg(L.ec_cast_scaled, 7, nd), d.ptr["dst"], s))


@job("ec_cast_scaled", want=_cast_scaled_want, call=_cast_scaled_call)
def _cast_scaled_make(k):
    rows, cols = shape(k)
    n, st = rows * cols, cast_ref.SCALED_SOURCES[k % len(cast_ref.SCALED_SOURCES)]
    x = cells(st, n, 2100 + k)
    if NP[st].kind == "f":
        x[::2] = (np.random.default_rng(2150 + k).uniform(-3000.0, 3000.0, size=x[::2].size)).astype(NP[st])
    return {"st": st, "dt": SCALED_TARGETS[k], "x": x, "mask": mask_bytes(n, 2160 + k), "scale": 0.37 + k, "offset": -1.5 - k, "nodata": 7 + k}


# ================================================================ windows
def _window_geometry(k):
    rows, cols = shape(k)
    return rows, cols, 3 + k, 2 + k % 3, cols - 21, rows - 13


def _raster(ct, k, seed, masked=True):
    rows, cols = shape(k)
    a = cells(ct, rows * cols, seed).reshape(rows, cols)
    return a, (mask_bytes(rows * cols, seed + 50).reshape(rows, cols) if masked else None)


def _window_copy_want(inp):
    out, om = resample_ref.resample(resample_ref.NEAREST, inp["a"], inp["m"], *inp["geo"], inp["geo"][2], inp["geo"][3])
    return {"dst": out.tobytes(), "dst_mask": om.tobytes()}


def _window_call(L, d, s):
    i = d.inp
    rows, cols = i["a"].shape
    x0, y0, w, h = i["geo"]
    ow, oh = i.get("out", (w, h))
    ok(L, L.ec_window(i["t"], d.ptr["a"], opt(d, "m"), cols, rows, x0, y0, w, h, ow, oh, d.ptr["dst"], opt(d, "dst_mask"), s))


@job("ec_window(copy)", want=_window_copy_want, call=_window_call)
def _window_copy_make(k):
    t = ct_of(k, 1)
    a, m = _raster(t, k, 2200 + k)
    return {"t": t, "a": a, "m": m, "geo": _window_geometry(k)[2:]}


def _window_nearest_want(inp):
    return {"dst": np.ascontiguousarray(resampled(inp["a"], *inp["geo"], *inp["out"])).tobytes()}


@job("ec_window(nearest)", want=_window_nearest_want, call=_window_call)
def _window_nearest_make(k):
    t = ct_of(k, 4)
    a, _ = _raster(t, k, 2300 + k, masked=False)
    _, _, x0, y0, w, h = _window_geometry(k)
    return {"t": t, "a": a, "geo": (x0, y0, w, h), "out": (2 * w // 3 + 1, 3 * h // 4)}


def _window_put_want(inp):
    rows, cols = inp["shape"]
    x0, y0 = inp["at"]
    h, w = inp["tile"].shape
    dst = np.full(rows * cols * inp["tile"].dtype.itemsize, inp["fill"], np.uint8).view(inp["tile"].dtype).reshape(rows, cols).copy()
    dm = np.full((rows, cols), inp["fill"], np.uint8)
    dst[y0:y0 + h, x0:x0 + w] = inp["tile"]
    dm[y0:y0 + h, x0:x0 + w] = inp["tile_mask"]
    return {"dst": dst.tobytes(), "dst_mask": dm.tobytes()}


def _window_put_call(L, d, s):
    i = d.inp
    rows, cols = i["shape"]
    h, w = i["tile"].shape
    ok(L, L.ec_window_put(i["t"], d.ptr["tile"], d.ptr["tile_mask"], w, h, d.ptr["dst"], d.ptr["dst_mask"], cols, rows, i["at"][0], i["at"][1], s))


@job("ec_window_put", want=_window_put_want, call=_window_put_call)
def _window_put_make(k):
    t = ct_of(k, 6)
    rows, cols, x0, y0, w, h = _window_geometry(k)
    return {"t": t, "shape": (rows, cols), "at": (x0, y0), "tile": cells(t, w * h, 2400 + k).reshape(h, w),
            "tile_mask": mask_bytes(w * h, 2450 + k).reshape(h, w), "fill": fill_byte(k)}   # the raster around the window keeps its pre-fill


def _resample_want(inp):
    out, om = resample_ref.resample(inp["alg"], inp["a"], inp["m"], *inp["geo"], *inp["out"])
    return {"dst": out.tobytes(), "dst_mask": om.tobytes()}


def _resample_call(L, d, s):
    i = d.inp
    rows, cols = i["a"].shape
    ok(L, L.ec_window_resample(i["alg"], i["t"], d.ptr["a"], d.ptr["m"], cols, rows, *i["geo"], *i["out"], d.ptr["dst"], d.ptr["dst_mask"], s))


def _small_values(a, seed):
    """floats of a moderate range, so that a weighted sum neither overflows nor meets an infinity"""
    if a.dtype.kind == "f":
        a[...] = np.random.default_rng(seed).uniform(-1000.0, 1000.0, size=a.shape).astype(a.dtype)
    return a


@job("ec_window_resample(average)", want=_resample_want, call=_resample_call)
def _average_make(k):
    t = ct_of(k, 2)
    a, m = _raster(t, k, 2500 + k)
    ow, oh = 24 + 2 * k, 20 + k
    return {"alg": resample_ref.AVERAGE, "t": t, "a": _small_values(a, 2550 + k), "m": m, "geo": (2, 1, 3 * ow + 2, 2 * oh + 1), "out": (ow, oh)}


@job("ec_window_resample(bilinear)", want=_resample_want, call=_resample_call)
def _bilinear_make(k):
    t = ct_of(k, 7)
    a, m = _raster(t, k, 2600 + k)
    w, h = 20 + 2 * k, 16 + k
    return {"alg": resample_ref.BILINEAR, "t": t, "a": _small_values(a, 2650 + k), "m": m, "geo": (5, 3, w, h), "out": (2 * w + 1, 2 * h - 1)}


# ================================================================ focal
def _two(out):
    return {"dst": np.ascontiguousarray(out[0]).tobytes(), "dst_mask": np.ascontiguousarray(out[1]).tobytes()}


def _focal_want(inp):
    return _two(focal_ref.focal(inp["op"], inp["a"], inp.get("m"), inp["rx"], inp["ry"], whole=bool(inp["flags"] & 1)))


def _focal_call(L, d, s):
    i = d.inp
    rows, cols = i["a"].shape
    ok(L, L.ec_focal(i["op"], i["t"], d.ptr["a"], opt(d, "m"), cols, rows, i["rx"], i["ry"], i["flags"], d.ptr["dst"], d.ptr["dst_mask"], s))


def _focal_make(op, shift, seed):
    def make(k):
        t = ct_of(k, shift)
        a, m = _raster(t, k, seed + k, masked=bool(k % 2))
        inp = {"op": op, "t": t, "a": _small_values(a, seed + 60 + k), "rx": 1 + k % 3, "ry": 1 + k % 2, "flags": 1 if k % 3 == 0 else 0}
        if m is not None:
            inp["m"] = m
        return inp
    return make


job("ec_focal(sum)", want=_focal_want, call=_focal_call)(_focal_make(focal_ref.SUM, 0, 2700))
job("ec_focal(min)", want=_focal_want, call=_focal_call)(_focal_make(focal_ref.MIN, 3, 2800))


def _convolve_want(inp):
    return _two(focal_ref.convolve(inp["a"], inp.get("m"), inp["w"], normalize=bool(inp["flags"] & 2), whole=bool(inp["flags"] & 1)))


def _convolve_call(L, d, s):
    i = d.inp
    rows, cols = i["a"].shape
    ry, rx = i["w"].shape[0] // 2, i["w"].shape[1] // 2
    w = np.ascontiguousarray(i["w"], dtype=np.float64)
    ok(L, L.ec_focal_convolve(i["t"], d.ptr["a"], opt(d, "m"), cols, rows, arg(L.ec_focal_convolve, 5, w.ctypes.data_as(C.c_void_p)), rx, ry, i["flags"],
                              d.ptr["dst"], d.ptr["dst_mask"], s))


@job("ec_focal_convolve", want=_convolve_want, call=_convolve_call)
def _convolve_make(k):
    t = ct_of(k, 5)
    a, m = _raster(t, k, 2900 + k, masked=k % 2 == 0)
    rx, ry = 1 + k % 2, 1 + k % 3
    inp = {"t": t, "a": _small_values(a, 2960 + k), "w": (np.arange((2 * ry + 1) * (2 * rx + 1), dtype=np.float64) * 0.25 - 1.0 + k).reshape(2 * ry + 1, 2 * rx + 1),
           "flags": 2 if k % 2 else 0}
    if m is not None:
        inp["m"] = m
    return inp


def _rank_call(L, d, s):
    i = d.inp
    rows, cols = i["a"].shape
    ok(L, L.ec_focal_rank(i["t"], d.ptr["a"], opt(d, "m"), cols, rows, i["rx"], i["ry"], 1, 2, i["method"], 0, d.ptr["dst"], d.ptr["dst_mask"], s))


@job("ec_focal_rank(median)", want=lambda inp: _two(focal_rank_ref.focal_rank(inp["a"], inp.get("m"), inp["rx"], inp["ry"], 1, 2, inp["method"])), call=_rank_call)
def _rank_make(k):
    t = ct_of(k, 6)
    a, m = _raster(t, k, 3000 + k, masked=bool(k % 2))
    inp = {"t": t, "a": a, "rx": 1 + k % 2, "ry": 1, "method": k % 2}
    if m is not None:
        inp["m"] = m
    return inp


def _majority_call(L, d, s):
    i = d.inp
    rows, cols = i["a"].shape
    ok(L, L.ec_focal_majority(i["t"], d.ptr["a"], opt(d, "m"), cols, rows, i["rx"], i["ry"], 0, d.ptr["dst"], d.ptr["dst_mask"], s))


@job("ec_focal_majority", want=lambda inp: _two(focal_rank_ref.focal_majority(inp["a"], inp.get("m"), inp["rx"], inp["ry"])), call=_majority_call)
def _majority_make(k):
    t = ct_of(k, 2)
    rows, cols = shape(k)
    inp = {"t": t, "a": classes(t, rows * cols, 3100 + k, 4).reshape(rows, cols), "rx": 1 + k % 2, "ry": 1}
    if k % 2 == 0:
        inp["m"] = mask_bytes(rows * cols, 3150 + k).reshape(rows, cols)
    return inp


# ================================================================ composites
def _stack_make(shift, seed, rank):
    def make(k):
        rows, cols = shape(k)
        n, t, layers = rows * cols, ct_of(k, shift), 3 + k % 3
        inp = {"t": t, "n_layers": layers, "min_count": 1 + k % 2}
        for j in range(layers):
            inp[f"layer{j}"] = _small_values(cells(t, n, seed + 10 * k + j), seed + 1000 + 10 * k + j)
            if j:                                     # layer 0 has no mask: every cell of it is valid
                inp[f"mask{j}"] = mask_bytes(n, seed + 500 + 10 * k + j)
        if rank:
            inp["method"] = k % 2
        else:
            inp["op"] = (composite_ref.MAX, composite_ref.MEAN, composite_ref.FIRST, composite_ref.SUM)[k % 4]
        return inp
    return make


def _stack_of(inp):
    ls = [inp[f"layer{j}"] for j in range(inp["n_layers"])]
    return ls, [inp.get(f"mask{j}") for j in range(inp["n_layers"])]


def _three(out):
    return {"dst": np.ascontiguousarray(out[0]).tobytes(), "dst_mask": np.ascontiguousarray(out[1]).tobytes(), "aux": np.ascontiguousarray(out[2]).tobytes()}


def _composite_want(inp):
    ls, ms = _stack_of(inp)
    out = composite_ref.composite(inp["op"], inp["t"], ls, ms, inp["min_count"])
    return _three((np.asarray(out[0], dtype=NP[composite_ref.result_type(inp["op"], inp["t"])]), out[1], out[2]))


def _stack_pointers(d):
    k = d.inp["n_layers"]
    return pointers([d.ptr[f"layer{j}"] for j in range(k)]), pointers([d.ptr.get(f"mask{j}") for j in range(k)])


def _composite_call(L, d, s):
    i = d.inp
    ls, ms = _stack_pointers(d)
    ok(L, L.ec_composite(i["op"], i["t"], ls, ms, i["n_layers"], i["layer0"].size, i["min_count"], d.ptr["dst"], d.ptr["dst_mask"], d.ptr["aux"], s))


job("ec_composite", want=_composite_want, call=_composite_call)(_stack_make(1, 3200, False))


def _composite_rank_want(inp):
    ls, ms = _stack_of(inp)
    return _three(composite_rank_ref.composite_rank(inp["t"], ls, ms, 1, 2, inp["method"], inp["min_count"]))


def _composite_rank_call(L, d, s):
    i = d.inp
    ls, ms = _stack_pointers(d)
    ok(L, L.ec_composite_rank(i["t"], ls, ms, i["n_layers"], i["layer0"].size, 1, 2, i["method"], i["min_count"], d.ptr["dst"], d.ptr["dst_mask"],
                              d.ptr["aux"], s))


job("ec_composite_rank", want=_composite_rank_want, call=_composite_rank_call)(_stack_make(4, 3400, True))


# ================================================================ reclass
def _reclass_want(inp):
    dst, dm = reclass_ref.reclass(inp["t"], inp["x"], inp.get("mask"), inp["t"], inp["breaks"], inp["right"], U8, inp["values"], None, inp.get("nodata"))
    return {"dst": dst.tobytes(), "dst_mask": dm.tobytes()}


def _reclass_prepare(L, inp):
    """the record of worker k's own breaks and class values, built by the library's host function"""
    nb = len(inp["breaks"])
    table = C.create_string_buffer(4384)
    values = C.create_string_buffer(b"".join(struct.pack("<B7xQ", U8, int(v)) for v in inp["values"]), 16 * (nb + 1))
    nodata = value(U8, inp["nodata"]) if "nodata" in inp else None
    fn = L.ec_reclass_table_build
    breaks = np.ascontiguousarray(inp["breaks"], dtype=NP[inp["t"]])
    ok(L, fn(inp["t"], inp["t"], breaks.ctypes.data_as(C.c_void_p), nb, inp["right"], U8, arg(fn, 6, values), None, arg(fn, 8, nodata), table))
    return {"table": table.raw}


def _reclass_call(L, d, s):
    i = d.inp
    ok(L, L.ec_reclass(i["t"], d.ptr["x"], opt(d, "mask"), i["x"].size, U8, d.ptr["table"], d.ptr["dst"], d.ptr["dst_mask"], s))


@job("ec_reclass", want=_reclass_want, call=_reclass_call, prepare=_reclass_prepare)
def _reclass_make(k):
    rows, cols = shape(k)
    n, t = rows * cols, ct_of(k, 3)
    breaks = reclass_ref.gpu_tables(t, t, 6 + k, seed=k)
    inp = {"t": t, "x": cells(t, n, 3600 + k), "breaks": breaks, "right": k % 2, "values": (np.arange(len(breaks) + 1) * 3 + k + 1).astype(np.uint8)}
    if k % 2:
        inp["mask"], inp["nodata"] = mask_bytes(n, 3650 + k), 255
    return inp


# ================================================================ band statistics
def _lists(inp):
    return inp["x"].tolist(), (None if inp.get("mask") is None else inp["mask"].tolist())


def _reduction_prefix(inp, n):
    out = dict(inp)
    for name in ("x", "mask", "y"):
        if inp.get(name) is not None:
            out[name] = inp[name][:n]
    return out


def _by_type(inp):
    return tile(inp["t"])


def _stats_make(seed, shift, short=False):
    def make(k):
        t = ct_of(k, shift)
        a, m = reduction_cells(t, k, seed + k, masked=bool(k % 2))
        if short:      # below one tile: the one-workgroup form, which writes its result itself
            a, m = a[-(1000 + 37 * k):].copy(), (None if m is None else m[-(1000 + 37 * k):].copy())
        return {"t": t, "x": a, "mask": m}
    return make


def _stats_device_call(L, d, s):
    ok(L, L.ec_stats_device(d.inp["t"], d.ptr["x"], opt(d, "mask"), d.inp["x"].size, d.ptr["record"], s))


def _stats_device_want(inp):
    return {"record": moments_bytes(R.record(inp["t"], *_lists(inp)))}


job("ec_stats_device", want=_stats_device_want, call=_stats_device_call, records=("record",), reduction=(_by_type, _reduction_prefix))(_stats_make(4000, 0))
job("ec_stats_device(one workgroup)", want=_stats_device_want, call=_stats_device_call, records=("record",))(_stats_make(4100, 2, short=True))


def _stats_compute_call(L, d, s):
    out = host_out(d, 64)
    ok(L, L.ec_stats_compute(d.inp["t"], d.ptr["x"], opt(d, "mask"), d.inp["x"].size, out, s))
    return {"stats": stats_from_abi(out.raw)}


job("ec_stats_compute", want=lambda inp: {"stats": stats_bytes(inp["t"], R.stats(inp["t"], *_lists(inp)))}, call=_stats_compute_call, host=("stats",),
    records=("stats",))(_stats_make(4200, 4))


# ================================================================ zonal statistics
ZONE_TYPES = (U8, U16, I32)


def _zonal_make(seed, shift):
    def make(k):
        rows, cols = shape(k)
        n, t, zt, n_zones = rows * cols, ct_of(k, shift), ZONE_TYPES[k % 3], 5 + k
        zones = np.random.default_rng(seed + 70 + k).integers(0, n_zones + 1, size=n, endpoint=True)   # n_zones and n_zones + 1 belong to no zone
        if zt == I32:
            zones[::17] = -1 - k
        return {"t": t, "zt": zt, "n_zones": n_zones, "x": random_cells(t, n, seed + k), "zones": zones.astype(NP[zt]),
                "mask": mask_bytes(n, seed + 90 + k) if k % 2 == 0 else None}
    return make


def _zonal_lists(inp):
    return inp["x"].tolist(), inp["zones"].tolist(), inp["n_zones"], (None if inp["mask"] is None else inp["mask"].tolist())


def _zonal_device_call(L, d, s):
    i = d.inp
    ok(L, L.ec_zonal_stats_device(i["t"], d.ptr["x"], opt(d, "mask"), i["zt"], d.ptr["zones"], i["x"].size, i["n_zones"], d.ptr["records"],
                                  d.ptr["workspace"], s))


job("ec_zonal_stats_device", want=lambda inp: {"records": b"".join(moments_bytes(r) for r in zonal_ref.records(inp["t"], *_zonal_lists(inp)))},
    call=_zonal_device_call, scratch=lambda L, inp: {"workspace": L.ec_zonal_workspace_bytes(inp["n_zones"])}, records=("records",))(_zonal_make(4300, 1))


def _zonal_compute_call(L, d, s):
    i = d.inp
    out = host_out(d, 64 * i["n_zones"])
    ok(L, L.ec_zonal_stats_compute(i["t"], d.ptr["x"], opt(d, "mask"), i["zt"], d.ptr["zones"], i["x"].size, i["n_zones"], out, s))
    return {"stats": b"".join(stats_from_abi(out.raw[z * 64:z * 64 + 64]) for z in range(i["n_zones"]))}


job("ec_zonal_stats_compute", want=lambda inp: {"stats": b"".join(stats_bytes(inp["t"], f) for f in zonal_ref.stats(inp["t"], *_zonal_lists(inp)))},
    call=_zonal_compute_call, host=("stats",), records=("stats",))(_zonal_make(4400, 5))


def _broadcast_want(inp):
    out, om = zonal_ref.broadcast(inp["zones"], inp["table"], inp["n_zones"])
    return {"dst": np.array(out).astype(NP[inp["t"]]).tobytes(), "dst_mask": np.array(om, np.uint8).tobytes()}


def _broadcast_call(L, d, s):
    i = d.inp
    ok(L, L.ec_zonal_broadcast(i["zt"], d.ptr["zones"], i["zones"].size, i["n_zones"], i["t"], d.ptr["table"], d.ptr["dst"], d.ptr["dst_mask"], s))


@job("ec_zonal_broadcast", want=_broadcast_want, call=_broadcast_call)
def _broadcast_make(k):
    inp = _zonal_make(4500, 3)(k)
    return {"t": inp["t"], "zt": inp["zt"], "n_zones": inp["n_zones"], "zones": inp["zones"], "table": cells(inp["t"], inp["n_zones"], 4550 + k)}


# ================================================================ distance, regions: the caller's workspace and the library's
def _distance_make(k):
    rows, cols = shape(k)
    m = (np.random.default_rng(4600 + k).integers(0, 400, size=(rows, cols)) == 0).astype(np.uint8)
    m[rows // 2 + k, cols // 3] = 1
    return {"mask": m, "max_sq": distance_ref.UNLIMITED if k % 2 == 0 else (10 + k) ** 2, "out_type": F64 if k % 4 < 2 else U32}


def _distance_call(workspace):
    def call(L, d, s):
        i = d.inp
        rows, cols = i["mask"].shape
        ok(L, L.ec_distance(d.ptr["mask"], cols, rows, i["max_sq"], i["out_type"], d.ptr["dst"], d.ptr["dst_mask"], d.ptr["workspace"] if workspace else None, s))
    return call


def _distance_workspace(L, inp):
    return {"workspace": L.ec_distance_workspace_bytes(inp["mask"].shape[1], inp["mask"].shape[0])}


_distance_memo = {}


def _distance_want(inp):
    key = inp["mask"].tobytes()     # both forms of a worker share one answer
    if key not in _distance_memo:
        _distance_memo[key] = _two(distance_ref.distance(inp["mask"], inp["max_sq"], inp["out_type"]))
    return _distance_memo[key]


job("ec_distance(caller's workspace)", want=_distance_want, call=_distance_call(True), scratch=_distance_workspace)(_distance_make)
job("ec_distance(library's workspace)", want=_distance_want, call=_distance_call(False))(_distance_make)


def _regions_make(k):
    rows, cols = shape(k)
    t = ct_of(k, 7)
    return {"t": t, "a": classes(t, rows * cols, 4700 + k, 2).reshape(rows, cols),
            "m": (np.random.default_rng(4750 + k).integers(0, 100, size=(rows, cols)) >= 12).astype(np.uint8), "connectivity": 8 if k % 2 else 4, "min_cells": 3 + k}


_regions_memo = {}


def _regions_want(inp):
    key = inp["a"].tobytes() + inp["m"].tobytes()
    if key not in _regions_memo:
        labels, dm, count = regions_ref.regions(inp["a"], inp["m"], inp["connectivity"], regions_ref.DENSE, inp["min_cells"])
        _regions_memo[key] = {"dst": labels.tobytes(), "dst_mask": dm.tobytes(), "n_regions": struct.pack("<Q", count)}
    return _regions_memo[key]


def _regions_call(workspace):
    def call(L, d, s):
        i = d.inp
        rows, cols = i["a"].shape
        ok(L, L.ec_regions(i["t"], d.ptr["a"], d.ptr["m"], cols, rows, i["connectivity"], regions_ref.DENSE, i["min_cells"], d.ptr["dst"], d.ptr["dst_mask"],
                           d.ptr["n_regions"], d.ptr["workspace"] if workspace else None, s))
    return call


def _regions_workspace(L, inp):
    return {"workspace": L.ec_regions_workspace_bytes(inp["a"].shape[1], inp["a"].shape[0])}


job("ec_regions(caller's workspace)", want=_regions_want, call=_regions_call(True), scratch=_regions_workspace)(_regions_make)
job("ec_regions(library's workspace)", want=_regions_want, call=_regions_call(False))(_regions_make)


# ================================================================ the older users of the stream's scratch
def _min_max_want(inp):
    mn, mx = eco.min_max(inp["x"], inp.get("mask"))
    return {"keys": keys_of(inp["t"], mn.get(), mx.get())}


def _min_max_keys_call(L, d, s):
    ok(L, L.ec_min_max_keys(d.inp["t"], d.ptr["x"], opt(d, "mask"), d.inp["x"].size, d.ptr["keys"], s))


job("ec_min_max_keys", want=_min_max_want, call=_min_max_keys_call, records=("keys",), reduction=(_by_type, _reduction_prefix))(_stats_make(4800, 6))


def _min_max_call(L, d, s):
    out = host_out(d, 32)
    fn = L.ec_min_max
    ok(L, fn(d.inp["t"], d.ptr["x"], opt(d, "mask"), d.inp["x"].size, arg(fn, 4, out), arg(fn, 5, C.addressof(out) + 16), s))
    return {"values": values_from_abi(out.raw)}


def _min_max_values_want(inp):
    mn, mx = eco.min_max(inp["x"], inp.get("mask"))
    return {"values": struct.pack("<BQBQ", inp["t"], mn.bits(), inp["t"], mx.bits())}


job("ec_min_max", want=_min_max_values_want, call=_min_max_call, host=("values",))(_stats_make(4900, 1))


def _counts_make(k):
    n = reduction_len(U8, k)
    m = mask_bytes(n, 5000 + k)
    m[(n - 1) // tile(U8) * tile(U8):n - 2] = 0     # the last tile's block of masked-out cells
    return {"t": U8, "x": m}


def _counts_want(inp):
    return {"counts": struct.pack("<QQ", *eco.mask_counts(inp["x"]))}


def _counts_device_call(L, d, s):
    ok(L, L.ec_mask_counts_device(d.ptr["x"], d.inp["x"].size, d.ptr["counts"], s))


job("ec_mask_counts_device", want=_counts_want, call=_counts_device_call, records=("counts",), reduction=(_by_type, _reduction_prefix))(_counts_make)


def _counts_call(L, d, s):
    out = host_out(d, 16)
    fn = L.ec_mask_counts
    ok(L, fn(d.ptr["x"], d.inp["x"].size, arg(fn, 2, out), arg(fn, 3, C.addressof(out) + 8), s))
    return {"counts": out.raw}


job("ec_mask_counts", want=_counts_want, call=_counts_call, host=("counts",), records=("counts",))(_counts_make)

EXPR_STEPS = bytes([eco.SUB, 0, 1, 0, eco.MUL, 4, 8, 1])     # reg0 = stream0 - stream1; reg1 = reg0 * scalar0
EXPR_SCALAR = 2.5


def _expr_make(k):
    """(x - y) * 2.5 over u16 cells: the f64 result is what the reduction folds, so the tile is the f64 one; the worker's extremes
    in the last tile as above"""
    n = reduction_len(F64, k)
    rng = np.random.default_rng(5100 + k)
    x, y = rng.integers(100, 40000, size=n).astype(np.uint16), rng.integers(100, 40000, size=n).astype(np.uint16)
    x[n - 2], y[n - 2] = 60000 + 7 * k, 0
    x[n - 1], y[n - 1] = 0, 60000 + 7 * k
    mask = None
    if k % 2:
        mask = mask_bytes(n, 5150 + k)
        last = (n - 1) // tile(F64) * tile(F64)
        x[last:n - 2:2], y[last:n - 2:2] = 65535, 0
        x[last + 1:n - 2:2], y[last + 1:n - 2:2] = 0, 65535
        mask[last:n - 2] = 0
        mask[n - 2:] = 1
    return {"t": F64, "x": x, "y": y, "mask": mask}


def _expr_want(inp):
    r = eco.f_binop_scalar(eco.MUL, eco.f_binop(eco.SUB, inp["x"], inp["y"]), eco.Value.of(eco.F64, EXPR_SCALAR))
    mn, mx = eco.f_min_max(r, inp["mask"])
    return {"keys": keys_of(F64, mn.get(), mx.get())}


def _expr_call(L, d, s):
    fn = L.ec_expr_min_max_keys
    dt = (C.c_uint8 * 2)(U16, U16)
    masks = pointers([d.ptr["mask"], d.ptr["mask"]]) if d.inp["mask"] is not None else None
    scalar, steps = value(F64, EXPR_SCALAR), C.create_string_buffer(EXPR_STEPS, len(EXPR_STEPS))
    ok(L, fn(dt, pointers([d.ptr["x"], d.ptr["y"]]), masks, 2, arg(fn, 4, scalar), 1, arg(fn, 6, steps), 2, d.inp["x"].size, d.ptr["keys"], s))


job("ec_expr_min_max_keys", want=_expr_want, call=_expr_call, records=("keys",), reduction=(lambda inp: tile(F64), _reduction_prefix))(_expr_make)


def _difference_make(k):
    t = ct_of(k, 3)
    x, _ = reduction_cells(t, k, 5200 + k, masked=False)
    y = x.copy()
    at = x.size - 1 - k                             # in the last tile; every later cell differs too
    bits_of(y)[at:] ^= 1
    return {"t": t, "x": x, "y": y}


def _difference_want(inp):
    differ = np.flatnonzero(bits_of(inp["x"]) != bits_of(inp["y"]))
    return {"index": struct.pack("<Q", int(differ[0]) if differ.size else inp["x"].size)}


def _difference_call(L, d, s):
    out = host_out(d, 8)
    fn = L.ec_first_difference
    ok(L, fn(d.inp["t"], d.ptr["x"], d.ptr["y"], d.inp["x"].size, arg(fn, 4, out), s))
    return {"index": out.raw}


job("ec_first_difference", want=_difference_want, call=_difference_call, host=("index",), records=("index",),
    reduction=(_by_type, _reduction_prefix))(_difference_make)

BY_NAME = {j.name: j for j in JOBS}
assert len(BY_NAME) == len(JOBS)


# ================================================================ the checker
def check(want, got, fill):
    """The complaints about one call's outputs `got` (name -> bytes) against `want`; none when every byte is right.  `fill` is the
    byte the outputs held before the call: an output that still holds it everywhere is reported as such."""
    out = []
    for name, w in want.items():
        g = got.get(name)
        if g is None:
            out.append(f"{name}: no output")
        elif len(g) != len(w):
            out.append(f"{name}: {len(g)} bytes, expected {len(w)}")
        elif g != w:
            if g == bytes([fill]) * len(g):
                out.append(f"{name}: still at its pre-fill")
            else:
                a, b = np.frombuffer(g, np.uint8), np.frombuffer(w, np.uint8)
                bad = np.flatnonzero(a != b)
                out.append(f"{name}: {bad.size} of {len(w)} bytes differ, the first at {int(bad[0])}")
    return out


def first_difference(a, b):
    """the first offset at which two byte strings differ within their common length, or None"""
    n = min(len(a), len(b))
    bad = np.flatnonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))
    return int(bad[0]) if bad.size else None
