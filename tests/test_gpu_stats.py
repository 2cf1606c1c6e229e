"""Band statistics on the device (ec_stats_device / ec_stats_compute / ec_sharded_stats and the Python mirror's `stats()`)
against tests/stats_ref.py — never against the library itself, except where a test says it holds min/max and the count to
ec_min_max and ec_mask_counts.  Records are compared field by field; for the exact integer kind that is the whole answer, for
the pivoted f64 kind the cells are integers within 2^10 of the pivot, so every partial sum of d and of d * d is representable
(n * 2^20 < 2^53) and the record must equal the exact sums whatever order the launch adds them in.

Sizes come from the vector kernels' tile, restated here: 512 threads x 8 loads of 16 bytes (kRBlock, ec_reduce_kernels.hpp;
kReduceU, ec_reduce_plan.hpp), i.e. T = 512 * 8 * (16 / size) cells."""
import ctypes as C
import math
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import stats_ref as R
from reduction_cases import DECOY_STRIDE
from tiff_util import read_tiff

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP = {R.U8: np.uint8, R.U16: np.uint16, R.U32: np.uint32, R.U64: np.uint64, R.I8: np.int8, R.I16: np.int16, R.I32: np.int32,
      R.I64: np.int64, R.F32: np.float32, R.F64: np.float64}
NAMES = {R.U8: "u8", R.U16: "u16", R.U32: "u32", R.U64: "u64", R.I8: "i8", R.I16: "i16", R.I32: "i32", R.I64: "i64", R.F32: "f32", R.F64: "f64"}
KIND0 = [t for t in range(10) if R.KIND[t] == 0]
BASE = {R.U64: 10**9, R.I64: -10**9, R.F64: 10**9, R.F32: 0}  # kind 1: cells are BASE + r, 0 < |r| <= 512


def size_of(ct):
    return np.dtype(NP[ct]).itemsize


def tile(ct):
    return 512 * 8 * (16 // size_of(ct))


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


@pytest.fixture(scope="module")
def slot(ec):
    """64 bytes of device memory for one record."""
    return ec.DeviceMem(64)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def random_cells(ct, n, seed):
    """Random non-zero cells: the whole range for the integer kind, BASE + r with 0 < |r| <= 512 for the f64 kind."""
    rng = np.random.default_rng(seed)
    if R.KIND[ct] == 0:
        info = np.iinfo(NP[ct])
        a = rng.integers(info.min, info.max, size=n, endpoint=True, dtype=np.int64)
        a[a == 0] = 1
        return a.astype(NP[ct])
    r = rng.integers(1, 512, size=n, endpoint=True, dtype=np.int64) * rng.choice(np.array([-1, 1], dtype=np.int64), size=n)
    return (r + BASE[ct]).astype(NP[ct])


def random_mask(n, seed):
    """About a third hidden, every DECOY_STRIDE-th cell among them (a prime: the hidden cells visit every slot, lane and load)."""
    m = (np.random.default_rng(seed).integers(0, 100, size=n) >= 33).astype(np.uint8)
    m[::DECOY_STRIDE] = 0
    return m


def device_record(ec, slot, ct, ptr, mask_ptr, n, stream=None):
    L, E = ec.lib(), ec._ffi
    E.check(L.ec_stats_device(ct, ptr, mask_ptr, n, slot.ptr, stream))
    rec = E.EcMoments()
    E.check(L.ec_download(C.byref(rec), slot.ptr, 64, stream))
    return rec


def assert_record(rec, ref, what):
    assert (rec.count, rec.kind, rec.dtype, rec.reserved) == (ref["count"], ref["kind"], ref["dtype"], 0), what
    dt = ref["dtype"]
    assert (rec.keys2[0], rec.keys2[1]) == (~R.order_key(dt, ref["min"]), R.order_key(dt, ref["max"])), (what, "min/max")
    if ref["kind"] == 0:
        assert (rec.u.i.sum, rec.u.i.sq_lo | (rec.u.i.sq_hi << 64)) == (ref["sum"], ref["sq"]), what
    else:
        got = (bits(rec.u.f.pivot), bits(rec.u.f.s1), bits(rec.u.f.s2))
        assert got == (bits(ref["pivot"]), bits(ref["s1"]), bits(ref["s2"])), (what, rec.u.f.pivot, rec.u.f.s1, rec.u.f.s2, ref["pivot"], ref["s1"], ref["s2"])


def assert_stats(st, exp, dt, what):
    """`st`: an EcStats.  Bit for bit; NaN by class (its sign is the host's choice in both)."""
    assert st.count == exp["count"], what
    for name in ("sum", "mean", "stddev"):
        got, want = getattr(st, name), exp[name]
        assert bits(got) == bits(want) or (math.isnan(got) and math.isnan(want)), (what, name, got, want)
    got = [int(x) for x in np.frombuffer(bytes(st.min) + bytes(st.max), dtype=np.uint64)[[1, 3]]]
    want = [int(np.array([v]).astype(NP[dt]).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[size_of(dt)])[0])
            for v in (exp["min"], exp["max"])]
    assert (st.min.dtype, st.max.dtype, got) == (dt, dt, want), (what, "min/max")


def compute(ec, ct, ptr, mask_ptr, n):
    out = ec._ffi.EcStats()
    ec._ffi.check(ec.lib().ec_stats_compute(ct, ptr, mask_ptr, n, C.byref(out), None))
    return out


def as_ref_record(rec):
    """A downloaded ec_moments as the dict stats_ref.fold takes."""
    dt = rec.dtype
    r = {"count": rec.count, "kind": rec.kind, "dtype": dt, "min": R.key_value(dt, ~rec.keys2[0]), "max": R.key_value(dt, rec.keys2[1])}
    if rec.kind == 0:
        r.update(sum=rec.u.i.sum, sq=rec.u.i.sq_lo | (rec.u.i.sq_hi << 64))
    else:
        r.update(pivot=rec.u.f.pivot, s1=rec.u.f.s1, s2=rec.u.f.s2)
    return r


# ---------------------------------------------------------------- 1. exact records, every type, every place a cell can be lost
@pytest.mark.parametrize("ct", range(10), ids=lambda t: NAMES[t])
def test_exact_records_at_every_size_offset_and_mask(ec, slot, ct):
    T, cpl = tile(ct), 16 // size_of(ct)
    sizes = [0, 1, cpl - 1, T - 1, T, T + 1, 2 * T + cpl + 3]
    pool = random_cells(ct, max(sizes) + 3, 0x57A7 + ct)
    mask = random_mask(pool.size, 0x3A5C + ct)
    dev, dmask = ec.CellBuffer.from_vec(pool), ec.Mask.new(mask.astype(bool))
    assert dev.mem.ptr % 16 == 0 and dmask.mem.ptr % 16 == 0
    host, hmask = pool.tolist(), mask.tolist()
    sz = size_of(ct)
    for off in (0, 1, 3):
        for n in sizes:
            cells = host[off:off + n]
            for masked in (False, True):
                mk = hmask[off:off + n] if masked else None
                what = (NAMES[ct], "n", n, "offset", off, "masked", masked)
                ref = R.record(ct, cells, mk)
                p, pm = dev.mem.ptr + off * sz, (dmask.mem.ptr + off) if masked else None
                assert_record(device_record(ec, slot, ct, p, pm, n), ref, what)
                assert_stats(compute(ec, ct, p, pm, n), R.fold([ref]), ct, what)


# ---------------------------------------------------------------- 2. grid-stride rounds and accumulator width
@pytest.mark.parametrize("ct", KIND0, ids=lambda t: NAMES[t])
def test_capped_grid_all_max_and_all_min(ec, slot, ct):
    """reduce_bpc = 1: one workgroup per CU, and every lane's accumulators carry the most a cell can add.  2^22 + 3 cells are
    at most 256 tiles — one round on 256 CUs — so a second length, 2^24 + 2^22 + 3 cells (320 tiles of bytes, 1280 of 4-byte
    cells), takes the grid-stride loop through further rounds.  The sums are exact; the 32-bit types need sq_hi."""
    info = np.iinfo(NP[ct])
    with ec.tuned(reduce_bpc=1):
        for n, v in [(n, v) for n in (2**22 + 3, 2**24 + 2**22 + 3) for v in (int(info.max), int(info.min))]:
            buf = ec.CellBuffer.fill(n, ec.CellValue(ct, v))
            ref = {"count": n, "kind": 0, "dtype": ct, "min": v, "max": v, "sum": n * v, "sq": n * v * v}
            if size_of(ct) == 4 and v != 0:
                assert ref["sq"] >> 64
            assert_record(device_record(ec, slot, ct, buf.mem.ptr, None, n), ref, (NAMES[ct], v))
            assert_stats(compute(ec, ct, buf.mem.ptr, None, n), R.fold([ref]), ct, (NAMES[ct], v))
    v = C.c_int64(-1)
    ec._ffi.check(ec.lib().ec_stat_get(b"tune.reduce_bpc", C.byref(v)))
    assert v.value == 0


@pytest.mark.parametrize("ct", [R.U8, R.I16, R.U32, R.F64], ids=lambda t: NAMES[t])
def test_cellwise_plan(ec, slot, ct):
    """unaligned_vector = 0 at an odd cell offset: the plan's other outcome, the cell-wise kernel — several workgroups, and under
    reduce_bpc = 1 two rounds of its grid-stride loop (256 threads per workgroup, one workgroup per CU: at most 65536 cells a
    round on 256 CUs)."""
    n, off, sz = 70001, 1, size_of(ct)
    pool = random_cells(ct, n + off, 0xCE11 + ct)
    mask = random_mask(n + off, 0xCE12 + ct)
    dev, dmask = ec.CellBuffer.from_vec(pool), ec.Mask.new(mask.astype(bool))
    refs = {masked: R.record(ct, pool[off:].tolist(), mask[off:].tolist() if masked else None) for masked in (False, True)}
    for knobs in ({"unaligned_vector": 0}, {"unaligned_vector": 0, "reduce_bpc": 1}):
        with ec.tuned(**knobs):
            for masked, ref in refs.items():
                p, pm = dev.mem.ptr + off * sz, (dmask.mem.ptr + off) if masked else None
                assert_record(device_record(ec, slot, ct, p, pm, n), ref, (NAMES[ct], knobs, masked))
                assert_stats(compute(ec, ct, p, pm, n), R.fold([ref]), ct, (NAMES[ct], knobs, masked))


# ---------------------------------------------------------------- 3. masks
@pytest.mark.parametrize("ct", [R.F32, R.F64], ids=lambda t: NAMES[t])
def test_hidden_cells_hold_nan_and_infinities(ec, slot, ct):
    """Every hidden cell is NaN, +Inf or -Inf — the first cell too, so the pivot falls back to 0.0 there: the result is the
    reference's over the visible cells.  All-true and all-false masks included."""
    T = tile(ct)
    n = T + 1
    base = 0 if ct == R.F32 else 2**16  # with the pivot at 0.0 the sums must stay exact: |x| <= 2^16 + 512, n * x^2 < 2^47
    rng = np.random.default_rng(0xBAD + ct)
    vis = (rng.integers(1, 512, size=n, endpoint=True) * rng.choice(np.array([-1, 1]), size=n) + base).astype(NP[ct])
    poison = np.array([np.nan, np.inf, -np.inf], dtype=NP[ct])[rng.integers(0, 3, size=n)]
    for name, mask in (("random, first cell hidden", random_mask(n, 0x111)), ("all true", np.ones(n, np.uint8)), ("all false", np.zeros(n, np.uint8)),
                       ("first cell visible", np.concatenate([[1], random_mask(n - 1, 0x112)]).astype(np.uint8))):
        cells = np.where(mask.astype(bool), vis, poison).astype(NP[ct])
        if name == "random, first cell hidden":
            assert mask[0] == 0 and not np.isfinite(cells[0])
        dev, dmask = ec.CellBuffer.from_vec(cells), ec.Mask.new(mask.astype(bool))
        ref = R.record(ct, cells.tolist(), mask.tolist())
        assert ref["s1_exact"] is not None and ref["count"] == int(mask.sum())
        assert_record(device_record(ec, slot, ct, dev.mem.ptr, dmask.mem.ptr, n), ref, (NAMES[ct], name))
        st = ec.MaskedCellBuffer(dev, dmask).stats()
        exp = R.fold([ref])
        assert st.count == exp["count"] and all(bits(getattr(st, k)) == bits(exp[k]) or (math.isnan(getattr(st, k)) and math.isnan(exp[k]))
                                                for k in ("sum", "mean", "stddev")), (NAMES[ct], name, st, exp)


# ---------------------------------------------------------------- 4. NaN propagation and determinism
@pytest.mark.parametrize("ct", [R.F32, R.F64], ids=lambda t: NAMES[t])
def test_one_visible_nan_propagates(ec, slot, ct):
    n = 2 * tile(ct) + 5
    cells = random_cells(ct, n, 0x4A4)
    mask = random_mask(n, 0x4A5)
    at = n - 7
    mask[at] = 1
    cells[at] = np.nan
    dev, dmask = ec.CellBuffer.from_vec(cells), ec.Mask.new(mask.astype(bool))
    for m in (None, dmask):
        buf = dev if m is None else ec.MaskedCellBuffer(dev, m)
        st = buf.stats()
        assert math.isnan(st.mean) and math.isnan(st.stddev) and math.isnan(st.sum)
        mn, mx = buf.min_max()
        assert (st.min.bits(), st.max.bits()) == (mn.bits(), mx.bits())
        assert st.count == (n if m is None else m.counts()[0])
        ref = R.record(ct, cells.tolist(), None if m is None else mask.tolist())
        rec = device_record(ec, slot, ct, dev.mem.ptr, None if m is None else m.mem.ptr, n)
        assert rec.count == ref["count"] and math.isnan(rec.u.f.s1) and math.isnan(rec.u.f.s2) and bits(rec.u.f.pivot) == bits(ref["pivot"])


def test_same_launch_twice_gives_the_same_bytes(ec, slot):
    n = 2 * tile(R.F64) + 5
    cells = np.random.default_rng(0xDE7).standard_normal(n) * 1e3 + 17.25
    mask = random_mask(n, 0xDE8)
    dev, dmask = ec.CellBuffer.from_vec(cells), ec.Mask.new(mask.astype(bool))
    for pm in (None, dmask.mem.ptr):
        a = bytes(device_record(ec, slot, R.F64, dev.mem.ptr, pm, n))
        b = bytes(device_record(ec, slot, R.F64, dev.mem.ptr, pm, n))
        assert a == b and len(a) == 64


# ---------------------------------------------------------------- 5. general data
def test_general_f64_within_the_summation_bound(ec, slot):
    """Random f64 that is not exactly summable: |s1 - exact| <= gamma * sum|d| and |s2 - exact| <= gamma * sum d^2 with gamma =
    (n + 1) u / (1 - (n + 1) u), u = 2^-53 — the worst case of ANY summation order of n terms, one more rounding for the fma
    (Higham, Accuracy and Stability of Numerical Algorithms, §4.2).  One lost cell changes the sums by about 1 / n of them: five
    orders of magnitude more."""
    n = 2 * tile(R.F64) + 5
    cells = np.random.default_rng(0x6E4).standard_normal(n) * 1e3 + 1e6
    mask = random_mask(n, 0x6E5)
    dev, dmask = ec.CellBuffer.from_vec(cells), ec.Mask.new(mask.astype(bool))
    u = Fraction(1, 2**53)
    for pm, mk in ((None, None), (dmask.mem.ptr, mask.tolist())):
        ref = R.record(R.F64, cells.tolist(), mk)
        m = ref["count"]
        gamma = (m + 1) * u / (1 - (m + 1) * u)
        rec = device_record(ec, slot, R.F64, dev.mem.ptr, pm, n)
        e1, e2 = abs(Fraction(rec.u.f.s1) - ref["s1_exact"]), abs(Fraction(rec.u.f.s2) - ref["s2_exact"])
        print("general f64:", "masked" if mk else "unmasked", "err s1", float(e1), "bound", float(gamma * ref["abs_d"]), "err s2", float(e2),
              "bound", float(gamma * ref["sq_d"]))
        assert rec.count == m and bits(rec.u.f.pivot) == bits(ref["pivot"])
        assert e1 <= gamma * ref["abs_d"] and e2 <= gamma * ref["sq_d"]
        assert float(ref["abs_d"]) / m > 100 * float(gamma * ref["abs_d"])  # a lost cell could not hide inside the bound


# ---------------------------------------------------------------- 6. the reference's known answer
def test_elkton_ndvi_known_answer(ec, golden_dir):
    """src/gdal/rasterband.rs:151-160 checks NDVI's min / max against gdal_calc's STATISTICS_* to 1e-8; MEAN and STDDEV of the same
    figures, which the reference cannot compute, to the same 1e-8."""
    from erased_cells_hip.fused import lazy
    b5, _ = read_tiff(os.path.join(golden_dir, "L8-Elkton-VA-B5.tiff"))
    b4, _ = read_tiff(os.path.join(golden_dir, "L8-Elkton-VA-B4.tiff"))
    nir, red = ec.CellBuffer.from_vec(b5.ravel()), ec.CellBuffer.from_vec(b4.ravel())
    tree = (lazy(nir) - red) / (lazy(nir) + red)
    st = tree.stats()
    assert st.count == b5.size == 31434
    assert abs(st.mean - 0.45559234941397) <= 1e-8 and abs(st.stddev - 0.10447748270797) <= 1e-8
    mn, mx = tree.eval().min_max()
    assert (st.min.bits(), st.max.bits()) == (mn.bits(), mx.bits())
    s5 = nir.stats()
    assert (s5.count, s5.sum) == (31434, 636953871.0)
    rec = device_record(ec, ec.DeviceMem(64), R.U16, nir.mem.ptr, None, nir.n)
    assert (rec.count, rec.u.i.sum, rec.u.i.sq_lo, rec.u.i.sq_hi) == (31434, 636953871, 13233427488439, 0)
    nd_cells, nd = read_tiff(os.path.join(golden_dir, "L8-Elkton-VA-B5-nd.tiff"))
    masked = ec.MaskedCellBuffer.from_vec_with_nodata(nd_cells.ravel(), ec.NoData.new(np.uint16(nd)))
    ms = masked.stats()
    assert ms.count == masked.counts()[0] == int((nd_cells != nd).sum()) < nd_cells.size


# ---------------------------------------------------------------- 7. sharded
@pytest.mark.parametrize("G", [1, 3])
def test_sharded_stats(ec, slot, G):
    from erased_cells_hip import sharded
    rows, cols = 37, 211
    for ct in (R.I16, R.U32, R.F64, R.F32):
        cells = random_cells(ct, rows * cols, 0x5A4D + ct)
        mask = random_mask(rows * cols, 0x5A4E + ct)
        whole = {None: R.record(ct, cells.tolist()), "masked": R.record(ct, cells.tolist(), mask.tolist())}
        with sharded.ShardGroup([0] * G, host_combine=G > 1) as g:
            sb, sm = g.scatter(cells, rows, cols), g.scatter(mask, rows, cols)
            for key, m in ((None, None), ("masked", sm)):
                st = g.stats(sb, m)
                if R.KIND[ct] == 0:  # exact integers: the cut does not matter
                    exp = R.fold([whole[key]])
                    if G > 1:  # ... to the record; the fold merges G records, which stats_ref restates from the cut
                        rng = [sharded.shard_range(rows, cols, i, G) for i in range(G)]
                        parts = [R.record(ct, cells[o:o + ln].tolist(), None if m is None else mask[o:o + ln].tolist()) for o, ln in rng]
                        assert sum(p["sum"] for p in parts) == whole[key]["sum"] and sum(p["sq"] for p in parts) == whole[key]["sq"]
                        exp = R.fold(parts)
                    assert (st.count, st.sum) == (whole[key]["count"], float(whole[key]["sum"]))
                else:  # the fold of the shards' own records, downloaded, in shard order
                    g.sync()
                    recs = [device_record(ec, slot, ct, sb.ptrs[i], None if m is None else m.ptrs[i], sb.lens[i]) for i in range(G)]
                    exp = R.fold([as_ref_record(r) for r in recs])
                    assert sum(r.count for r in recs) == whole[key]["count"]
                for name in ("count", "sum", "mean", "stddev"):
                    got, want = getattr(st, name), exp[name]
                    assert got == want and (name == "count" or bits(got) == bits(want)), (NAMES[ct], G, key, name, got, want)
                assert (R.order_key(ct, st.min.value.item()), R.order_key(ct, st.max.value.item())) == \
                    (R.order_key(ct, whole[key]["min"]), R.order_key(ct, whole[key]["max"]))
            if G == 1 and R.KIND[ct] == 0:
                st = g.stats(sb)
                one = ec.CellBuffer.from_vec(cells).stats()
                assert (st.count, bits(st.sum), bits(st.mean), bits(st.stddev)) == (one.count, bits(one.sum), bits(one.mean), bits(one.stddev))
            sb.free()
            sm.free()


# ---------------------------------------------------------------- 8. graph capture
def _hip():
    """The HIP runtime the process already runs on (torch's copy, which the library shares: erased_cells_hip._ffi.lib)."""
    import torch
    lib = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    for name, args in (("hipStreamBeginCapture", [C.c_void_p, C.c_int]), ("hipStreamEndCapture", [C.c_void_p, C.POINTER(C.c_void_p)]),
                       ("hipGraphGetNodes", [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
                       ("hipGraphGetEdges", [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
                       ("hipGraphInstantiate", [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
                       ("hipGraphLaunch", [C.c_void_p, C.c_void_p]), ("hipGraphExecDestroy", [C.c_void_p]), ("hipGraphDestroy", [C.c_void_p])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C.c_int, args
    return lib


def test_captured_in_a_graph_as_a_single_chain(ec):
    """ec_stats_device inside a stream capture: no allocation, nothing synchronised, the captured nodes form ONE chain (every node
    at most one predecessor and one successor: nothing for the runtime to replay side by side), and two replays on the capture
    stream give the eager record."""
    import torch
    L, E, hip = ec.lib(), ec._ffi, _hip()
    side = torch.cuda.Stream()
    s = side.cuda_stream
    E.check(L.ec_prepare_stream(s))
    slots = {"eager": ec.DeviceMem(64), "graph": ec.DeviceMem(64)}
    for ct, n, masked in ((R.U8, 3 * tile(R.U8) + 21, True), (R.F64, 2 * tile(R.F64) + 5, False), (R.I32, 100, True)):
        cells, mask = random_cells(ct, n, 0x6C4 + ct), random_mask(n, 0x6C5 + ct)
        dev, dmask = ec.CellBuffer.from_vec(cells), ec.Mask.new(mask.astype(bool))
        pm = dmask.mem.ptr if masked else None
        ref = R.record(ct, cells.tolist(), mask.tolist() if masked else None)
        eager = device_record(ec, slots["eager"], ct, dev.mem.ptr, pm, n, s)  # also runs every first-use probe outside the capture
        assert_record(eager, ref, (NAMES[ct], "eager"))
        torch.cuda.synchronize()
        before, after = C.c_int64(), C.c_int64()
        E.check(L.ec_stat_get(b"pool_allocs", C.byref(before)))
        graph, gexec = C.c_void_p(), C.c_void_p()
        assert hip.hipStreamBeginCapture(s, 1) == 0  # hipStreamCaptureModeThreadLocal
        st = L.ec_stats_device(ct, dev.mem.ptr, pm, n, slots["graph"].ptr, s)
        assert hip.hipStreamEndCapture(s, C.byref(graph)) == 0 and graph.value
        E.check(st)
        n_nodes, n_edges = C.c_size_t(), C.c_size_t()
        assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0 and hip.hipGraphGetEdges(graph, None, None, C.byref(n_edges)) == 0
        assert 1 <= n_nodes.value <= 2 and n_edges.value == n_nodes.value - 1, (n_nodes.value, n_edges.value)
        src, dst = (C.c_void_p * max(1, n_edges.value))(), (C.c_void_p * max(1, n_edges.value))()
        assert hip.hipGraphGetEdges(graph, src, dst, C.byref(n_edges)) == 0
        froms, tos = [src[i] for i in range(n_edges.value)], [dst[i] for i in range(n_edges.value)]
        assert len(set(froms)) == len(froms) and len(set(tos)) == len(tos)  # no fork, no join: a chain
        assert hip.hipGraphInstantiate(C.byref(gexec), graph, None, None, 0) == 0
        try:
            for replay in range(2):
                E.check(L.ec_upload(slots["graph"].ptr, bytes(64), 64, s))  # a stale record would show
                assert hip.hipGraphLaunch(gexec, s) == 0
                got = E.EcMoments()
                E.check(L.ec_download(C.byref(got), slots["graph"].ptr, 64, s))
                assert bytes(got) == bytes(eager), (NAMES[ct], "replay", replay)
        finally:
            hip.hipGraphExecDestroy(gexec)
            hip.hipGraphDestroy(graph)
        E.check(L.ec_stat_get(b"pool_allocs", C.byref(after)))
        assert after.value == before.value


# ---------------------------------------------------------------- the C++ mirror
def test_cpp_mirror_stats_program():
    """erased-cells_amd/host/test_stats_mirror.cpp: CellBuffer / MaskedCellBuffer / ShardedCellBuffer stats() of the C++ host mirror on
    hand-checkable cells and against the C ABI called directly."""
    host = os.path.join(ROOT, "erased-cells_amd", "host")
    binary = os.path.join(host, "test_stats_mirror")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", host, "-s", "test_stats_mirror"])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
