"""The in-process sharded path and the runtime around it, through the C ABI.

`examples/sharded.c` is a plain C program (no torch, no Python) that drives an ec_shard_group: row-block
scatter, per-shard divide, RCCL all-reduce of the min/max keys and of the counts.  A 1-GPU box can run it
with one device over RCCL (a 1-rank clique) and with the same device listed several times under
EC_GROUP_HOST_COMBINE (the fan-out threads, shard ranges and the combine are all exercised; only the xGMI
hop is not).  Every number it prints is recomputed here with the oracle.
"""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

from oracle import eco

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "erased-cells_amd")


def _build(tmp_path):
    exe = str(tmp_path / "sharded_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-O1", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "sharded.c"), "-L" + LIBDIR, "-lerased_cells_hip",
                        "-Wl,-rpath," + LIBDIR, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_sharded_example_is_plain_c99_and_links():
    import tempfile
    import pathlib
    with tempfile.TemporaryDirectory() as d:
        _build(pathlib.Path(d))


def _expected(rows, cols, n_shards):
    cells = rows * cols
    k = np.arange(cells, dtype=np.uint64)
    x = (((k * np.uint64(2654435761)) >> np.uint64(13)) & np.uint64(0xFFFF)).astype(np.uint16)
    x[(x == 0) | (x == 65535)] = 1
    d = (np.uint64(1) + (k * np.uint64(40503)) % np.uint64(65535)).astype(np.uint16)
    q, rem = divmod(rows, n_shards)
    lens = [(q + (1 if g < rem else 0)) * cols for g in range(n_shards)]
    x[cells - 1 - lens[-1] // 2] = 0
    x[lens[0] // 2] = 65535
    mn, mx = eco.min_max(x)
    qq = eco.f_binop(eco.DIV, x, d)
    qmn, qmx = eco.f_min_max(qq)
    m = eco.mask_from_nodata(x, eco.ND_VALUE, eco.Value.of(eco.U16, 7))
    data, nodata = eco.mask_counts(m)
    return f"min {int(mn.get())} max {int(mx.get())} qmin {qmn.bits()} qmax {qmx.bits()} data {data} nodata {nodata}"


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("devices,host_combine", [(["0"], 0), (["0"], 1), (["0", "0"], 1), (["0", "0", "0", "0", "0"], 1)])
def test_sharded_path_from_plain_c(tmp_path, devices, host_combine):
    rows, cols = 1031, 997  # rows not divisible by the shard counts: ragged row-blocks
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    r = subprocess.run([_build(tmp_path), str(rows), str(cols), str(host_combine)] + devices, capture_output=True, text=True,
                       timeout=500, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("min ")]
    assert lines == [_expected(rows, cols, len(devices))], r.stdout


@pytest.mark.gpu
def test_duplicate_device_needs_host_combine(tmp_path):
    r = subprocess.run([_build(tmp_path), "64", "64", "0", "0", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "listed twice" in r.stderr


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_comm_bootstrap_through_the_abi(ec):
    """ec_comm_get_unique_id / ec_comm_init_rank / ec_comm_init_all / ec_comm_destroy: communicators made by the
    library itself (1 rank is what one GPU allows) carry the reduction payloads unchanged."""
    from erased_cells_hip import sharded
    from vectors import rand_cells, rand_mask
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    L, chk = ec.lib(), ec._ffi.check
    a, m = rand_cells(eco.I32, 300007, 11), rand_mask(300007, 12)
    d, dm = ec.CellBuffer.from_vec(a), ec.Mask.new(m)
    uid, comm = ec._ffi.EcCommUid(), C.c_void_p()
    chk(L.ec_comm_get_unique_id(C.byref(uid)))
    chk(L.ec_comm_init_rank(C.byref(uid), 1, 0, C.byref(comm)))
    comms = (C.c_void_p * 1)()
    chk(L.ec_comm_init_all((C.c_int32 * 1)(0), 1, comms))
    try:
        for cm in (comm, C.c_void_p(comms[0])):
            keys, counts = ec.DeviceMem(16), ec.DeviceMem(16)
            chk(L.ec_min_max_keys(ec.Int32, d.mem.ptr, dm.mem.ptr, d.len(), keys.ptr, None))
            chk(L.ec_allreduce_min_max_keys(cm, keys.ptr, None))
            chk(L.ec_mask_counts_device(dm.mem.ptr, dm.len(), counts.ptr, None))
            chk(L.ec_allreduce_counts(cm, counts.ptr, None))
            k, c = np.empty(2, np.int64), np.empty(2, np.uint64)
            chk(L.ec_download(k.ctypes.data_as(C.c_void_p), keys.ptr, 16, None))
            chk(L.ec_download(c.ctypes.data_as(C.c_void_p), counts.ptr, 16, None))
            mn, mx = sharded.combine_min_max_keys(ec.Int32, (int(k[0]), int(k[1])))
            emn, emx = eco.f_min_max(a, m)
            assert (mn.bits(), mx.bits()) == (emn.bits(), emx.bits())
            assert (int(c[0]), int(c[1])) == eco.mask_counts(m)
        assert L.ec_comm_init_rank(C.byref(uid), 1, 1, C.byref(C.c_void_p())) == ec._ffi.EC_ERR_ARG
        assert L.ec_comm_init_all((C.c_int32 * 2)(0, 0), 2, (C.c_void_p * 2)()) == ec._ffi.EC_ERR_ARG
    finally:
        chk(L.ec_comm_destroy(comm))
        chk(L.ec_comm_destroy(comms[0]))


@pytest.mark.gpu
def test_shard_group_from_python_matches_oracle(ec):
    """The same group API through ctypes: 3 shards (one device, host combine) of a masked f32 raster; an empty shard
    (more shards than rows) contributes the idempotent sentinels."""
    from erased_cells_hip import sharded
    from vectors import rand_cells, rand_mask
    L, chk = ec.lib(), ec._ffi.check
    for rows, cols, G in ((50, 401, 3), (2, 17, 4)):
        a, m = rand_cells(eco.F32, rows * cols, 21), rand_mask(rows * cols, 22)
        grp = C.c_void_p()
        chk(L.ec_shard_group_create((C.c_int32 * G)(*([0] * G)), G, 1, C.byref(grp)))
        try:
            assert L.ec_shard_group_size(grp) == G
            rng = [sharded.shard_range(rows, cols, g, G) for g in range(G)]
            n = (C.c_size_t * G)(*[r[1] for r in rng])
            b4, b1 = (C.c_size_t * G)(*[r[1] * 4 for r in rng]), (C.c_size_t * G)(*[r[1] for r in rng])
            o4, o1 = (C.c_size_t * G)(*[r[0] * 4 for r in rng]), (C.c_size_t * G)(*[r[0] for r in rng])
            da, dm = (C.c_void_p * G)(), (C.c_void_p * G)()
            chk(L.ec_sharded_alloc(grp, b4, da))
            chk(L.ec_sharded_alloc(grp, b1, dm))
            chk(L.ec_sharded_upload(grp, da, a.ctypes.data_as(C.c_void_p), o4, b4))
            chk(L.ec_sharded_upload(grp, dm, m.ctypes.data_as(C.c_void_p), o1, b1))
            mn, mx = ec._ffi.EcValue(), ec._ffi.EcValue()
            chk(L.ec_sharded_min_max(grp, ec.Float32, da, dm, n, C.byref(mn), C.byref(mx)))
            emn, emx = eco.f_min_max(a, m)
            assert (ec.CellValue.from_ec(mn).bits(), ec.CellValue.from_ec(mx).bits()) == (emn.bits(), emx.bits())
            t, f = C.c_uint64(), C.c_uint64()
            chk(L.ec_sharded_counts(grp, dm, n, C.byref(t), C.byref(f)))
            assert (t.value, f.value) == eco.mask_counts(m)
            back = np.empty_like(a)
            chk(L.ec_sharded_download(grp, back.ctypes.data_as(C.c_void_p), da, o4, b4))
            assert np.array_equal(back.view(np.uint32), a.view(np.uint32))
            dev, st = C.c_int32(-1), C.c_void_p()
            chk(L.ec_shard_group_shard(grp, G - 1, C.byref(dev), C.byref(st)))
            assert dev.value == 0 and st.value
            assert L.ec_shard_group_shard(grp, G, None, None) == ec._ffi.EC_ERR_ARG
            chk(L.ec_shard_group_sync(grp))
            chk(L.ec_sharded_free(grp, da))
            chk(L.ec_sharded_free(grp, dm))
        finally:
            chk(L.ec_shard_group_destroy(grp))


@pytest.mark.gpu
@pytest.mark.timeout(180)
@pytest.mark.parametrize("blocking", [0, 2], ids=["fire-and-forget", "blocking-issue"])
def test_shard_group_calls_are_issued_in_order_and_failures_do_not_hang(ec, blocking):
    """Round 3: element-wise sharded calls return once their jobs are queued.  (1) A chain of dependent calls — each
    reads what the one before wrote, the ctypes argument arrays of each call are dropped at once — gives the oracle's
    result: the per-shard pointers are copied and every device issues in call order.  (2) A shard that cannot take part
    in a reduction (NULL pointer with cells to read) is refused on the calling thread with EC_ERR_ARG — before any
    launch thread has enqueued a collective, so nothing waits for a missing rank (round 2: the other shards hung).
    (3) A failure inside a queued job is kept by the group and returned once by the next sync / reduction."""
    from erased_cells_hip import sharded
    from vectors import rand_cells
    L, chk, E = ec.lib(), ec._ffi.check, ec._ffi
    G, rows, cols = 3, 41, 257
    a = rand_cells(eco.U16, rows * cols, 31, specials=False)
    a[a == 0] = 1
    grp = C.c_void_p()
    chk(L.ec_shard_group_create((C.c_int32 * G)(*([0] * G)), G, 1 | blocking, C.byref(grp)))
    try:
        v = C.c_int64(-1)
        chk(L.ec_shard_group_stat(grp, b"blocking_issue", C.byref(v)))
        assert v.value == (1 if blocking else 0)
        rng = [sharded.shard_range(rows, cols, g, G) for g in range(G)]
        lens = [r[1] for r in rng]

        def sizes(item):
            return (C.c_size_t * G)(*[ln * item for ln in lens])

        def offs(item):
            return (C.c_size_t * G)(*[r[0] * item for r in rng])

        da, t0, t1 = (C.c_void_p * G)(), (C.c_void_p * G)(), (C.c_void_p * G)()
        chk(L.ec_sharded_alloc(grp, sizes(2), da))
        chk(L.ec_sharded_alloc(grp, sizes(8), t0))
        chk(L.ec_sharded_alloc(grp, sizes(8), t1))
        chk(L.ec_sharded_upload(grp, da, a.ctypes.data_as(C.c_void_p), offs(2), sizes(2)))
        # (1) t0 = a + a; then 24 dependent steps t_next = t_prev op a, ping-pong between t0 and t1
        chk(L.ec_shard_group_stat(grp, b"jobs_posted", C.byref(v)))
        posted0 = v.value
        chk(L.ec_sharded_binop(grp, eco.ADD, eco.U16, (C.c_void_p * G)(*da), eco.U16, (C.c_void_p * G)(*da), (C.c_size_t * G)(*lens), (C.c_void_p * G)(*t0)))
        exp = eco.f_binop(eco.ADD, a, a)
        src, dst = t0, t1
        for k in range(24):
            op = (eco.MUL, eco.SUB, eco.DIV, eco.ADD)[k % 4]
            chk(L.ec_sharded_binop(grp, op, eco.F64, (C.c_void_p * G)(*src), eco.U16, (C.c_void_p * G)(*da), (C.c_size_t * G)(*lens),
                                   (C.c_void_p * G)(*dst)))  # temporaries: gone when the call returns
            exp = eco.f_binop(op, exp, a)
            src, dst = dst, src
        chk(L.ec_shard_group_stat(grp, b"jobs_posted", C.byref(v)))
        assert v.value - posted0 == (0 if blocking else 25 * G)
        back = np.empty(rows * cols, np.float64)
        chk(L.ec_sharded_download(grp, back.ctypes.data_as(C.c_void_p), src, offs(8), sizes(8)))  # queued behind the launches
        assert np.array_equal(back.view(np.uint64), exp.view(np.uint64))
        # (2) arguments are checked before any fan-out
        n = (C.c_size_t * G)(*lens)
        holed = (C.c_void_p * G)(*da)
        holed[1] = None
        mn, mx = E.EcValue(), E.EcValue()
        t, f = C.c_uint64(), C.c_uint64()
        assert L.ec_sharded_min_max(grp, eco.U16, holed, None, n, C.byref(mn), C.byref(mx)) == E.EC_ERR_ARG
        assert b"p[1] is null" in L.ec_last_error_string()
        assert L.ec_sharded_min_max(grp, eco.U16, da, holed, n, C.byref(mn), C.byref(mx)) == E.EC_ERR_ARG
        assert L.ec_sharded_counts(grp, holed, n, C.byref(t), C.byref(f)) == E.EC_ERR_ARG
        assert L.ec_sharded_binop(grp, eco.ADD, eco.U16, holed, eco.U16, da, n, t0) == E.EC_ERR_ARG
        assert L.ec_sharded_binop(grp, eco.ADD, eco.U16, da, eco.U16, da, n, holed) == E.EC_ERR_ARG
        assert L.ec_sharded_binop(grp, eco.ADD, 10, da, eco.U16, da, n, t0) == E.EC_ERR_UNSUPPORTED_TYPE
        assert L.ec_sharded_min_max(grp, 10, da, None, n, C.byref(mn), C.byref(mx)) == E.EC_ERR_UNSUPPORTED_TYPE
        assert L.ec_sharded_convert(grp, eco.F64, t0, eco.U16, da, n) == E.EC_ERR_NARROWING
        empty_ok = (C.c_size_t * G)(lens[0], 0, lens[2])  # ... but a shard with no cells may have no pointer
        chk(L.ec_sharded_min_max(grp, eco.U16, holed, None, empty_ok, C.byref(mn), C.byref(mx)))
        part = np.concatenate([a[rng[0][0]:rng[0][0] + lens[0]], a[rng[2][0]:rng[2][0] + lens[2]]])
        emn, emx = eco.f_min_max(part)
        assert (ec.CellValue.from_ec(mn).bits(), ec.CellValue.from_ec(mx).bits()) == (emn.bits(), emx.bits())
        # the group is still usable
        chk(L.ec_sharded_min_max(grp, eco.U16, da, None, n, C.byref(mn), C.byref(mx)))
        emn, emx = eco.f_min_max(a)
        assert (ec.CellValue.from_ec(mn).bits(), ec.CellValue.from_ec(mx).bits()) == (emn.bits(), emx.bits())
        # (3) a job that fails after the call has returned
        if not blocking:
            chk(L.ec_tune_set(b"inject_shard_failure", 2))  # shard 1's next job
            chk(L.ec_sharded_binop(grp, eco.ADD, eco.U16, da, eco.U16, da, n, t0))  # returns EC_OK: only queued
            st = L.ec_shard_group_sync(grp)
            assert st == E.EC_ERR_HIP and b"shard 1" in L.ec_last_error_string() and b"injected" in L.ec_last_error_string()
            chk(L.ec_shard_group_sync(grp))  # reported once
            chk(L.ec_tune_set(b"inject_shard_failure", 1))
            chk(L.ec_sharded_binop(grp, eco.ADD, eco.U16, da, eco.U16, da, n, t0))
            assert L.ec_sharded_min_max(grp, eco.F64, t0, None, n, C.byref(mn), C.byref(mx)) == E.EC_ERR_HIP  # its input is suspect
            chk(L.ec_sharded_min_max(grp, eco.U16, da, None, n, C.byref(mn), C.byref(mx)))
        chk(L.ec_shard_group_stat(grp, b"poisoned", C.byref(v)))
        assert v.value == 0
        for p in (da, t0, t1):
            chk(L.ec_sharded_free(grp, p))
    finally:
        chk(L.ec_tune_set(b"inject_shard_failure", 0))
        chk(L.ec_shard_group_destroy(grp))


@pytest.mark.gpu
def test_device_selection_and_pool(ec):
    L, chk = ec.lib(), ec._ffi.check
    dev = C.c_int32(-1)
    chk(L.ec_get_device(C.byref(dev)))
    assert dev.value == 0
    chk(L.ec_set_device(0))
    import torch
    bad = torch.cuda.device_count()  # first index that does not exist
    assert L.ec_set_device(bad) == ec._ffi.EC_ERR_NOT_INITIALIZED
    assert L.ec_init(bad) == ec._ffi.EC_ERR_ARG
    # pooled blocks: allocate on one stream, last use on another, free ordered behind that use
    s1, s2 = C.c_void_p(), C.c_void_p()
    chk(L.ec_stream_create(C.byref(s1)))
    chk(L.ec_stream_create(C.byref(s2)))
    n = 1 << 22
    a = np.arange(n, dtype=np.uint16)
    src = ec.CellBuffer.from_vec(a)
    for _ in range(8):
        p, q = C.c_void_p(), C.c_void_p()
        chk(L.ec_alloc_async(C.byref(p), 4 * n, s1))
        chk(L.ec_stream_sync(s1))
        chk(L.ec_convert(ec.UInt16, src.mem.ptr, ec.Float32, p, n, s2))   # last use on s2
        chk(L.ec_free_ordered(p, s1, s2))                                   # returned on s1, behind s2's kernel
        chk(L.ec_alloc_async(C.byref(q), 4 * n, s1))                        # may be the same block again
        chk(L.ec_convert(ec.UInt16, src.mem.ptr, ec.Int32, q, n, s1))
        got = np.empty(n, np.int32)
        chk(L.ec_download(got.ctypes.data_as(C.c_void_p), q, 4 * n, s1))
        assert np.array_equal(got, a.astype(np.int32))
        chk(L.ec_free_async(q, s1))
    chk(L.ec_stream_sync(s2))
    chk(L.ec_pool_trim(0))
    chk(L.ec_tune_set(b"pool_keep_mb", 1024))
    chk(L.ec_tune_set(b"pool_keep_mb", 32768))
    chk(L.ec_stream_destroy(s1))
    chk(L.ec_stream_destroy(s2))


@pytest.mark.gpu
def test_scratch_table_is_bounded_and_streams_can_be_released(ec):
    """More streams than the library keeps scratch for (64 per device): the least recently used entries are recycled
    and every stream still gets the right answer, also when it comes back after its entry was dropped."""
    from vectors import rand_cells
    L, chk = ec.lib(), ec._ffi.check
    a = rand_cells(eco.I16, 70001, 31)
    d = ec.CellBuffer.from_vec(a)
    emn, emx = eco.f_min_max(a)
    streams = []
    for _ in range(80):
        s = C.c_void_p()
        chk(L.ec_stream_create(C.byref(s)))
        streams.append(s)
    for rnd in range(2):
        for s in streams:
            mn, mx = ec._ffi.EcValue(), ec._ffi.EcValue()
            chk(L.ec_min_max(ec.Int16, d.mem.ptr, None, d.len(), C.byref(mn), C.byref(mx), s))
            assert (ec.CellValue.from_ec(mn).bits(), ec.CellValue.from_ec(mx).bits()) == (emn.bits(), emx.bits())
    chk(L.ec_release_stream(streams[0]))
    chk(L.ec_release_stream(streams[0]))  # idempotent
    for s in streams:
        chk(L.ec_stream_destroy(s))


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_host_threads_sharing_one_stream_take_turns(ec):
    """Synchronous-result entry points on ONE stream from several host threads: all five go through one hand-over that guards
    the stream's result slots (the pinned words of ec_min_max, ec_mask_counts and ec_first_difference, the device slots of
    ec_stats_compute's record and ec_expr_min_max's keys), so each thread reads its own answer, every time.  Past one workgroup:
    the partials and the finalize launches share the scratch as well."""
    import stats_ref
    from vectors import rand_cells, rand_mask
    L, E, chk = ec.lib(), ec._ffi, ec._ffi.check
    s = C.c_void_p()
    chk(L.ec_stream_create(C.byref(s)))
    one_u16 = (C.c_uint8 * 1)(ec.UInt16)
    add_1_5 = ((E.EcValue * 1)(ec.CellValue.new(1.5).to_ec()), (E.EcExprStep * 1)(E.EcExprStep(eco.ADD, 0, 8, 0)))  # s0 + k0
    cases = []
    for i in range(4):
        a = rand_cells(eco.U16, 50000 + 977 * i, 41 + i)
        m = rand_mask(a.size, 51 + i)
        other, at = a.copy(), 30011 + 4099 * i  # one planted difference, beyond the first workgroup's tile
        other[at] ^= 1
        plus = eco.f_min_max(eco.f_binop(eco.ADD, a, np.full(a.size, 1.5)))
        cases.append((ec.CellBuffer.from_vec(a), ec.Mask.new(m), eco.f_min_max(a), eco.mask_counts(m),
                      ec.CellBuffer.from_vec(other), at, stats_ref.stats(stats_ref.U16, a), plus))
    errors = []

    def f64_bits(x):
        return np.float64(x).view(np.uint64)

    def work(i):
        try:
            buf, msk, (emn, emx), ecnt, other, at, est, (pmn, pmx) = cases[i]
            for _ in range(200):
                mn, mx = E.EcValue(), E.EcValue()
                chk(L.ec_min_max(ec.UInt16, buf.mem.ptr, None, buf.len(), C.byref(mn), C.byref(mx), s))
                assert (ec.CellValue.from_ec(mn).bits(), ec.CellValue.from_ec(mx).bits()) == (emn.bits(), emx.bits())
                t, f = C.c_uint64(), C.c_uint64()
                chk(L.ec_mask_counts(msk.mem.ptr, msk.len(), C.byref(t), C.byref(f), s))
                assert (t.value, f.value) == ecnt
                idx = C.c_uint64(0)
                chk(L.ec_first_difference(ec.UInt16, buf.mem.ptr, other.mem.ptr, buf.len(), C.byref(idx), s))
                assert idx.value == at
                st = E.EcStats()
                chk(L.ec_stats_compute(ec.UInt16, buf.mem.ptr, None, buf.len(), C.byref(st), s))
                got = (st.count, st.min.dtype, st.max.dtype, ec.CellValue.from_ec(st.min).bits(), ec.CellValue.from_ec(st.max).bits(),
                       f64_bits(st.sum), f64_bits(st.mean), f64_bits(st.stddev))
                assert got == (est["count"], ec.UInt16, ec.UInt16, est["min"], est["max"],
                               f64_bits(est["sum"]), f64_bits(est["mean"]), f64_bits(est["stddev"])), ("stats", got, est)
                mn, mx = E.EcValue(), E.EcValue()
                chk(L.ec_expr_min_max(one_u16, (C.c_void_p * 1)(buf.mem.ptr), None, 1, add_1_5[0], 1, add_1_5[1], 1, buf.len(),
                                      C.byref(mn), C.byref(mx), s))
                assert (ec.CellValue.from_ec(mn).bits(), ec.CellValue.from_ec(mx).bits()) == (pmn.bits(), pmx.bits())
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errors, errors[:3]
    chk(L.ec_stream_destroy(s))


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_shard_group_property_any_shape_any_shard_count(ec):
    """Property test (hypothesis): any raster shape (ragged, fewer rows than shards, empty), shard count, cell type
    and mask gives the whole raster's answers — scatter/gather round trip, per-shard divide, min_max (masked and
    not) and counts, against the oracle on the unsharded data."""
    import os
    from hypothesis import HealthCheck, given, settings, strategies as st
    from erased_cells_hip import sharded
    from vectors import bits_of, rand_cells, rand_mask
    L, chk = ec.lib(), ec._ffi.check
    groups = {}
    try:
        for G in (1, 2, 3, 8):
            g = C.c_void_p()
            chk(L.ec_shard_group_create((C.c_int32 * G)(*([0] * G)), G, 1, C.byref(g)))
            groups[G] = g
        pool = {ct: rand_cells(ct, 40000 + 64, 700 + ct) for ct in range(eco.NTYPES)}  # 40 x 1000 cells + the largest offset
        mpool = rand_mask(40000 + 64, 77)

        @settings(max_examples=int(os.environ.get("EC_PROP_EXAMPLES", "120")), deadline=None, suppress_health_check=list(HealthCheck))
        @given(G=st.sampled_from([1, 2, 3, 8]), rows=st.integers(0, 40), cols=st.sampled_from([0, 1, 7, 64, 333, 1000]),
               ct=st.integers(0, eco.NTYPES - 1), rt=st.integers(0, eco.NTYPES - 1), off=st.integers(0, 37), masked=st.booleans())
        def prop(G, rows, cols, ct, rt, off, masked):
            n = rows * cols
            a, b, m = pool[ct][off:off + n], pool[rt][off + 1:off + 1 + n], mpool[off:off + n]
            assert a.size == b.size == m.size == n
            grp = groups[G]
            rng = [sharded.shard_range(rows, cols, g, G) for g in range(G)]
            assert sum(r[1] for r in rng) == n and all(rng[i][0] + rng[i][1] == rng[i + 1][0] for i in range(G - 1))
            lens = (C.c_size_t * G)(*[r[1] for r in rng])
            sa, sb = a.dtype.itemsize, b.dtype.itemsize

            def sizes(sz):
                return (C.c_size_t * G)(*[r[1] * sz for r in rng]), (C.c_size_t * G)(*[r[0] * sz for r in rng])

            (ba, oa), (bb, ob), (b8, o8), (b1, o1) = sizes(sa), sizes(sb), sizes(8), sizes(1)
            da, db, dq, dm = (C.c_void_p * G)(), (C.c_void_p * G)(), (C.c_void_p * G)(), (C.c_void_p * G)()
            for d, bts in ((da, ba), (db, bb), (dq, b8), (dm, b1)):
                chk(L.ec_sharded_alloc(grp, bts, d))
            try:
                aa, bb_, mm = np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(m)
                chk(L.ec_sharded_upload(grp, da, aa.ctypes.data_as(C.c_void_p), oa, ba))
                chk(L.ec_sharded_upload(grp, db, bb_.ctypes.data_as(C.c_void_p), ob, bb))
                chk(L.ec_sharded_upload(grp, dm, mm.ctypes.data_as(C.c_void_p), o1, b1))
                chk(L.ec_sharded_binop(grp, ec.DIV, ct, da, rt, db, lens, dq))
                q = np.empty(n, np.float64)
                chk(L.ec_sharded_download(grp, q.ctypes.data_as(C.c_void_p), dq, o8, b8))
                from vectors import assert_f64_bits_equal
                assert_f64_bits_equal(q, eco.f_binop(eco.DIV, aa, bb_))
                mn, mx = ec._ffi.EcValue(), ec._ffi.EcValue()
                chk(L.ec_sharded_min_max(grp, ct, da, dm if masked else None, lens, C.byref(mn), C.byref(mx)))
                emn, emx = eco.f_min_max(aa, mm if masked else None)
                assert (ec.CellValue.from_ec(mn).bits(), ec.CellValue.from_ec(mx).bits()) == (emn.bits(), emx.bits())
                t, f = C.c_uint64(), C.c_uint64()
                chk(L.ec_sharded_counts(grp, dm, lens, C.byref(t), C.byref(f)))
                assert (t.value, f.value) == eco.mask_counts(mm)
            finally:
                for d in (da, db, dq, dm):
                    chk(L.ec_sharded_free(grp, d))

        prop()
    finally:
        for g in groups.values():
            chk(L.ec_shard_group_destroy(g))


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 3, 8])
def test_config5_ndvi_in_one_process_over_a_shard_group(ec, golden_dir, G):
    """BASELINE config 5 from ONE process: the reference's GDAL test (src/gdal/rasterband.rs:166-191) on its own
    fixtures — bands scattered as row-blocks over the group's devices (169 rows over 8 shards: 22, 21 x 7), nodata
    masks, u16 -> f32 convert and the fused NDVI fanned out per shard with ec_shard_group_foreach (no communication),
    then data/nodata counts and min/max through the sharded reductions; the reference's known answers."""
    from erased_cells_hip import raster, sharded
    L, chk = ec.lib(), ec._ffi.check
    red_rb = raster.RasterBand.open(os.path.join(golden_dir, "L8-Elkton-VA-B4.tiff"))
    nir_rb = raster.RasterBand.open(os.path.join(golden_dir, "L8-Elkton-VA-B5-nd.tiff"))
    cols, rows = red_rb.size()
    red_h, nir_h = red_rb.cells, nir_rb.cells
    assert red_rb.no_data_value() == 0.0 and nir_rb.no_data_value() == 0.0  # GDAL_NODATA = "0" on both fixtures
    with sharded.ShardGroup([0] * G, host_combine=G > 1) as g:
        red, nir = g.scatter(red_h, rows, cols), g.scatter(nir_h, rows, cols)
        if G == 8:
            assert [ln // cols for ln in red.lens] == [22, 21, 21, 21, 21, 21, 21, 21]
        lens = red.lens
        red_f, nir_f = g.alloc(ec.Float32, lens), g.alloc(ec.Float32, lens)
        red_m, nir_m, out_m = g.alloc(ec.UInt8, lens), g.alloc(ec.UInt8, lens), g.alloc(ec.UInt8, lens)
        out = g.alloc(ec.Float64, lens)
        nd = ec.CellValue(ec.UInt16, 0).to_ec()

        def per_shard(i, device, stream):
            n = lens[i]
            chk(L.ec_mask_from_nodata(ec.UInt16, red.ptrs[i], n, C.byref(nd), red_m.ptrs[i], stream))
            chk(L.ec_mask_from_nodata(ec.UInt16, nir.ptrs[i], n, C.byref(nd), nir_m.ptrs[i], stream))
            chk(L.ec_convert(ec.UInt16, red.ptrs[i], ec.Float32, red_f.ptrs[i], n, stream))
            chk(L.ec_convert(ec.UInt16, nir.ptrs[i], ec.Float32, nir_f.ptrs[i], n, stream))
            dt = (C.c_uint8 * 4)(ec.Float32, ec.Float32, ec.Float32, ec.Float32)
            p = (C.c_void_p * 4)(nir_f.ptrs[i], red_f.ptrs[i], nir_f.ptrs[i], red_f.ptrs[i])
            m = (C.c_void_p * 4)(nir_m.ptrs[i], red_m.ptrs[i], nir_m.ptrs[i], red_m.ptrs[i])
            chk(L.ec_masked_fused(ec.SUB, ec.DIV, ec.ADD, dt, p, m, None, n, out.ptrs[i], out_m.ptrs[i], stream))

        g.foreach(per_shard)
        assert g.counts(out_m) == (31430, 4)                                  # rasterband.rs:180-183
        # the same pipeline through the sharded entry points (what a C caller without callbacks uses), eager chain
        n_arr = (C.c_size_t * G)(*lens)
        red_m2, nir_m2, m_sub, m_add, m_div = (g.alloc(ec.UInt8, lens) for _ in range(5))
        t_sub, t_add, out2 = (g.alloc(ec.Float64, lens) for _ in range(3))
        chk(L.ec_sharded_mask_from_nodata(g.handle, ec.UInt16, red.ptrs, n_arr, C.byref(nd), red_m2.ptrs))
        chk(L.ec_sharded_mask_from_nodata(g.handle, ec.UInt16, nir.ptrs, n_arr, C.byref(nd), nir_m2.ptrs))
        chk(L.ec_sharded_convert(g.handle, ec.UInt16, red.ptrs, ec.Float32, red_f.ptrs, n_arr))
        chk(L.ec_sharded_convert(g.handle, ec.UInt16, nir.ptrs, ec.Float32, nir_f.ptrs, n_arr))
        assert L.ec_sharded_convert(g.handle, ec.Float32, red_f.ptrs, ec.UInt16, red.ptrs, n_arr) == ec._ffi.EC_ERR_NARROWING
        for op, dst, dm_ in ((ec.SUB, t_sub, m_sub), (ec.ADD, t_add, m_add)):
            chk(L.ec_sharded_masked_binop(g.handle, op, ec.Float32, nir_f.ptrs, nir_m2.ptrs, ec.Float32, red_f.ptrs, red_m2.ptrs,
                                          n_arr, dst.ptrs, dm_.ptrs))
        chk(L.ec_sharded_masked_binop(g.handle, ec.DIV, ec.Float64, t_sub.ptrs, m_sub.ptrs, ec.Float64, t_add.ptrs, m_add.ptrs,
                                      n_arr, out2.ptrs, m_div.ptrs))
        assert np.array_equal(g.gather(out2).view(np.uint64), g.gather(out).view(np.uint64))
        assert np.array_equal(g.gather(m_div), g.gather(out_m)) and g.counts(m_div) == (31430, 4)
        # and the fused form fanned out by the library: (nir - red) / (nir + 2.5) with a scalar operand, unmasked
        dt4 = (C.c_uint8 * 4)(ec.Float32, ec.Float32, ec.Float32, 0)
        PVP = C.POINTER(C.c_void_p)
        p4 = (PVP * 4)(C.cast(nir_f.ptrs, PVP), C.cast(red_f.ptrs, PVP), C.cast(nir_f.ptrs, PVP), PVP())
        sc = (ec._ffi.EcValue * 4)()
        sc[3] = ec.CellValue.new(2.5).to_ec()
        chk(L.ec_sharded_fused(g.handle, ec.SUB, ec.DIV, ec.ADD, dt4, p4, None, sc, n_arr, out2.ptrs, None))
        nf, rf = eco.f_convert(nir_h.ravel(), eco.F32), eco.f_convert(red_h.ravel(), eco.F32)
        exp = eco.f_binop(eco.DIV, eco.f_binop(eco.SUB, nf, rf), eco.f_binop_scalar(eco.ADD, nf, eco.Value.of(eco.F64, 2.5)))
        assert np.array_equal(g.gather(out2).view(np.uint64), exp.view(np.uint64))
        # an expression program fanned out by the library: EVI-shaped, (nir - red) * 2.5 / (nir + 6 red + 1), masked and plain
        E = ec._ffi
        S, R, K = (lambda k: k), (lambda k: 4 + k), (lambda k: 8 + k)
        prog = [(ec.SUB, S(0), S(1), 0), (ec.MUL, R(0), K(0), 0), (ec.MUL, S(1), K(1), 1), (ec.ADD, S(0), R(1), 1), (ec.ADD, R(1), K(2), 1),
                (ec.DIV, R(0), R(1), 0)]
        st = (E.EcExprStep * len(prog))(*[E.EcExprStep(*q) for q in prog])
        ks = (E.EcValue * 3)(*[ec.CellValue.new(x).to_ec() for x in (2.5, 6.0, 1.0)])
        dt2 = (C.c_uint8 * 2)(ec.UInt16, ec.Float32)
        p2 = (PVP * 2)(C.cast(nir.ptrs, PVP), C.cast(red_f.ptrs, PVP))
        m2 = (PVP * 2)(C.cast(nir_m2.ptrs, PVP), C.cast(red_m2.ptrs, PVP))
        chk(L.ec_sharded_expr(g.handle, dt2, p2, None, 2, ks, 3, st, len(prog), n_arr, out2.ptrs, None))
        nh = nir_h.ravel()
        full = lambda c: np.full(nh.size, c)  # noqa: E731
        top = eco.f_binop(eco.MUL, eco.f_binop(eco.SUB, nh, rf), full(2.5))
        bot = eco.f_binop(eco.ADD, eco.f_binop(eco.ADD, nh, eco.f_binop(eco.MUL, rf, full(6.0))), full(1.0))
        exp = eco.f_binop(eco.DIV, top, bot)
        assert np.array_equal(g.gather(out2).view(np.uint64), exp.view(np.uint64))
        chk(L.ec_sharded_expr(g.handle, dt2, p2, m2, 2, ks, 3, st, len(prog), n_arr, t_sub.ptrs, m_sub.ptrs))
        assert np.array_equal(g.gather(t_sub).view(np.uint64), exp.view(np.uint64)) and g.counts(m_sub) == (31430, 4)
        bad = (E.EcExprStep * 1)(E.EcExprStep(ec.ADD, S(0), R(2), 0))  # register 2 read before any step wrote it: refused on the calling thread
        assert L.ec_sharded_expr(g.handle, dt2, p2, None, 2, ks, 3, bad, 1, n_arr, out2.ptrs, None) == E.EC_ERR_ARG
        assert L.ec_sharded_expr(g.handle, dt2, p2, m2, 2, ks, 3, st, len(prog), n_arr, out2.ptrs, None) == E.EC_ERR_ARG  # masks without out_mask
        g.sync()  # nothing deferred
        via_mirror, via_mirror_mask = g.program([nir, red_f], [2.5, 6.0, 1.0], prog, masks=[nir_m2, red_m2])
        assert np.array_equal(g.gather(via_mirror).view(np.uint64), exp.view(np.uint64)) and g.counts(via_mirror_mask) == (31430, 4)
        via_mirror.free()
        via_mirror_mask.free()
        # statistics of the program over the whole raster without the raster: per-shard keys, one exchange — interpreted (two
        # passes per shard) and compiled (the reduce kernel), plain and masked; the masked answer is the reference's NDVI-like one
        whole = ec.fused.program([ec.CellBuffer.from_vec(nh), ec.CellBuffer.from_vec(rf)], [2.5, 6.0, 1.0], prog).min_max()
        for mode in (0, 2):
            chk(L.ec_tune_set(b"expr_jit", mode))
            try:
                mn_, mx_ = g.program_min_max([nir, red_f], [2.5, 6.0, 1.0], prog)
                assert (mn_.bits(), mx_.bits()) == (whole[0].bits(), whole[1].bits())
                mn_m, mx_m = g.program_min_max([nir, red_f], [2.5, 6.0, 1.0], prog, masks=[nir_m2, red_m2])
                valid_h = (nh != 0) & (red_h.ravel() != 0)
                assert float(mn_m.value) == float(exp[valid_h].min()) and float(mx_m.value) == float(exp[valid_h].max())
            finally:
                chk(L.ec_tune_set(b"expr_jit", 1))
        # the compiled form from the group's launch threads at once (expr_jit = 2: the first thread to arrive compiles, the
        # others wait for it; one module load per device)
        chk(L.ec_tune_set(b"expr_jit", 2))
        try:
            prog2 = prog[:-1] + [(ec.DIV, R(1), R(0), 3)]  # a program no other test has compiled
            v = C.c_int64(0)
            chk(L.ec_stat_get(b"expr_jit_launches", C.byref(v)))
            before = v.value
            compiled = g.program([nir, red_f], [2.5, 6.0, 1.0], prog2)
            g.sync()
            chk(L.ec_stat_get(b"expr_jit_launches", C.byref(v)))
            assert v.value == before + G
            assert np.array_equal(g.gather(compiled).view(np.uint64), eco.f_binop(eco.DIV, bot, top).view(np.uint64))
            compiled.free()
        finally:
            chk(L.ec_tune_set(b"expr_jit", 1))
        for b in (red_m2, nir_m2, m_sub, m_add, m_div, t_sub, t_add, out2):
            b.free()
        mn, mx = g.min_max(out, out_m)
        assert float(mn.value).hex() == "-0x1.ff8ca5bcc77dcp-4" and float(mx.value).hex() == "0x1.5708125b0ed28p-1"
        # and cell for cell against the oracle's chain on the whole raster
        e = eco.f_binop(eco.DIV, eco.f_binop(eco.SUB, eco.f_convert(nir_h.ravel(), eco.F32), eco.f_convert(red_h.ravel(), eco.F32)),
                        eco.f_binop(eco.ADD, eco.f_convert(nir_h.ravel(), eco.F32), eco.f_convert(red_h.ravel(), eco.F32)))
        from vectors import assert_f64_bits_equal
        assert_f64_bits_equal(g.gather(out), e)
        with pytest.raises(ZeroDivisionError):
            g.foreach(lambda i, d, s: 1 // 0)                                 # a failing shard function surfaces here
        for b in (red, nir, red_f, nir_f, red_m, nir_m, out_m, out):
            b.free()


def _build_example(tmp_path, name):
    exe = str(tmp_path / name)
    r = subprocess.run(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Wextra", "-Werror", "-pedantic", "-O1",
                        "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", name + ".c"), "-L" + LIBDIR, "-lerased_cells_hip",
                        "-Wl,-rpath," + LIBDIR, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_lifecycle_example_is_plain_c99_and_links(tmp_path):
    _build_example(tmp_path, "lifecycle")


@pytest.mark.gpu
def test_runtime_lifecycle_init_shutdown_init_from_plain_c(tmp_path):
    """ec_init -> work -> ec_shutdown (pool destroyed, scratch freed) -> ec_init again, three times over, in one process."""
    r = subprocess.run([_build_example(tmp_path, "lifecycle")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["round", "0", "ok", "round", "1", "ok", "round", "2", "ok"]


def test_rank_example_is_plain_c99_and_links(tmp_path):
    _build_example(tmp_path, "rank")


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_one_process_per_gpu_shape_without_torch(tmp_path):
    """examples/rank.c: the one-process-per-GPU shape through the ABI's own communicator bootstrap (unique id handed
    over in a file).  One GPU allows one rank; its answers are the whole raster's, recomputed by the oracle."""
    rows, cols = 257, 1021
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    r = subprocess.run([_build_example(tmp_path, "rank"), str(tmp_path / "ec.uid"), "1", "0", "0", str(rows), str(cols)],
                       capture_output=True, text=True, timeout=250, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("rank 0: ")]
    assert lines == ["rank 0: " + _expected(rows, cols, 1)], r.stdout
    assert not (tmp_path / "ec.uid").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 3, 8])
def test_host_to_host_over_a_shard_group_on_the_fixtures(ec, golden_dir, G):
    """`ec_sharded_host_expr`: the reference's GDAL NDVI tests (src/gdal/rasterband.rs:138-191) with the bands in host memory
    and the row-blocks streamed through the group's devices side by side (169 rows over 8 shards: 22, 21 x 7); plain and
    masked; the reference's known answers (B.25-B.27), and the same cells as the one-pipeline form."""
    from erased_cells_hip import raster, sharded
    red_rb = raster.RasterBand.open(os.path.join(golden_dir, "L8-Elkton-VA-B4.tiff"))
    nir_rb = raster.RasterBand.open(os.path.join(golden_dir, "L8-Elkton-VA-B5-nd.tiff"))
    cols, rows = red_rb.size()
    red_h, nir_h = red_rb.cells.ravel(), nir_rb.cells.ravel()
    S, R = (lambda k: k), (lambda k: 4 + k)
    ndvi = [(ec.SUB, S(0), S(1), 0), (ec.ADD, S(0), S(1), 1), (ec.DIV, R(0), R(1), 0)]
    one = ec.fused.program_host_masked([nir_h, red_h], [0, 0], [], ndvi, out_nodata=-9999.0, want_mask=True)
    with sharded.ShardGroup([0] * G, host_combine=G > 1) as g:
        out, valid = g.program_host([nir_h, red_h], [], ndvi, rows, cols, nodata=[0, 0], out_nodata=-9999.0, want_mask=True, chunk_cells=1500)
        assert (int(valid.sum()), int((~valid).sum())) == (31430, 4)
        assert np.array_equal(out.view(np.uint64), one[0].view(np.uint64)) and np.array_equal(valid, one[1])
        assert float(out[valid].min()).hex() == "-0x1.ff8ca5bcc77dcp-4" and float(out[valid].max()).hex() == "0x1.5708125b0ed28p-1"
        plain = g.program_host([nir_h, red_h], [], ndvi, rows, cols)
        assert np.array_equal(plain.view(np.uint64), ec.fused.program_host([nir_h, red_h], [], ndvi).view(np.uint64))
        bad = [(ec.ADD, S(0), R(3), 0)]
        with pytest.raises(Exception):
            g.program_host([nir_h, red_h], [], bad, rows, cols)


_REFUSED_PIN_BODY = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import erased_cells_hip as ec
from erased_cells_hip import sharded
refuse, tmp = sys.argv[2] == "1", sys.argv[3]
ec.init(0)
rows, cols = 3000, 4001  # 12 M cells: 132 MB over the link — above the 64 MiB from which the pipelines page-lock at all
n = rows * cols
rng = np.random.default_rng(7)
a = rng.integers(1, 60000, n, dtype=np.uint16)
b = rng.integers(0, 200, n, dtype=np.uint8)
a.tofile(tmp + "/a.bin")
b.tofile(tmp + "/b.bin")
ra = np.memmap(tmp + "/a.bin", dtype=np.uint16, mode="r")  # PROT_READ, file-backed
rb = np.memmap(tmp + "/b.bin", dtype=np.uint8, mode="r")
S, R = (lambda k: k), (lambda k: 4 + k)
prog = [(ec.SUB, S(0), S(1), 0), (ec.ADD, S(0), S(1), 1), (ec.DIV, R(0), R(1), 0)]
af, bf = a.astype(np.float64), b.astype(np.float64)
exp = (af - bf) / (af + bf)
L = ec.lib()
ec._ffi.check(L.ec_tune_set(b"inject_pin_refusal", 1 if refuse else 0))
one = ec.fused.program_host([ra, rb], [], prog, chunk_cells=1_000_000)
assert np.array_equal(one.view(np.uint64), exp.view(np.uint64))
for G in (1, 3):
    with sharded.ShardGroup([0] * G, host_combine=G > 1) as g:
        out = g.program_host([ra, rb], [], prog, rows, cols, chunk_cells=1_000_000)
        assert np.array_equal(out.view(np.uint64), exp.view(np.uint64)), G
        out, valid = g.program_host([ra, rb], [], prog, rows, cols, nodata=[None, 0], out_nodata=-1.0, want_mask=True, chunk_cells=1_000_000)
        assert np.array_equal(valid, b != 0) and np.array_equal(out[valid].view(np.uint64), exp[valid].view(np.uint64))
        assert np.all(out[~valid] == -1.0)
        # chunk_cells = 0 takes the one-chunk form below 64 MiB: it enters its ranges with use_all and must pass a refused entry of its caller too
        out = g.program_host([ra, rb], [], prog, rows, cols)
        assert np.array_equal(out.view(np.uint64), exp.view(np.uint64)), G
        # a nodata value of the wrong cell type is refused on the calling thread, before any page is locked
        k = 2
        dt = (C.c_uint8 * k)(ec.UInt16, ec.UInt8)
        p = (C.c_void_p * k)(ra.ctypes.data, rb.ctypes.data)
        wrong = ec.CellValue(ec.UInt16, 0).to_ec()
        nd = (C.POINTER(ec._ffi.EcValue) * k)(C.POINTER(ec._ffi.EcValue)(), C.pointer(wrong))
        st = (ec._ffi.EcExprStep * len(prog))(*[ec._ffi.EcExprStep(*q) for q in prog])
        o = np.empty(n)
        try:
            ec._ffi.check(L.ec_sharded_host_expr(g.handle, dt, p, nd, k, None, 0, st, len(prog), rows, cols, o.ctypes.data, None, None, 1_000_000))
            raise SystemExit("a nodata value of the wrong cell type was accepted")
        except ec._ffi.EcError as e:
            assert "nodata" in str(e), str(e)
print("REFUSED-PIN OK")
'''


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("refuse", [False, True])
def test_host_to_host_when_page_locking_is_refused(tmp_path, refuse):
    """Host arrays the runtime will not page-lock — with `inject_pin_refusal` every array whatever its kind; without it a read-only
    file mapping (`np.memmap(mode="r")`, which this runtime does register) — go through the host-to-host pipelines correctly, and above
    all RETURNING.  Round 3 hung here: `ec_sharded_host_expr` entered the whole arrays as ranges in use after a refused registration,
    and every shard's own pipeline (chunk_cells != 0, so it asks for a registration too) then waited for its caller's entry, forever,
    at any shard count.  One pipeline (`ec_host_expr`), a group of one shard, a group of three; plain and masked.  In a process of its
    own (a hang or an abort there fails this test and nothing else)."""
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "erased-cells_amd", "python")
    r = subprocess.run([sys.executable, "-c", _REFUSED_PIN_BODY, pkg, "1" if refuse else "0", str(tmp_path)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "REFUSED-PIN OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
