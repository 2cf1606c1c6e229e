"""Every entry point from concurrent host threads — on streams of their own and on one shared stream — through the C ABI with an
explicit stream argument, never through the Python mirror (whose stream is a module global).  INTEGRATION.md, "Thread safety":
the library is re-entrant for concurrent calls on distinct streams, and host threads that share one stream may call concurrently.

The jobs, their inputs and the bytes they must leave are tests/concurrent_cases.py's (the families' own references and the oracle);
tests/test_concurrent_cases.py shows on the CPU that no two workers share an answer and that a reduction whose finalize step
folds another call's partials, or too few of its own, is wrong for certain.

How every test here runs.  The main thread uploads every input and cuts every output and workspace out of one device block,
then synchronises; it also sets the knobs, before the workers start, and puts them back afterwards.  A worker only launches,
downloads on its own stream argument and compares.  Every output is filled with the worker's own byte pattern before every call,
by a copy queued on the call's stream.  Workers leave a threading.Barrier together, so their calls overlap on the host (ctypes
releases the GIL for the length of a call).  Loop counts are numbers, not seconds.  A worker's exception fails the test; a
worker that does not come back ends the session: nothing more is launched behind a call that hangs."""
import collections
import ctypes as C
import threading
import traceback

import pytest

import concurrent_cases as K

pytestmark = pytest.mark.gpu

JOIN_SECONDS = 120          # far beyond any test here (a few seconds): a worker still running then is taken for hung
FAMILY_ROUNDS = 20          # passes over the whole table per worker
REDUCTION_ROUNDS = 500      # rounds of the four asynchronous reductions per worker
TURNOVER_STREAMS = 70       # more than the scratch table's 64 entries per device


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


class Slot:
    """What worker k needs for one job: `inp`, `ptr` and `fill` are what Job.call reads."""

    def __init__(self, job, k):
        self.job, self.k, self.inp, self.want, self.fill = job, k, job.inputs(k), job.expected(k), K.fill_byte(k)
        self.ptr, self.outs, self.pattern = {}, [], None


class Table:
    """Every job for every worker, resident: one ec_alloc block cut at 256-byte boundaries, filled on the main thread."""

    def __init__(self, ec):
        self.L, self.check = ec.lib(), ec._ffi.check
        L, check = self.L, self.check
        self.slots, pieces, total = {}, [], 0

        def take(nbytes):
            nonlocal total
            at = total
            total += -(-max(nbytes, 1) // 256) * 256
            return at

        for job in K.JOBS:
            for k in range(K.WORKERS):
                s = self.slots[job.name, k] = Slot(job, k)
                uploads = {name: v.tobytes() for name, v in s.inp.items() if hasattr(v, "tobytes")}
                if job.prepare:
                    uploads.update(job.prepare(L, s.inp))
                for name, raw in uploads.items():
                    pieces.append((s, name, take(len(raw)), raw))
                for name, w in s.want.items():
                    if name not in job.host:
                        pieces.append((s, name, take(len(w)), None))
                        s.outs.append((name, len(w)))
                for name, nbytes in (job.scratch(L, s.inp) if job.scratch else {}).items():
                    assert nbytes > 0, (job.name, k, name)
                    pieces.append((s, name, take(nbytes), None))
        longest = [max([n for (j, w), s in self.slots.items() if w == k for _, n in s.outs], default=1) for k in range(K.WORKERS)]
        patterns = [take(n) for n in longest]
        self.block, self.stream = C.c_void_p(), C.c_void_p()
        check(L.ec_alloc(C.byref(self.block), total))
        check(L.ec_stream_create(C.byref(self.stream)))
        for s, name, at, raw in pieces:
            s.ptr[name] = self.block.value + at
            if raw:
                check(L.ec_upload(s.ptr[name], raw, len(raw), self.stream))
        for k in range(K.WORKERS):
            raw = bytes([K.fill_byte(k)]) * longest[k]
            check(L.ec_upload(self.block.value + patterns[k], raw, len(raw), self.stream))
        for (_, k), s in self.slots.items():
            s.pattern = self.block.value + patterns[k]
        check(L.ec_stream_sync(self.stream))

    def close(self):
        self.check(self.L.ec_stream_sync(self.stream))
        self.check(self.L.ec_stream_destroy(self.stream))
        self.check(self.L.ec_free(self.block))

    def run(self, name, k, stream):
        """One call of job `name` with worker k's buffers on `stream`: the pre-fill, the call, the downloads -> the checker's
        complaints."""
        L, s = self.L, self.slots[name, k]
        for out, nbytes in s.outs:
            self.check(L.ec_copy(s.ptr[out], s.pattern, nbytes, stream))
        got = s.job.call(L, s, stream) or {}
        for out, nbytes in s.outs:
            buf = C.create_string_buffer(nbytes)
            self.check(L.ec_download(buf, s.ptr[out], nbytes, stream))
            got[out] = buf.raw
        return K.check(s.want, got, s.fill)


@pytest.fixture(scope="module")
def table(ec):
    t = Table(ec)
    yield t
    t.close()


class Streams:
    """n streams of ec_stream_create, and more on demand; all released and destroyed on the way out"""

    def __init__(self, ec, n):
        self.L, self.check, self.streams = ec.lib(), ec._ffi.check, []
        for _ in range(n):
            self.add()

    def add(self):
        s = C.c_void_p()
        self.check(self.L.ec_stream_create(C.byref(s)))
        self.streams.append(s)
        return s

    def __enter__(self):
        return self.streams

    def __exit__(self, *exc):
        for s in self.streams:
            self.check(self.L.ec_stream_sync(s))
            self.check(self.L.ec_release_stream(s))
            self.check(self.L.ec_stream_destroy(s))
        return False


def drive(n_workers, body):
    """body(i, barrier, calls, bad) on n_workers threads -> (calls made per entry point, complaints).  A worker that raises breaks
    the barrier, so the others stop at their next round; one that does not return within JOIN_SECONDS ends the session."""
    barrier = threading.Barrier(n_workers)
    calls, bad, errors = [collections.Counter() for _ in range(n_workers)], [[] for _ in range(n_workers)], []

    def target(i):
        try:
            body(i, barrier, calls[i], bad[i])
        except threading.BrokenBarrierError:
            pass
        except BaseException:  # noqa: BLE001 — reported below
            errors.append((i, traceback.format_exc()))
            barrier.abort()

    threads = [threading.Thread(target=target, args=(i,), daemon=True) for i in range(n_workers)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_SECONDS)
    hung = [i for i, t in enumerate(threads) if t.is_alive()]
    if hung:
        pytest.exit(f"workers {hung} did not return within {JOIN_SECONDS} s: taken for hung, nothing more is launched", returncode=1)
    assert not errors, "\n".join(f"worker {i}:\n{tb}" for i, tb in errors)
    return sum(calls, collections.Counter()), sum(bad, [])


def verdict(calls, bad):
    """All calls right — or how many of which entry point were not, and the first complaints."""
    per_job = collections.Counter(name for name, *_ in bad)
    summary = ", ".join(f"{name}: {n} of {calls[name]}" for name, n in sorted(per_job.items()))
    assert not bad, f"{len(bad)} of {sum(calls.values())} calls left wrong bytes ({summary}); the first: {bad[:5]}"


def family_body(table, streams):
    names = [j.name for j in K.JOBS]

    def body(i, barrier, calls, bad):
        first = i * (len(names) // 6)
        for r in range(FAMILY_ROUNDS):
            barrier.wait(JOIN_SECONDS)
            for step in range(len(names)):
                name = names[(first + step) % len(names)]
                report = table.run(name, i, streams[i])
                calls[name] += 1
                if report:
                    bad.append((name, "worker", i, "round", r, report))
    return body


def test_families_on_own_streams(ec, table):
    """Six workers, a stream each, the whole table FAMILY_ROUNDS times, worker k starting a sixth of the table further on: different
    families overlap in time, and the library-workspace forms take and return pool blocks on six streams at once."""
    with ec.tuned(expr_jit=0), Streams(ec, 6) as streams:
        calls, bad = drive(6, family_body(table, streams))
    assert sum(calls.values()) == 6 * FAMILY_ROUNDS * len(K.JOBS)
    verdict(calls, bad)


def test_families_sharing_one_stream(ec, table):
    """The same with all six workers on ONE created stream: the stream orders their launches, the library everything else."""
    with ec.tuned(expr_jit=0), Streams(ec, 1) as streams:
        calls, bad = drive(6, family_body(table, streams * 6))
    assert sum(calls.values()) == 6 * FAMILY_ROUNDS * len(K.JOBS)
    verdict(calls, bad)


ASYNC_REDUCTIONS = ("ec_stats_device", "ec_min_max_keys", "ec_mask_counts_device", "ec_expr_min_max_keys")
SYNC_FORMS = ("ec_stats_compute", "ec_min_max", "ec_mask_counts", "ec_first_difference", "ec_zonal_stats_compute")


@pytest.mark.parametrize("counts_one_launch", [0, 2], ids=["two-launch counts", "one-launch counts"])
def test_async_reductions_sharing_one_stream(ec, table, counts_one_launch):
    """Four workers on one stream, each calling the four asynchronous reductions on its own cells into its own device slots —
    grids of 2, 3, 4 and 5 workgroups, all leaving the barrier together at every call; in even rounds all four call the same entry
    point, in odd rounds four different ones (min/max, the counts and first difference share one partials slot).  A fifth worker
    puts the synchronous forms between them.  A partials kernel and its finalize step are two launches: if another thread's
    partials could land between them, the finalize step would fold those, with its own workgroup count."""
    def body(i, barrier, calls, bad):
        for r in range(REDUCTION_ROUNDS):
            for step in range(len(ASYNC_REDUCTIONS)):
                if i < 4:
                    name = ASYNC_REDUCTIONS[(step + (i if r % 2 else 0)) % len(ASYNC_REDUCTIONS)]
                else:
                    name = SYNC_FORMS[(r * len(ASYNC_REDUCTIONS) + step) % len(SYNC_FORMS)]
                barrier.wait(JOIN_SECONDS)
                report = table.run(name, i, streams[0])
                calls[name] += 1
                if report:
                    bad.append((name, "worker", i, "round", r, report))

    with ec.tuned(expr_jit=0, counts_one_launch=counts_one_launch), Streams(ec, 1) as streams:
        calls, bad = drive(5, body)
    assert sum(calls.values()) == 5 * REDUCTION_ROUNDS * len(ASYNC_REDUCTIONS)
    verdict(calls, bad)


def test_scratch_table_turnover(ec, table):
    """One thread, TURNOVER_STREAMS streams one after the other — more than the table of per-stream scratch holds.  Each runs the
    one-launch counts (the accumulator word), the band statistics and min/max, is checked and drained before the next stream is
    first used, so no entry is recycled with work in flight.  Then the first six streams again, whose entries have been recycled:
    fresh scratch, the right answers twice in a row, the accumulator back at zero in between."""
    L = ec.lib()
    calls, bad = collections.Counter(), []

    def visit(s, k, what):
        for name in ("ec_mask_counts_device", "ec_stats_device", "ec_min_max_keys"):
            report = table.run(name, k, s)
            calls[name] += 1
            if report:
                bad.append((name, what, report))
        ec._ffi.check(L.ec_stream_sync(s))

    held = C.c_int64()
    made = Streams(ec, 0)
    with ec.tuned(counts_one_launch=2), made as streams:
        for n in range(TURNOVER_STREAMS):
            visit(made.add(), n % K.WORKERS, ("stream", n))      # the stream comes into being only now
        ec._ffi.check(L.ec_stat_get(b"scratch_streams", C.byref(held)))
        assert 0 < held.value <= 64, held.value
        for again in range(2):
            for n, s in enumerate(streams[:6]):
                visit(s, (n + 3) % K.WORKERS, ("stream", n, "again", again))
    verdict(calls, bad)
