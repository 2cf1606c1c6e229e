"""What the shard group's host code must keep doing, whatever shape that code takes (csrc/ec_sharded.hip).

Three properties through the C ABI, on one GPU (device 0 listed several times under EC_GROUP_HOST_COMBINE, and a 1-rank
RCCL clique): which per-shard pointer columns are refused on the calling thread, that the three phased reductions give
the oracle's answers in every group form, and that each of them returns a failure a fire-and-forget call left behind.
The raster is the 41 x 257 u16 one of test_gpu_sharded_group.py: over 3 shards every row-block ends off a 16-byte boundary.
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import eco

ROWS, COLS = 41, 257
S, R = (lambda k: k), (lambda k: 4 + k)  # operand codes of an expression step: stream k, register k
NDVI = [(eco.SUB, S(0), S(1), 0), (eco.ADD, S(0), S(1), 1), (eco.DIV, R(0), R(1), 0)]  # (a - b) / (a + b)


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


@pytest.fixture(scope="module")
def raster():
    """The cells, the masks and the oracle's evaluation of the program: computed once, never written to."""
    from vectors import rand_cells, rand_mask
    n = ROWS * COLS
    a = rand_cells(eco.U16, n, 31)             # with the type's extremes, zeros included
    b = rand_cells(eco.U16, n, 32, specials=False)
    b[b == 0] = 1                              # a + b > 0 everywhere: no 0 / 0 cell, so no NaN whose order would need a rule
    ma, mb = rand_mask(n, 33), rand_mask(n, 34)
    ma[(a == a.min()) | (a == a.max())] = 0    # the extremes are masked out: a reduction that ignored the mask gives another answer
    ndvi = eco.f_binop(eco.DIV, eco.f_binop(eco.SUB, a, b), eco.f_binop(eco.ADD, a, b))
    for arr in (a, b, ma, mb, ndvi):
        arr.setflags(write=False)
    return dict(a=a, b=b, ma=ma, mb=mb, ndvi=ndvi)


class _Group:
    """A shard group with the raster's four columns (a, b: u16; ma, mb: byte masks) resident as row-blocks."""

    def __init__(self, ec, raster, G, flags):
        from erased_cells_hip import sharded
        self.ec, self.L, self.chk, self.G = ec, ec.lib(), ec._ffi.check, G
        self.h = C.c_void_p()
        self.chk(self.L.ec_shard_group_create((C.c_int32 * G)(*([0] * G)), G, flags, C.byref(self.h)))
        self.rng = [sharded.shard_range(ROWS, COLS, g, G) for g in range(G)]
        self.lens = [r[1] for r in self.rng]
        self.cols, self._alive = {}, []  # _alive: the columns behind the pointer tables handed to calls
        for name, item in (("a", 2), ("b", 2), ("ma", 1), ("mb", 1), ("out", 8), ("om", 1)):
            p = (C.c_void_p * G)()
            self.chk(self.L.ec_sharded_alloc(self.h, self.sizes(item), p))
            if name in raster:
                self.chk(self.L.ec_sharded_upload(self.h, p, raster[name].ctypes.data_as(C.c_void_p), self.offs(item), self.sizes(item)))
            self.cols[name] = p

    def sizes(self, item):
        return (C.c_size_t * self.G)(*[ln * item for ln in self.lens])

    def offs(self, item):
        return (C.c_size_t * self.G)(*[r[0] * item for r in self.rng])

    def n(self, lens=None):
        return (C.c_size_t * self.G)(*(self.lens if lens is None else lens))

    def col(self, name, hole=None):
        """A copy of column `name`, with a null pointer at shard `hole`."""
        p = (C.c_void_p * self.G)(*self.cols[name])
        if hole is not None:
            p[hole] = None
        return p

    def stat(self, key):
        v = C.c_int64(-1)
        self.chk(self.L.ec_shard_group_stat(self.h, key, C.byref(v)))
        return v.value

    def close(self):
        for p in self.cols.values():
            self.chk(self.L.ec_sharded_free(self.h, p))
        self.chk(self.L.ec_shard_group_destroy(self.h))

    # the three reductions; `hole`: that shard has no cells and no pointers
    def min_max(self, name, mask=None, hole=None):
        E = self.ec._ffi
        mn, mx = E.EcValue(), E.EcValue()
        st = self.L.ec_sharded_min_max(self.h, eco.U16, self.col(name, hole), self.col(mask, hole) if mask else None, self._n(hole),
                                       C.byref(mn), C.byref(mx))
        return st, (self.ec.CellValue.from_ec(mn).bits(), self.ec.CellValue.from_ec(mx).bits())

    def counts(self, mask, hole=None):
        t, f = C.c_uint64(), C.c_uint64()
        st = self.L.ec_sharded_counts(self.h, self.col(mask, hole), self._n(hole), C.byref(t), C.byref(f))
        return st, (t.value, f.value)

    def ndvi_min_max(self, masked=False, hole=None):
        E = self.ec._ffi
        mn, mx = E.EcValue(), E.EcValue()
        st = self.L.ec_sharded_expr_min_max(self.h, (C.c_uint8 * 2)(eco.U16, eco.U16), self.streams(("a", "b"), hole),
                                            self.streams(("ma", "mb"), hole) if masked else None, 2, None, 0, self.steps(), len(NDVI), self._n(hole),
                                            C.byref(mn), C.byref(mx))
        return st, (self.ec.CellValue.from_ec(mn).bits(), self.ec.CellValue.from_ec(mx).bits())

    def _n(self, hole):
        return self.n([0 if g == hole else ln for g, ln in enumerate(self.lens)])

    def steps(self):
        E = self.ec._ffi
        return (E.EcExprStep * len(NDVI))(*[E.EcExprStep(*q) for q in NDVI])

    def streams(self, names, hole=None, hole_in=None):
        """The pointer-array table of an expr / fused call; the null pointer goes to every column, or to column `hole_in` alone."""
        PVP = self.ec._ffi.PVP
        cols = [self.col(nm, hole if hole_in in (None, k) else None) for k, nm in enumerate(names)]
        self._alive.append(cols)
        return (PVP * len(names))(*[C.cast(p, PVP) for p in cols])


def _kept(raster, name, g, hole):
    """Column `name` without the cells of shard `hole`."""
    if hole is None:
        return raster[name]
    off, ln = g.rng[hole]
    return np.concatenate([raster[name][:off], raster[name][off + ln:]])


def _bits(pair):
    return pair[0].bits(), pair[1].bits()


@pytest.mark.gpu
def test_null_shard_pointer_is_refused_on_the_calling_thread_for_every_checked_column(ec, raster):
    """Every per-shard pointer column that the library checks, at every sharded entry point: a null at shard 1 with n[1] > 0 is
    refused with EC_ERR_ARG and a message that names the entry `[1] is null`, before anything is posted (`jobs_posted` stands
    still) and without harm to the group.  The columns the library copies unchecked — the mask columns and `out_mask` of
    ec_sharded_fused — are not in the table."""
    g = _Group(ec, raster, 3, 1)
    L, E = g.L, ec._ffi
    try:
        U16 = eco.U16
        dt2, dt4 = (C.c_uint8 * 2)(U16, U16), (C.c_uint8 * 4)(U16, U16, U16, U16)
        mn, mx, t, f = E.EcValue(), E.EcValue(), C.c_uint64(), C.c_uint64()

        def c(name, want, col):  # column `name`, holed if it is the one under test
            return g.col(name, 1 if want == col else None)

        def tab(names, want, label):  # the table of columns `label`, of which column want[1] is holed if want is (label, k)
            k = want[1] if isinstance(want, tuple) and want[0] == label else None
            return g.streams(names, None if k is None else 1, k)

        P, M = (lambda k: ("p", k)), (lambda k: ("masks", k))
        calls = {
            "binop": (("l", "r", "out"), lambda w: L.ec_sharded_binop(
                g.h, eco.ADD, U16, c("a", w, "l"), U16, c("b", w, "r"), g.n(), c("out", w, "out"))),
            "masked_binop": (("l", "lmask", "r", "rmask", "out", "out_mask"), lambda w: L.ec_sharded_masked_binop(
                g.h, eco.ADD, U16, c("a", w, "l"), c("ma", w, "lmask"), U16, c("b", w, "r"), c("mb", w, "rmask"), g.n(),
                c("out", w, "out"), c("om", w, "out_mask"))),
            "convert": (("src", "dst"), lambda w: L.ec_sharded_convert(g.h, U16, c("a", w, "src"), eco.F64, c("out", w, "dst"), g.n())),
            "mask_from_nodata": (("p", "mask"), lambda w: L.ec_sharded_mask_from_nodata(
                g.h, U16, c("a", w, "p"), g.n(), None, c("om", w, "mask"))),
            # (p0 - p1) / (p2 + p3): four operand columns, unmasked
            "fused": ((P(0), P(1), P(2), P(3), "out"), lambda w: L.ec_sharded_fused(
                g.h, eco.SUB, eco.DIV, eco.ADD, dt4, tab(("a", "b", "a", "b"), w, "p"), None, None, g.n(), c("out", w, "out"), None)),
            "expr": ((P(0), P(1), M(0), M(1), "out", "out_mask"), lambda w: L.ec_sharded_expr(
                g.h, dt2, tab(("a", "b"), w, "p"), tab(("ma", "mb"), w, "masks"), 2, None, 0, g.steps(), len(NDVI), g.n(),
                c("out", w, "out"), c("om", w, "out_mask"))),
            "min_max": (("p", "masks"), lambda w: L.ec_sharded_min_max(
                g.h, U16, c("a", w, "p"), c("ma", w, "masks"), g.n(), C.byref(mn), C.byref(mx))),
            "expr_min_max": ((P(0), P(1), M(0), M(1)), lambda w: L.ec_sharded_expr_min_max(
                g.h, dt2, tab(("a", "b"), w, "p"), tab(("ma", "mb"), w, "masks"), 2, None, 0, g.steps(), len(NDVI), g.n(),
                C.byref(mn), C.byref(mx))),
            "counts": (("masks",), lambda w: L.ec_sharded_counts(g.h, c("ma", w, "masks"), g.n(), C.byref(t), C.byref(f))),
        }
        g.chk(L.ec_shard_group_sync(g.h))
        posted = g.stat(b"jobs_posted")
        for entry, (columns, call) in calls.items():
            for col in columns:
                st = call(col)
                msg = L.ec_last_error_string()
                assert st == E.EC_ERR_ARG and b"[1] is null" in msg and b"ec_sharded_" + entry.encode() + b":" in msg, (entry, col, st, msg)
        assert g.stat(b"jobs_posted") == posted
        st, got = g.min_max("a")
        assert st == E.EC_OK and got == _bits(eco.f_min_max(raster["a"]))
        assert g.stat(b"poisoned") == 0
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("G,flags,hole", [(1, 0, None), (1, 1, None), (3, 1, None), (3, 1, 1)],
                         ids=["one-shard-rccl", "one-shard-host", "three-shards-host", "three-shards-middle-empty"])
def test_each_phased_reduction_matches_the_oracle_in_every_group_form(ec, raster, G, flags, hole):
    """ec_sharded_min_max (plain and masked), ec_sharded_counts and ec_sharded_expr_min_max of (a - b) / (a + b) (plain and masked):
    a 1-rank RCCL clique, one host-combined shard, three host-combined shards, and three with the middle one empty (n = 0 and
    null pointers: it contributes the idempotent payload).  Bit for bit the oracle's f_min_max of the cells, numpy's count of the
    mask, and f_min_max of the oracle's evaluation of the program."""
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    E = ec._ffi
    g = _Group(ec, raster, G, flags)
    try:
        a, ma, ndvi = (_kept(raster, k, g, hole) for k in ("a", "ma", "ndvi"))
        both = _kept(raster, "ma", g, hole) & _kept(raster, "mb", g, hole)
        assert g.min_max("a", hole=hole) == (E.EC_OK, _bits(eco.f_min_max(a)))
        assert g.min_max("a", "ma", hole=hole) == (E.EC_OK, _bits(eco.f_min_max(a, ma)))
        assert g.counts("ma", hole=hole) == (E.EC_OK, (int(np.count_nonzero(ma)), int(ma.size - np.count_nonzero(ma))))
        assert g.ndvi_min_max(hole=hole) == (E.EC_OK, _bits(eco.f_min_max(ndvi)))
        assert g.ndvi_min_max(masked=True, hole=hole) == (E.EC_OK, _bits(eco.f_min_max(ndvi, both)))
        assert g.stat(b"poisoned") == 0
    finally:
        g.close()


@pytest.mark.gpu
def test_each_phased_reduction_returns_a_deferred_failure_once(ec, raster):
    """A fire-and-forget call whose job fails on shard 1 after the call returned: the NEXT reduction — each of the three in turn —
    returns that failure (its input may be the failed call's output), the one after it succeeds, and the group is not poisoned."""
    E = ec._ffi
    g = _Group(ec, raster, 3, 1)
    L = g.L
    reductions = {
        "min_max": (lambda: g.min_max("a"), _bits(eco.f_min_max(raster["a"]))),
        "counts": (lambda: g.counts("ma"), (int(np.count_nonzero(raster["ma"])), int(raster["ma"].size - np.count_nonzero(raster["ma"])))),
        "expr_min_max": (lambda: g.ndvi_min_max(), _bits(eco.f_min_max(raster["ndvi"]))),
    }
    try:
        for name, (reduce, expected) in reductions.items():
            g.chk(L.ec_tune_set(b"inject_shard_failure", 2))  # shard 1's next posted job
            g.chk(L.ec_sharded_binop(g.h, eco.ADD, eco.U16, g.col("a"), eco.U16, g.col("b"), g.n(), g.col("out")))  # EC_OK: only queued
            st, _ = reduce()
            msg = L.ec_last_error_string()
            assert st == E.EC_ERR_HIP and b"shard" in msg and b"injected" in msg, (name, st, msg)
            assert reduce() == (E.EC_OK, expected), name
            assert g.stat(b"poisoned") == 0
    finally:
        g.chk(L.ec_tune_set(b"inject_shard_failure", 0))
        g.close()
