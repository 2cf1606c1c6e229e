"""Element-wise kernels write all of their output and nothing else — wherever the output sits — and leave their operands alone.

The parity files compare results bit for bit over all types, many lengths and many INPUT window offsets, but every output there
is a fresh block of the library's pool of which only [0, n) is read back: a store past `n`, a cell that is never written (the
pool recycles blocks that may already hold the right answer), an output at 8 mod 16 and a written operand would all pass.  Here
every call writes into an `Arena` (tests/arena.py): random guards on both sides, the payload pre-filled with the complement of
the oracle's result, at a chosen offset from a 256-byte boundary; every operand sits in a guarded arena of its own that is
compared byte for byte after each sweep.  tests/test_arena_faults.py shows (without a GPU) that the arenas notice the faults
this file is for.

Inputs are `rand_cells(..., specials=False)` with zeros salted in (x / 0 and 0 / 0): no operand holds a NaN, every NaN a kernel
makes is the default one, so every comparison is bit-exact with no NaN-by-class exception.  This file is about placement.

Sizes come from the kernels' constants: the base list around the 16-cell groups, and T - 1 .. 3 T + 7 for each family's tile T
(1024 cells for the pair grids of the binop, fused, ahead-of-time and compiled expression kernels, 1536 for the interpreter,
256 x map_u x CPL for the map kernels), each also one cell longer so that a peeled head puts n - head on both sides of every
boundary.  f64 outputs sit at cell offsets 0 and 1 (0 and 8 mod 16), byte outputs at byte offsets 0, 1, 3, 8, 15, typed outputs
at cells 0, 1, 16 / W - 1; operands at cell offsets 0 and 1 (with a 1-byte operand that is `peel_head` = 0 and 1; `peel` = 2
peels for 2-byte operands).  One type pair per pair of byte widths: the instantiations are covered elsewhere.
"""
import ctypes as C

import numpy as np
import pytest

import stats_ref as R
from arena import Arena, operand, output
from oracle import eco
from vectors import rand_cells, rand_mask

pytestmark = pytest.mark.gpu

BASE = [0, 1, 2, 3, 4, 15, 16, 17, 31, 33, 255, 256, 257]
NMAX = 70016   # cells per operand: the largest size below is 70001 (one past the 65536-cell tile of the byte reductions)
S, RG, K = (lambda k: k), (lambda k: 4 + k), (lambda k: 8 + k)   # operand references of a program step
F64_OFFS = (0, 1)
BYTE_OFFS = (0, 1, 3, 8, 15)
IN_OFFS = (0, 1)
# one pair per (width_l, width_r): signed, unsigned and float mixed
WIDTH_PAIRS = {(1, 1): (eco.U8, eco.I8), (1, 2): (eco.U8, eco.U16), (1, 4): (eco.I8, eco.F32), (1, 8): (eco.U8, eco.F64),
               (2, 1): (eco.I16, eco.U8), (2, 2): (eco.U16, eco.I16), (2, 4): (eco.U16, eco.F32), (2, 8): (eco.I16, eco.I64),
               (4, 1): (eco.F32, eco.I8), (4, 2): (eco.I32, eco.U16), (4, 4): (eco.F32, eco.U32), (4, 8): (eco.U32, eco.F64),
               (8, 1): (eco.F64, eco.U8), (8, 2): (eco.U64, eco.I16), (8, 4): (eco.I64, eco.F32), (8, 8): (eco.F64, eco.I64)}
OPS = (eco.DIV, eco.SUB, eco.MUL, eco.ADD)


def sizes(T):
    """The base list, the sizes around the boundaries of a tile of T cells, and each of those one cell longer (a peeled head)."""
    around = [T - 1, T, T + 1, T + 2, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 7]
    return sorted(set(BASE + around + [x + 1 for x in around]))


def typed_offs(width):
    return sorted({0, 1, 16 // width - 1})


def size_of(ct):
    return np.dtype(eco.NP_DTYPES[ct]).itemsize


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


class Pool:
    """The operands: per (cell type, cell offset, slot) one guarded arena of NMAX cells, uploaded once.  A sweep uses prefixes."""

    def __init__(self, ec):
        self.ec, self.cells, self.masks, self.arenas = ec, {}, {}, {}

    def host(self, ct, slot=0):
        key = (ct, slot)
        if key not in self.cells:
            a = rand_cells(ct, NMAX, 7700 + 16 * slot, specials=False)
            a[11::211] = 0                    # shared by every operand: 0 / 0
            a[(3 + slot) % 7::53] = 0         # x / 0
            self.cells[key] = a
        return self.cells[key]

    def host_mask(self, slot=0):
        if slot not in self.masks:
            self.masks[slot] = rand_mask(NMAX, 7800 + slot)
        return self.masks[slot]

    def get(self, ct, off=0, slot=0):
        """(pointer to the first cell, host cells) of operand `slot` of type `ct`, `off` cells behind a 256-byte boundary."""
        key = ("c", ct, off, slot)
        if key not in self.arenas:
            self.arenas[key] = operand(self.ec, self.host(ct, slot), off, seed=len(self.arenas) + 1)
        return self.arenas[key].ptr, self.host(ct, slot)

    def mask(self, off=0, slot=0):
        key = ("m", off, slot)
        if key not in self.arenas:
            self.arenas[key] = operand(self.ec, self.host_mask(slot), off, seed=len(self.arenas) + 1)
        return self.arenas[key].ptr, self.host_mask(slot)

    def recheck(self):
        """Operands are not written: every arena, guards included, byte for byte as uploaded."""
        for key, a in self.arenas.items():
            a.check_unchanged(f"operand {key}")


@pytest.fixture(scope="module")
def pool(ec):
    return Pool(ec)


@pytest.fixture(scope="module")
def memo():
    """The oracle's full-length answers, shared between the arms of a family: they do not depend on a knob."""
    return {}


@pytest.fixture(autouse=True)
def operands_stay_as_they_were(pool):
    yield
    pool.recheck()


def _stat(ec, key):
    v = C.c_int64(0)
    assert ec.lib().ec_stat_get(key, C.byref(v)) == 0, key
    return v.value


def _value(ec, ct, x):
    return ec.CellValue(ct, x).to_ec()


def _oracle_steps(streams, scalars, steps):
    """A program evaluated step by step on the oracle's typed loops (a scalar widened to f64 once, as the library does)."""
    n = min(len(s_) for s_ in streams)
    val = {k: s_[:n] for k, s_ in enumerate(streams)}
    for k, c in enumerate(scalars):
        val[8 + k] = np.full(n, float(c))
    last = None
    for op, a, b, dst in steps:
        val[4 + dst] = eco.f_binop(op, val[a], val[b])
        last = 4 + dst
    return val[last]


def _seed(*parts):
    return hash(parts) & 0xFFFF


# ================================================================ ec_binop
@pytest.mark.parametrize("variant,uv,peel", [(0, 1, 1), (1, 1, 1), (0, 0, 1), (1, 0, 1), (0, 1, 2), (0, 1, 0)],
                         ids=["direct", "lds", "direct-cellwise-when-unaligned", "lds-cellwise-when-unaligned", "direct-peel-2-byte", "direct-no-peel"])
def test_binop(ec, pool, memo, variant, uv, peel):
    """Direct and LDS-staged kernels; with unaligned_vector = 0 every call with an odd operand offset or an output at 8 mod 16
    takes the cell-wise kernel — same cells, same guards.  peel = 2 / 0: the pairs with a 2-byte / 1-byte operand only."""
    L, chk = ec.lib(), ec._ffi.check
    pairs = WIDTH_PAIRS
    if peel == 2:
        pairs = {w: p for w, p in WIDTH_PAIRS.items() if 2 in w}
    if peel == 0:
        pairs = {w: p for w, p in WIDTH_PAIRS.items() if 1 in w}
    with ec.tuned(binop_variant=variant, unaligned_vector=uv, peel=peel):
        for k, (lt, rt) in enumerate(pairs.values()):
            op = OPS[k % 4]
            for io in IN_OFFS:
                (pl, hl), (pr, hr) = pool.get(lt, io), pool.get(rt, io)
                if ("binop", lt, rt, op) not in memo:
                    memo["binop", lt, rt, op] = eco.f_binop(op, hl, hr)
                full = memo["binop", lt, rt, op]
                for oo in F64_OFFS:
                    for n in sizes(1024):
                        out = output(ec, full[:n], oo, _seed(lt, rt, n, oo))
                        chk(L.ec_binop(op, lt, pl, rt, pr, n, out.ptr, ec.stream()))
                        out.check(full[:n], f"ec_binop {eco.CT_NAMES[lt]} {op} {eco.CT_NAMES[rt]} n {n} in +{io} out +{oo} cells")


# ================================================================ ec_binop_scalar
@pytest.mark.parametrize("uv", [1, 0], ids=["vector", "cellwise-when-unaligned"])
def test_binop_scalar(ec, pool, uv):
    """Integer cells with a finite scalar (the form without the NaN rule), with a zero divisor and an infinite scalar (the form
    with it), and float cells."""
    L, chk = ec.lib(), ec._ffi.check
    cases = [(eco.U8, eco.MUL, 2.5), (eco.I16, eco.DIV, 4.0), (eco.U32, eco.SUB, 0.1), (eco.I64, eco.ADD, 3.0),     # no NaN possible
             (eco.U8, eco.DIV, 0.0), (eco.I16, eco.MUL, float("inf")), (eco.U64, eco.DIV, 0.0),                      # the NaN rule
             (eco.F32, eco.MUL, 2.5), (eco.F64, eco.DIV, 0.0)]                                                         # float cells
    with ec.tuned(unaligned_vector=uv):
        for ct, op, s in cases:
            sv, so = _value(ec, eco.F64, s), eco.Value.of(eco.F64, s)
            for io in IN_OFFS:
                p, h = pool.get(ct, io)
                full = eco.f_binop_scalar(op, h, so)
                for oo in F64_OFFS:
                    for n in sizes(1024):
                        out = output(ec, full[:n], oo, _seed(ct, n, oo))
                        chk(L.ec_binop_scalar(op, ct, p, n, C.byref(sv), out.ptr, ec.stream()))
                        out.check(full[:n], f"ec_binop_scalar {eco.CT_NAMES[ct]} {op} {s} n {n} in +{io} out +{oo}")


# ================================================================ ec_masked_binop
MASKED_PAIRS = [(1, 1), (1, 2), (2, 4), (4, 8), (8, 2), (8, 8)]   # six of the sixteen width pairs: the sizes and offsets are kept whole


@pytest.mark.parametrize("variant,uv", [(0, 1), (1, 1), (0, 0), (1, 0)],
                         ids=["direct", "lds", "direct-cellwise-when-unaligned", "lds-cellwise-when-unaligned"])
def test_masked_binop(ec, pool, memo, variant, uv):
    """`out` and `out_mask` each in an arena of its own, each offset on its own; the operand masks share the operands' offset."""
    L, chk = ec.lib(), ec._ffi.check
    with ec.tuned(binop_variant=variant, unaligned_vector=uv):
        for k, w in enumerate(MASKED_PAIRS):
            lt, rt = WIDTH_PAIRS[w]
            op = OPS[k % 4]
            for io in IN_OFFS:
                (pl, hl), (pr, hr) = pool.get(lt, io), pool.get(rt, io)
                (plm, hlm), (prm, hrm) = pool.mask(io, 0), pool.mask(io, 1)
                if ("binop", lt, rt, op) not in memo:
                    memo["binop", lt, rt, op] = eco.f_binop(op, hl, hr)
                full, fmask = memo["binop", lt, rt, op], eco.mask_and(hlm, hrm)
                for oo in F64_OFFS:
                    for mo in BYTE_OFFS:
                        for n in sizes(1024):
                            what = f"ec_masked_binop {eco.CT_NAMES[lt]} {op} {eco.CT_NAMES[rt]} n {n} in +{io} out +{oo} cells, mask +{mo} bytes"
                            out, om = output(ec, full[:n], oo, _seed(n, oo, mo)), output(ec, fmask[:n], mo, _seed(n, mo, oo, 1))
                            chk(L.ec_masked_binop(op, lt, pl, plm, rt, pr, prm, n, out.ptr, om.ptr, ec.stream()))
                            out.check(full[:n], what + ": values")
                            om.check(fmask[:n], what + ": mask")


# ================================================================ ec_fused / ec_masked_fused
def _fused_case(arm):
    """(cell types, scalar operand index or None, ops, distinct masks) of a chain `(x o1 y) o2 (z o3 w)` / `(x o1 y) o2 z`."""
    if arm == "single-type":
        return [eco.U16, eco.U16, eco.U16], None, (eco.SUB, eco.DIV, ec_none()), 0
    if arm == "mixed-four":
        return [eco.U8, eco.I16, eco.F32, eco.F64], None, (eco.SUB, eco.DIV, eco.ADD), 0
    if arm == "scalar":
        return [eco.I8, None, eco.F32], 1, (eco.MUL, eco.ADD, ec_none()), 0
    if arm == "masked-one-mask":
        return [eco.U16, eco.U16, eco.U16], None, (eco.ADD, eco.MUL, ec_none()), 1
    return [eco.U8, eco.I16, eco.F32, eco.F64], None, (eco.SUB, eco.DIV, eco.ADD), 3


def ec_none():
    return -1   # EC_OP_NONE


@pytest.mark.parametrize("uv", [1, 0], ids=["vector", "cellwise-when-unaligned"])
@pytest.mark.parametrize("arm", ["single-type", "mixed-four", "scalar", "masked-one-mask", "masked-three-masks"])
def test_fused(ec, pool, arm, uv):
    L, chk = ec.lib(), ec._ffi.check
    cts, sc_at, (o1, o2, o3), nmask = _fused_case(arm)
    nops = len(cts)
    scalars = (ec._ffi.EcValue * 4)()
    if sc_at is not None:
        scalars[sc_at] = _value(ec, eco.F32, 0.0001)
    with ec.tuned(unaligned_vector=uv):
        for io in IN_OFFS:
            dt, p, m = (C.c_uint8 * 4)(), (C.c_void_p * 4)(), (C.c_void_p * 4)()
            hs, hms = [], []
            for k, ct in enumerate(cts):
                if ct is None:
                    hs.append(np.full(NMAX, float(np.float32(0.0001))))
                    continue
                p[k], h = pool.get(ct, io, slot=k)
                dt[k] = ct
                hs.append(h)
                if nmask:
                    slot = 0 if nmask == 1 else min(k, 2)   # three distinct masks: the fourth operand shares the third's
                    m[k], hm = pool.mask(io, slot)
                    hms.append(hm)
            e1 = eco.f_binop(o1, hs[0], hs[1])
            e2 = eco.f_binop(o3, hs[2], hs[3]) if nops == 4 else hs[2]
            full = eco.f_binop(o2, e1, e2)
            fmask = None
            for hm in hms:
                fmask = hm.copy() if fmask is None else fmask & hm
            for oo in F64_OFFS:
                for mo in (BYTE_OFFS if nmask else (0,)):
                    for n in sizes(1024):
                        what = f"ec_fused {arm} n {n} in +{io} out +{oo} mask +{mo}"
                        out = output(ec, full[:n], oo, _seed(n, oo, mo))
                        if nmask:
                            om = output(ec, fmask[:n], mo, _seed(n, mo, oo, 2))
                            chk(L.ec_masked_fused(o1, o2, o3, dt, p, m, scalars, n, out.ptr, om.ptr, ec.stream()))
                            om.check(fmask[:n], what + ": mask")
                        else:
                            chk(L.ec_fused(o1, o2, o3, dt, p, scalars if sc_at is not None else None, n, out.ptr, ec.stream()))
                        out.check(full[:n], what + ": values")


# ================================================================ ec_expr / ec_masked_expr
NDVI = [(eco.SUB, S(0), S(1), 0), (eco.ADD, S(0), S(1), 1), (eco.DIV, RG(0), RG(1), 0)]
AFFINE = [(eco.MUL, S(0), K(0), 0), (eco.ADD, RG(0), K(1), 0)]
TREE = [(eco.MUL, S(0), K(0), 0), (eco.SUB, RG(0), S(1), 1), (eco.DIV, RG(1), S(2), 0)]   # not in the ahead-of-time catalogue
# form -> (knobs, the counter that must advance, tile in cells, [(cell types, scalars, steps, masked)])
EXPR_FORMS = {
    "interpreter": (dict(expr_jit=0, expr_fixed=0), b"expr_interp_launches", 1536,
                    [([eco.U8, eco.I16, eco.F64], [0.5], TREE, False), ([eco.U8, eco.I16, eco.F64], [0.5], TREE, True),
                     ([eco.U16, eco.I16], [], NDVI, False)]),
    "ahead-of-time": (dict(expr_jit=0, expr_fixed=1), b"expr_fixed_launches", 1024,
                      [([eco.U16, eco.I16], [], NDVI, False), ([eco.U8, eco.I8], [], NDVI, True),
                       ([eco.F32], [0.0001, -273.15], AFFINE, False), ([eco.I64], [0.0001, -273.15], AFFINE, True)]),
    # at most four (program, cell types, masked or not) combinations: each is one hiprtc compile
    "compiled": (dict(expr_jit=2, expr_fixed=0), b"expr_jit_launches", 1024,
                 [([eco.U8, eco.I16, eco.F64], [0.5], TREE, False), ([eco.U8, eco.I16, eco.F64], [0.5], TREE, True),
                  ([eco.U16, eco.I16], [], NDVI, False), ([eco.U16, eco.I16], [], NDVI, True)]),
}
COUNTERS = (b"expr_interp_launches", b"expr_fixed_launches", b"expr_jit_launches")


def _expr_args(ec, pool, cts, scalars, steps, io, masked):
    k = len(cts)
    dt, p, m = (C.c_uint8 * k)(*cts), (C.c_void_p * k)(), (C.c_void_p * k)()
    hs, fmask = [], None
    for j, ct in enumerate(cts):
        p[j], h = pool.get(ct, io, slot=j)
        hs.append(h)
        if masked:
            m[j], hm = pool.mask(io, j % 2)
            fmask = hm.copy() if fmask is None else fmask & hm
    sc = (ec._ffi.EcValue * max(1, len(scalars)))(*[_value(ec, eco.F64, x) for x in scalars])
    st = (ec._ffi.EcExprStep * len(steps))(*[ec._ffi.EcExprStep(*s_) for s_ in steps])
    return dt, p, m, sc, st, _oracle_steps(hs, scalars, steps), fmask


def _expr_sweep(ec, pool, cts, scalars, steps, masked, tile, counter, vector_only_when_aligned=False):
    L, chk = ec.lib(), ec._ffi.check
    for io in IN_OFFS:
        dt, p, m, sc, st, full, fmask = _expr_args(ec, pool, cts, scalars, steps, io, masked)
        for oo in F64_OFFS:
            for mo in (BYTE_OFFS if masked else (0,)):
                for n in sizes(tile):
                    what = f"ec_expr {[eco.CT_NAMES[c] for c in cts]} {len(steps)} steps masked {masked} n {n} in +{io} out +{oo} mask +{mo}"
                    out = output(ec, full[:n], oo, _seed(n, oo, mo))
                    before = [_stat(ec, c) for c in COUNTERS]
                    if masked:
                        om = output(ec, fmask[:n], mo, _seed(n, mo, oo, 3))
                        chk(L.ec_masked_expr(dt, p, m, len(cts), sc, len(scalars), st, len(steps), n, out.ptr, om.ptr, ec.stream()))
                        om.check(fmask[:n], what + ": mask")
                    else:
                        chk(L.ec_expr(dt, p, len(cts), sc, len(scalars), st, len(steps), n, out.ptr, ec.stream()))
                    out.check(full[:n], what + ": values")
                    # the intended form ran, and no other (n = 0 launches nothing; the knob-off arm runs the cell-wise kernel,
                    # which has no counter, wherever a pointer is not 16-byte aligned)
                    ran = n > 0 and not (vector_only_when_aligned and (io or oo or mo))
                    after = [_stat(ec, c) for c in COUNTERS]
                    assert [a - b for a, b in zip(after, before)] == [int(ran and c == counter) for c in COUNTERS], what


@pytest.mark.parametrize("form", list(EXPR_FORMS))
def test_expr(ec, pool, form):
    knobs, counter, tile, programs = EXPR_FORMS[form]
    with ec.tuned(**knobs):
        for cts, scalars, steps, masked in programs:
            _expr_sweep(ec, pool, cts, scalars, steps, masked, tile, counter)


def test_expr_cellwise_when_unaligned(ec, pool):
    """unaligned_vector = 0: the interpreter's vector kernel only where every pointer is 16-byte aligned, else the cell-wise one."""
    with ec.tuned(expr_jit=0, expr_fixed=0, unaligned_vector=0):
        for masked in (False, True):
            _expr_sweep(ec, pool, [eco.U8, eco.I16, eco.F64], [0.5], TREE, masked, 1536, b"expr_interp_launches", vector_only_when_aligned=True)


# ================================================================ the map kernels
def _map_sweep(ec, call, full, in_offs, out_offs, T, what, seed):
    """`call(io, out_ptr, n)` for every size around a tile of T cells, input offset and output offset (in cells of the output)."""
    for io in in_offs:
        for oo in out_offs:
            for n in sizes(T):
                out = output(ec, full[:n], oo, _seed(seed, n, oo, io))
                call(io, out.ptr, n)
                out.check(full[:n], f"{what} n {n} in +{io} out +{oo}")


CONVERT_PAIRS = [(eco.U8, eco.I16), (eco.U8, eco.U32), (eco.U16, eco.F32), (eco.F32, eco.F64), (eco.I8, eco.I64),   # CPL 8, 4, 4, 2, 2
                 (eco.U16, eco.U16), (eco.F64, eco.F64)]                                                              # st == dt: the copy
MAP_FAMILIES = ["convert", "neg", "fill", "mask_from_nodata", "mask_select", "mask_logic", "synth"]


@pytest.mark.parametrize("uv", [1, 0], ids=["vector", "cellwise-when-unaligned"])
@pytest.mark.parametrize("map_u", [1, 2, 4])
@pytest.mark.parametrize("family", MAP_FAMILIES)
def test_map(ec, pool, memo, family, map_u, uv):
    """CPL = 16 / the widest cell of a kernel; its tile is 256 x map_u x CPL cells.  (A convert of CPL 16 does not exist — both sides
    one byte wide is the copy; ec_neg of i8, ec_fill and ec_mask_select of u8 and the mask operators have CPL 16.)"""
    L, chk, s = ec.lib(), ec._ffi.check, ec.stream()

    def tile(widest):
        return 256 * map_u * (16 // widest)

    def cached(key, make):
        if key not in memo:
            memo[key] = make()
        return memo[key]

    with ec.tuned(map_u=map_u, unaligned_vector=uv):
        if family == "convert":
            for st, dt in CONVERT_PAIRS:
                full = cached(("convert", st, dt), lambda: eco.f_convert(pool.host(st), dt) if st != dt else pool.host(st).copy())
                _map_sweep(ec, lambda io, o, n: chk(L.ec_convert(st, pool.get(st, io)[0], dt, o, n, s)), full, IN_OFFS,
                           typed_offs(size_of(dt)), tile(max(size_of(st), size_of(dt))), f"ec_convert {eco.CT_NAMES[st]} -> {eco.CT_NAMES[dt]}", st)
        elif family == "neg":
            for ct in (eco.I8, eco.U8, eco.U16, eco.F32, eco.I64, eco.U32):   # CPL 16, 8, 4, 4, 2, 2
                full = cached(("neg", ct), lambda: eco.f_neg(pool.host(ct)))
                _map_sweep(ec, lambda io, o, n: chk(L.ec_neg(ct, pool.get(ct, io)[0], n, o, s)), full, IN_OFFS,
                           typed_offs(full.dtype.itemsize), tile(max(size_of(ct), full.dtype.itemsize)), f"ec_neg {eco.CT_NAMES[ct]}", ct)
        elif family == "fill":
            for ct, x in ((eco.U8, 201), (eco.I16, -12345), (eco.F32, 2.5), (eco.U64, 2**63 + 5)):
                v = _value(ec, ct, x)
                full = np.full(NMAX, x, dtype=eco.NP_DTYPES[ct])
                _map_sweep(ec, lambda io, o, n: chk(L.ec_fill(ct, o, n, C.byref(v), s)), full, (0,), typed_offs(size_of(ct)),
                           tile(size_of(ct)), f"ec_fill {eco.CT_NAMES[ct]}", ct)
        elif family == "mask_from_nodata":
            for ct in (eco.U8, eco.I16, eco.F32, eco.U64):
                h = pool.host(ct)
                nd_o, nd_d = eco.Value.of(ct, h[3]), _value(ec, ct, h[3])
                full = cached(("mfn", ct), lambda: eco.f_mask_from_nodata(h, nd_o))
                _map_sweep(ec, lambda io, o, n: chk(L.ec_mask_from_nodata(ct, pool.get(ct, io)[0], n, C.byref(nd_d), o, s)), full, IN_OFFS,
                           BYTE_OFFS, tile(size_of(ct)), f"ec_mask_from_nodata {eco.CT_NAMES[ct]}", ct)
            ones = np.ones(NMAX, np.uint8)   # NoData::None: all true
            _map_sweep(ec, lambda io, o, n: chk(L.ec_mask_from_nodata(eco.U16, pool.get(eco.U16, io)[0], n, None, o, s)), ones, IN_OFFS,
                       BYTE_OFFS, tile(2), "ec_mask_from_nodata without a nodata value", 99)
        elif family == "mask_select":
            for ct in (eco.U8, eco.I16, eco.F32, eco.U64):
                h, hm = pool.host(ct), pool.host_mask(0)
                nd_o, nd_d = eco.nodata_value(eco.ND_DEFAULT, ct), ec._ffi.EcValue()
                chk(L.ec_nodata_default(ct, C.byref(nd_d)))
                full = cached(("sel", ct), lambda: eco.f_mask_select(h, hm, nd_o))
                _map_sweep(ec, lambda io, o, n: chk(L.ec_mask_select(ct, pool.get(ct, io)[0], pool.mask(io, 0)[0], n, C.byref(nd_d), o, s)),
                           full, IN_OFFS, typed_offs(size_of(ct)), tile(size_of(ct)), f"ec_mask_select {eco.CT_NAMES[ct]}", ct)
        elif family == "mask_logic":
            ha, hb = pool.host_mask(0), pool.host_mask(1)
            for name, fn, want in (("and", L.ec_mask_and, eco.mask_and(ha, hb)), ("or", L.ec_mask_or, eco.mask_or(ha, hb))):
                _map_sweep(ec, lambda io, o, n: chk(fn(pool.mask(io, 0)[0], pool.mask(io, 1)[0], n, o, s)), want, IN_OFFS,
                           BYTE_OFFS, tile(1), f"ec_mask_{name}", 5)
            _map_sweep(ec, lambda io, o, n: chk(L.ec_mask_not(pool.mask(io, 0)[0], n, o, s)), eco.mask_not(ha), IN_OFFS, BYTE_OFFS,
                       tile(1), "ec_mask_not", 6)
            # the documented in-place forms (out == l): a window in the middle of an arena, the bytes in front of it AND behind it kept
            for n in sizes(tile(1)):
                for bo in BYTE_OFFS:
                    for name, run, want in (("and", lambda w: L.ec_mask_and(w, pool.mask(0, 1)[0], n, w, s), eco.mask_and(ha[:n], hb[:n])),
                                            ("or", lambda w: L.ec_mask_or(w, pool.mask(0, 1)[0], n, w, s), eco.mask_or(ha[:n], hb[:n])),
                                            ("not", lambda w: L.ec_mask_not(w, n, w, s), eco.mask_not(ha[:n]))):
                        win = Arena(n, offset=bo, seed=_seed(n, bo), ec=ec).hold(ha[:n])
                        chk(run(win.ptr))
                        win.check(want, f"ec_mask_{name} in place n {n} at +{bo} bytes")
        else:
            for ct, seed, lo, hi, ref in ((eco.U8, 0x5EED0001, 0, 255, eco.fill_u8), (eco.U16, 0x5EED0002, 1, 65535, eco.fill_u16)):
                full = cached(("synth", ct), lambda: ref(NMAX, seed, base=5, lo=lo, hi=hi))
                _map_sweep(ec, lambda io, o, n: chk(L.ec_synth_fill(ct, o, n, seed, 5, float(lo), float(hi), s)), full, (0,),
                           typed_offs(size_of(ct)), tile(size_of(ct)), f"ec_synth_fill {eco.CT_NAMES[ct]}", ct)
            full = cached("synth_mask", lambda: (_splitmix64(np.uint64(0x5EED0013) ^ np.arange(7, 7 + NMAX, dtype=np.uint64)) % np.uint64(100)
                                                 >= np.uint64(30)).astype(np.uint8))
            assert full[:64].tolist() == [int(eco.splitmix64(0x5EED0013 ^ (7 + i)) % 100 >= 30) for i in range(64)]   # the numpy restatement
            _map_sweep(ec, lambda io, o, n: chk(L.ec_synth_mask(o, n, 0x5EED0013, 7, 30, s)), full, (0,), BYTE_OFFS, tile(1), "ec_synth_mask", 7)


def _splitmix64(x):
    """splitmix64 over a uint64 array (the oracle's eco_splitmix64, vectorised; checked against it where it is used)."""
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


# ================================================================ device-side records
def _f64_keys(mn, mx):
    """{~key(min), key(max)} of two Float64 oracle values, as ec_min_max_keys writes them."""
    def key(v):
        b = v.bits() - (1 << 64) if v.bits() >> 63 else v.bits()
        return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFF)
    return np.array([~key(mn), key(mx)], dtype=np.int64)


def _record_arena(ec, expected, at, seed):
    """A record in the middle of a small guarded arena, `at` bytes behind a 256-byte boundary."""
    return Arena(expected.nbytes, guard=4096, offset=at, seed=seed, ec=ec).expect(expected)


@pytest.mark.parametrize("n", [1000, 70001], ids=["below-a-tile", "above-a-tile"])
def test_device_records(ec, pool, n):
    """The 16-byte payloads of ec_min_max_keys, ec_expr_min_max_keys and ec_mask_counts_device and the 64-byte ec_moments of
    ec_stats_device: the record equals the oracle's, its neighbours are as they were."""
    L, chk, s = ec.lib(), ec._ffi.check, ec.stream()
    pm, hm = pool.mask(1, 0)
    for ct in (eco.U16, eco.F32, eco.I64):
        p, h = pool.get(ct, 1)
        for masked in (False, True):
            mn, mx = eco.f_min_max(h[:n], hm[:n] if masked else None)
            want = np.array([~R.order_key(ct, mn.get().item()), R.order_key(ct, mx.get().item())], dtype=np.int64)
            for at in (16, 24):
                rec = _record_arena(ec, want, at, n + at)
                chk(L.ec_min_max_keys(ct, p, pm if masked else None, n, rec.ptr, s))
                rec.check(want, f"ec_min_max_keys {eco.CT_NAMES[ct]} n {n} masked {masked} at +{at}")
    # min / max of a program's result: the two-pass form (expr_jit = 0) and, from its first sight, the compiled one
    cts = [eco.U16, eco.I16]
    for jit in (0, 2):
        with ec.tuned(expr_jit=jit):
            for masked in (False, True):
                dt, pp, m, sc, st, full, fmask = _expr_args(ec, pool, cts, [], NDVI, 1, masked)
                want = _f64_keys(*eco.f_min_max(full[:n], fmask[:n] if masked else None))
                for at in (16, 24):
                    rec = _record_arena(ec, want, at, n + at + 1)
                    chk(L.ec_expr_min_max_keys(dt, pp, m if masked else None, 2, sc, 0, st, len(NDVI), n, rec.ptr, s))
                    rec.check(want, f"ec_expr_min_max_keys n {n} masked {masked} expr_jit {jit} at +{at}")
    for mode in (0, 1, 2):
        with ec.tuned(counts_one_launch=mode):
            want = np.array(eco.mask_counts(hm[:n]), dtype=np.uint64)
            for at in (16, 24):
                rec = _record_arena(ec, want, at, n + at + 2)
                chk(L.ec_mask_counts_device(pm, n, rec.ptr, s))
                rec.check(want, f"ec_mask_counts_device n {n} counts_one_launch {mode} at +{at}")
    for ct in (eco.U16, eco.I8):   # the exact integer kind: every byte of the record is pinned
        p, h = pool.get(ct, 1)
        for masked in (False, True):
            ref = R.record(ct, h[:n], hm[:n] if masked else None)
            want = ec._ffi.EcMoments()
            want.count, want.kind, want.dtype, want.reserved = ref["count"], ref["kind"], ref["dtype"], 0
            want.keys2[0], want.keys2[1] = ~R.order_key(ct, ref["min"]), R.order_key(ct, ref["max"])
            want.u.i.sum, want.u.i.sq_lo, want.u.i.sq_hi = ref["sum"], ref["sq"] & (2**64 - 1), ref["sq"] >> 64
            want = np.frombuffer(bytes(want), dtype=np.uint8)
            assert want.size == 64
            for at in (64, 72):
                rec = _record_arena(ec, want, at, n + at + 3)
                chk(L.ec_stats_device(ct, p, pm if masked else None, n, rec.ptr, s))
                rec.check(want, f"ec_stats_device {eco.CT_NAMES[ct]} n {n} masked {masked} at +{at}")


# ================================================================ host memory in, host memory out
@pytest.mark.parametrize("chunk", [0, 777, 5001])
def test_host_expr(ec, chunk):
    """`out_host` and `out_mask_host` are slices in the middle of larger host arrays, guarded and complemented like device
    outputs; the operands are compared with their copies afterwards; one f64 operand serves as `out_host` in place."""
    L, chk = ec.lib(), ec._ffi.check
    n = 5001
    a, b, c = (rand_cells(ct, n, 8100 + ct, specials=False) for ct in (eco.U16, eco.F32, eco.I8))
    a[::37], b[5::41] = 0, np.float32(-9999.0)
    keep = [x.copy() for x in (a, b, c)]
    steps = [(eco.SUB, S(0), S(1), 0), (eco.MUL, S(2), K(0), 1), (eco.DIV, RG(0), RG(1), 2), (eco.ADD, RG(2), S(0), 0)]
    vals = _oracle_steps([a, b, c], [0.5], steps)
    dt, p = (C.c_uint8 * 3)(eco.U16, eco.F32, eco.I8), (C.c_void_p * 3)(a.ctypes.data, b.ctypes.data, c.ctypes.data)
    sc = (ec._ffi.EcValue * 1)(_value(ec, eco.F64, 0.5))
    st = (ec._ffi.EcExprStep * len(steps))(*[ec._ffi.EcExprStep(*s_) for s_ in steps])
    for oo in F64_OFFS:
        out = output(None, vals, oo, seed=chunk + oo)
        chk(L.ec_host_expr(dt, p, 3, sc, 1, st, len(steps), n, out.ptr, chunk))
        out.check(vals, f"ec_host_expr chunk {chunk} out +{oo}")
    # the masked form: nodata 0 in the u16 band, -9999 in the f32 band, none in the i8 band
    valid = eco.f_mask_from_nodata(a, eco.Value.of(eco.U16, 0)) & eco.f_mask_from_nodata(b, eco.Value.of(eco.F32, -9999.0))
    nds = [_value(ec, eco.U16, 0), _value(ec, eco.F32, -9999.0)]
    nd = (C.POINTER(ec._ffi.EcValue) * 3)(C.pointer(nds[0]), C.pointer(nds[1]), C.POINTER(ec._ffi.EcValue)())
    ond = C.c_double(-1e30)
    for oo in F64_OFFS:
        for mo in BYTE_OFFS:
            want = np.where(valid.astype(bool), vals, -1e30)
            out, om = output(None, want, oo, seed=chunk + oo + 7), output(None, valid, mo, seed=chunk + mo + 11)
            chk(L.ec_host_masked_expr(dt, p, nd, 3, sc, 1, st, len(steps), n, out.ptr, C.byref(ond), om.ptr, chunk))
            out.check(want, f"ec_host_masked_expr chunk {chunk} out +{oo}")
            om.check(valid, f"ec_host_masked_expr chunk {chunk} mask +{mo}")
    out = output(None, vals, 1, seed=chunk + 19)   # no output nodata value, no mask wanted: the values of all cells
    chk(L.ec_host_masked_expr(dt, p, nd, 3, sc, 1, st, len(steps), n, out.ptr, None, None, chunk))
    out.check(vals, f"ec_host_masked_expr chunk {chunk}, values of all cells")
    for x, k in zip((a, b, c), keep):
        assert np.array_equal(x.view(np.uint8), k.view(np.uint8)), "a host operand was written"
    # in place (documented: out_host may be one of the f64 operands itself): the operand is the payload of a host arena
    x = rand_cells(eco.F64, n, 8200, specials=False)
    want = eco.f_binop(eco.MUL, x, np.full(n, 2.5))
    for oo in F64_OFFS:
        inout = Arena(8 * n, offset=8 * oo, seed=chunk + oo + 23).hold(x)
        d1, p1 = (C.c_uint8 * 1)(eco.F64), (C.c_void_p * 1)(inout.ptr)
        s1 = (ec._ffi.EcValue * 1)(_value(ec, eco.F64, 2.5))
        t1 = (ec._ffi.EcExprStep * 1)(ec._ffi.EcExprStep(eco.MUL, S(0), K(0), 0))
        chk(L.ec_host_expr(d1, p1, 1, s1, 1, t1, 1, n, inout.ptr, chunk))
        inout.check(want, f"ec_host_expr in place chunk {chunk} at +{oo}")
