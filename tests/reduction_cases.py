"""Inputs for the reduction tests in which ONE cell holds each answer, and the places a reduction kernel can lose a cell.

A reduction returns one or two words per launch.  Over `rand_cells` the minimum and the maximum are held by many cells at
once, so a kernel that skips a lane, a slot of a 16-byte group, the ragged tail, the peeled head or a round of its
grid-stride loop still returns the right words.  Here every field lies in a middle band of the type and two planted cells
are the sole minimum and the sole maximum under the reference's total order; a masked variant hides cells that are more
extreme than the plants (decoys), the neighbours of each plant among them.  `position_classes` names the cells of a window
by where the kernel geometry puts them, `faults` names what a kernel could drop, and `windows` / `cases` list what the GPU
test (test_gpu_reduction_positions.py) runs — tests/test_reduction_inputs.py checks on the CPU, against the oracle, that
every fault changes the answer of at least one listed case.

Nothing is imported from the product: the kernel constants are restated below, each with its source.  Cells travel as
BITS (unsigned integers of the cell's width) wherever a value is planted, so NaN signs and payloads survive unchanged.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from oracle import eco
from oracle.eco import NP_DTYPES

# ---- kernel geometry, restated
WAVE = 64                    # kWave, ec_binop_kernels.hpp
SHAPES = {0: (512, 8), 1: (512, 16), 2: (256, 8), 3: (1024, 8), 4: (512, 4)}   # reduce_shape -> (BLOCK, U): ec_abi.hip launch_min_max
RBLOCK, RU = 512, 8          # k_first_diff_partials / k_mask_count_partials: kRBlock (ec_reduce_kernels.hpp), kReduceU (ec_reduce_plan.hpp); kScanShape, ec_abi.hip
CELLWISE_BLOCK = 256         # k_min_max_partials_cellwise: kBlock (ec_binop_kernels.hpp), at most 8 workgroups per CU (ec_reduce_launch.hpp launch_reduction)
CELLWISE_PER_CU = 8
FINALIZE_BLOCK = 1024        # kFinalizeBlock, ec_reduce_kernels.hpp (finalize_fold): four load slots per thread
MAX_PARTS = 4096             # kMaxReduceBlocks (ec_reduce_plan.hpp, reduce_cap) = kFinalizeMaxParts (ec_reduce_kernels.hpp): the grid's hard cap
JIT_BLOCK, JIT_U, JIT_PER_CU = 256, 4, 8   # generated reduce kernel: 256 threads, 4 PAIRS per lane per tile, grid <= 8 per CU (ec_expr_jit.hip)
# Nothing pins these to the product but the GPU test: it plants at the cells these constants name and fails if the kernels drift only
# where a class then misses its place — re-read the sources when a launch shape changes: the cell geometry is that of the three
# partials kernels (ec_reduce_kernels.hpp), the grid is reduce_plan's (ec_reduce_plan.hpp), the shapes are the launchers' (ec_abi.hip).  JIT_U is the library's default;
# the GPU test refuses to run with EC_EXPR_REDUCE_U set to anything else.
DECOY_STRIDE = 997           # a prime: the hidden cells walk through every slot, lane and in-flight load of any launch shape

_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
INT8 = (eco.U64, eco.I64)
FLOATS = (eco.F32, eco.F64)


def dtype_of(ct: int) -> np.dtype:
    return np.dtype(NP_DTYPES[ct])


def as_bits(a: np.ndarray) -> np.ndarray:
    return a.view(_UINT[a.dtype.itemsize])


def bits_of_value(ct: int, v) -> int:
    return int(as_bits(np.array([v]).astype(dtype_of(ct)))[0])


# ---- the reference's total order, restated in numpy (keys from bits, as oracle/eco.py's CellValue order)
def keys(a: np.ndarray) -> np.ndarray:
    """Integers order as themselves; floats by total_cmp: the bits as a signed integer, the low bits flipped when negative."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    it = np.int32 if a.itemsize == 4 else np.int64
    b = a.view(it)
    return b ^ ((b >> (8 * a.itemsize - 1)) & it(np.iinfo(it).max))


def _limits(dt: np.dtype):
    if dt.kind == "f":
        return np.array([np.finfo(dt).max, np.finfo(dt).min], dt)   # the fold's identities are finite for floats
    return np.array([np.iinfo(dt).max, np.iinfo(dt).min], dt)


def fold_min_max(a: np.ndarray, mask=None, keep=None) -> tuple[int, int]:
    """Bits of (min, max) of the cells where `mask` and `keep` are true, folded from (T::MAX, T::MIN) as the reference does."""
    a = np.ascontiguousarray(a)
    sel = None if mask is None else np.asarray(mask).astype(bool)
    if keep is not None:
        sel = keep if sel is None else (sel & keep)
    k = keys(a)
    khi, klo = keys(_limits(a.dtype))
    kmin = int(k.min(initial=khi)) if sel is None else int(k.min(initial=khi, where=sel))
    kmax = int(k.max(initial=klo)) if sel is None else int(k.max(initial=klo, where=sel))
    out = np.array([kmin, kmax], dtype=keys(a[:0]).dtype)
    if a.dtype.kind == "f":
        out = keys(out.view(a.dtype))     # the key map is its own inverse
    return int(as_bits(out)[0]), int(as_bits(out)[1])


# ---- fields and plants
KINDS_INT = ("extremes", "adjacent")
KINDS_INT8 = KINDS_INT + ("blind63", "blind53")
KINDS_FLOAT = ("extremes", "adjacent", "inf", "nan", "neg_zero", "pos_zero", "subnormal")


def kinds_of(ct: int) -> tuple:
    return KINDS_FLOAT if ct in FLOATS else KINDS_INT8 if ct in INT8 else KINDS_INT


def _band_block(ct: int, seed: int, kind: str) -> np.ndarray:
    """One period of the field: the middle half of an integer type, finite non-zero normal floats of moderate size."""
    dt = dtype_of(ct)
    rng = np.random.default_rng(seed * 7919 + ct)
    period = (1 << 16) + 1   # odd: the field never lines up with a tile, a wave or a group
    if kind in ("neg_zero", "subnormal"):
        return np.zeros(period, dt)
    if kind == "pos_zero":
        return -np.zeros(period, dt)
    if dt.kind == "f":
        return ((rng.uniform(1.0, 999.0, period) * 10.0 ** rng.integers(-3, 4, period)) * rng.choice([-1.0, 1.0], period)).astype(dt)
    info = np.iinfo(dt)
    if kind == "blind53":        # every cell below 2^53 in magnitude: f64 holds them exactly, and not the plants
        lo, hi = ((1 << 52) + 2, (1 << 53) - 1) if dt.kind == "u" else (-(1 << 53) + 1, (1 << 53) - 1)
    elif kind == "blind63":      # a band that tops out two below the type's (or i64's) maximum
        lo, hi = (1 << 62, (1 << 63) - 3) if dt.kind == "u" else (info.min + 2, info.max - 2)
    else:
        q = (int(info.max) - int(info.min)) // 4
        lo, hi = int(info.min) + q, int(info.max) - q
    return rng.integers(lo, hi, size=period, dtype=dt, endpoint=True)


def plant_bits(ct: int, kind: str, block: np.ndarray):
    """(bits of the sole minimum or None, bits of the sole maximum or None, bits of the runners-up scattered over the field)."""
    dt = dtype_of(ct)
    U = _UINT[dt.itemsize]
    w = 8 * dt.itemsize
    b = lambda v: bits_of_value(ct, v)   # noqa: E731
    kb = keys(block)
    vmin, vmax = block[int(np.argmin(kb))], block[int(np.argmax(kb))]
    if kind == "extremes":
        hi, lo = _limits(dt)
        return b(lo), b(hi), []
    if kind == "adjacent":
        if dt.kind == "f":
            return b(np.nextafter(vmin, dt.type(-np.inf))), b(np.nextafter(vmax, dt.type(np.inf))), []
        return b(int(vmin) - 1), b(int(vmax) + 1), []
    if kind == "wide":           # 8-byte integers seen through f64 (an expression program): 2^13 beyond the band, four f64 steps at 2^63
        return b(int(vmin) - (1 << 13)), b(int(vmax) + (1 << 13)), []
    if kind == "blind63":        # 2^63 - 1 against 2^63 - 2: one f64; u64 also gets a minimum of 2^63 - ... below the band
        if dt.kind == "u":
            return (1 << 62) - 1, (1 << 63) - 1, [(1 << 63) - 2, 1 << 62]
        return int(U(1 << 63)), (1 << 63) - 1, [(1 << 63) - 2, int(U((1 << 63) + 1))]
    if kind == "blind53":        # 2^53 + 1 against 2^53: `as f64` rounds the plant onto its runner-up
        if dt.kind == "u":
            return 1 << 52, (1 << 53) + 1, [1 << 53, (1 << 52) + 1]
        return int(U((1 << 64) - (1 << 53) - 1)), (1 << 53) + 1, [1 << 53, int(U((1 << 64) - (1 << 53)))]
    sign = 1 << (w - 1)
    if kind == "inf":
        return b(-np.inf), b(np.inf), []
    if kind == "nan":            # negative NaNs order below -inf, positive above +inf, larger payloads further out: payload 5 beats 1
        quiet = b(np.nan) & ~sign
        inf = b(np.inf)
        return sign | quiet | 5, quiet | 5, [sign | quiet | 1, quiet | 1, sign | inf | 1, inf | 1, b(-np.inf), b(np.inf)]
    if kind == "neg_zero":       # +0.0 everywhere, one -0.0: the minimum comes back with bits 0x8000...
        return sign, None, []
    if kind == "pos_zero":       # -0.0 everywhere, one +0.0
        return None, 0, []
    if kind == "subnormal":      # the smallest subnormals of either sign around a field of zeros
        return sign | 1, 1, []
    raise ValueError(kind)


def decoy_bits(ct: int) -> tuple[int, int]:
    """Values beyond every plant, for cells the mask hides: the type's MIN / MAX, for floats NaNs of both signs with every payload bit set."""
    dt = dtype_of(ct)
    if dt.kind == "f":
        ones = (1 << (8 * dt.itemsize)) - 1
        return ones, ones >> 1
    hi, lo = _limits(dt)
    return bits_of_value(ct, lo), bits_of_value(ct, hi)


def field_cells(ct: int, n: int, seed: int, kind: str = "adjacent") -> np.ndarray:
    """The field without its two plants: the band, with the kind's runners-up at a few hundred scattered cells."""
    block = _band_block(ct, seed, kind)
    a = np.resize(block, n)
    runners = plant_bits(ct, kind, block)[2]
    for j, r in enumerate(runners):
        as_bits(a)[(37 + 211 * j)::(1009 * len(runners))] = r
    return a


def sole_extreme_cells(ct: int, n: int, i_min, i_max, seed: int, kind: str = "adjacent") -> np.ndarray:
    """n cells of type ct in which cell i_min is strictly below and cell i_max strictly above every other cell under the total
    order.  `kind` chooses the plants (see `plant_bits`); a kind that has only one plant ignores the other index."""
    a = field_cells(ct, n, seed, kind)
    mn, mx, _ = plant_bits(ct, kind, _band_block(ct, seed, kind))
    if mn is not None and i_min is not None:
        as_bits(a)[i_min] = mn
    if mx is not None and i_max is not None:
        assert i_max != i_min or mn is None
        as_bits(a)[i_max] = mx
    return a


def hide_decoys(ct: int, a: np.ndarray, plants=()) -> np.ndarray:
    """Turns `a` into the masked variant IN PLACE and returns its mask: every DECOY_STRIDE-th cell and both neighbours of every
    plant are hidden and hold a value beyond the plants.  A kernel that ignores the mask, or reads it one cell off, returns one."""
    mask = np.ones(a.size, np.uint8)
    lo, hi = decoy_bits(ct)
    v = as_bits(a)
    near = [q for p in plants for q in (p - 1, p + 1) if 0 <= q < a.size]
    idx = np.concatenate([np.arange(DECOY_STRIDE // 2, a.size, DECOY_STRIDE), np.array(near, dtype=np.int64)]).astype(np.int64)
    idx = idx[~np.isin(idx, np.array(list(plants), dtype=np.int64))]
    v[idx] = np.where(idx % 2 == 1, v.dtype.type(lo), v.dtype.type(hi))
    mask[idx] = 0
    return mask


def _from_keys(k: np.ndarray, dt: np.dtype) -> np.ndarray:
    return keys(k.view(dt)).view(dt) if dt.kind == "f" else k.astype(dt)


def differing_bits(a: np.ndarray, q: int, up: bool) -> int:
    """Bits of the neighbour of cell q under the total order: the next larger value (`up`) or the next smaller; at the end of
    the type's range the other one."""
    kt = keys(a[:0]).dtype
    info = np.iinfo(kt)
    k = int(keys(a[q:q + 1])[0])
    nk = k + 1 if (up and k != int(info.max)) or k == int(info.min) else k - 1
    return int(as_bits(_from_keys(np.array([nk], dtype=kt), a.dtype))[0])


def sole_difference(a: np.ndarray, i: int, later=()) -> np.ndarray:
    """A copy of `a` that differs from it at cell i and at the `later` indices, and nowhere else.  Cell i becomes the next LARGER
    value under the total order and the later cells the next smaller, so the ordering of the two buffers tells which difference
    was found."""
    b = a.copy()
    for q, up in [(i, True)] + [(j, False) for j in later]:
        as_bits(b)[q] = differing_bits(a, q, up)
    return b


def sole_true_mask(n: int, i: int) -> np.ndarray:
    m = np.zeros(n, np.uint8)
    m[i] = 1
    return m


def sole_false_mask(n: int, i: int) -> np.ndarray:
    m = np.ones(n, np.uint8)
    m[i] = 0
    return m


# ---- where a cell sits in the launch
@dataclass(frozen=True)
class Geometry:
    """A window of n cells, `head` of them in front of the first 16-byte boundary, under a launch of `block` threads with `u`
    16-byte loads in flight per lane and `grid` workgroups (None: one per tile).  `cpg` = cells per 16-byte group (the generated
    kernel: cells per PAIR, 2)."""
    n: int
    cell_size: int
    block: int
    u: int
    head: int = 0
    grid: int | None = None
    cpg: int | None = None
    finalize: bool = True   # the workgroups' partials are folded by the finalize kernel (the generated kernel joins with atomics)

    @property
    def cpl(self):
        return self.cpg or 16 // self.cell_size

    @property
    def tile_groups(self):
        return self.block * self.u

    @property
    def tile(self):
        return self.tile_groups * self.cpl

    @property
    def ngroups(self):
        return (self.n - self.head) // self.cpl

    @property
    def nfull(self):
        return self.ngroups // self.tile_groups

    @property
    def ntiles(self):
        return max(1, -(-self.ngroups // self.tile_groups))

    @property
    def workgroups(self):
        return min(self.ntiles, self.grid) if self.grid else self.ntiles

    def cell(self, tile: int, j: int, thread: int, k: int) -> int:
        return self.head + ((tile * self.tile_groups) + j * self.block + thread) * self.cpl + k

    def coords(self):
        """Per cell of the window: (is_body, tile, j, thread, k); head and tail cells have is_body False."""
        i = np.arange(self.n, dtype=np.int32 if self.n < 2**31 - 64 else np.int64) - self.head
        body = (i >= 0) & (i < self.ngroups * self.cpl)
        g = np.where(body, i // self.cpl, 0)
        in_tile = g % self.tile_groups
        return body, g // self.tile_groups, in_tile // self.block, in_tile % self.block, np.where(body, i % self.cpl, 0)


def position_classes(n: int, cell_size: int, block: int, u: int, head: int, grid: int | None = None, cpg: int | None = None,
                     finalize: bool = True) -> dict:
    """Named cell indices of a window of n cells: one per place the kernel geometry distinguishes (module docstring).  A class
    that the window does not have (no full tile, no tail, ...) is absent."""
    ge = Geometry(n, cell_size, block, u, head, grid, cpg)
    cpl, waves, out = ge.cpl, block // WAVE, {}
    body_end = head + ge.ngroups * cpl
    for h in range(head):
        out[f"head{h}"] = h
    for r in range(n - body_end):
        out[f"tail{r}"] = body_end + r
    if n:
        out["first_cell"], out["last_cell"] = 0, n - 1
    if ge.nfull:
        t0, t1 = 0, ge.nfull - 1
        for k in range(cpl):                      # every element slot of one group, in a wave whose other lanes are ordinary
            out[f"slot{k}"] = ge.cell(t0, 1 % u, WAVE * (1 % waves) + 5, k)
        for lane in range(WAVE):                  # every lane of one wave
            out[f"lane{lane}"] = ge.cell(t1, u - 1, WAVE * (waves - 1) + lane, lane % cpl)
        for w in range(waves):                    # the two edge lanes of every wave of a workgroup
            out[f"wave{w}_lane0"] = ge.cell(t0, 0, WAVE * w, w % cpl)
            out[f"wave{w}_lane63"] = ge.cell(t0, 0, WAVE * w + 63, (w + 1) % cpl)
        for j in range(u):                        # every in-flight load
            out[f"load{j}"] = ge.cell(t1, j, block // 2 + 1, j % cpl)
        out["tile_first"], out["tile_last"] = ge.cell(t1, 0, 0, 0), ge.cell(t1, u - 1, block - 1, cpl - 1)
    part = ge.ngroups - ge.nfull * ge.tile_groups
    if part:
        g0 = ge.nfull * ge.tile_groups
        out["partial_first"] = head + g0 * cpl
        out["partial_last_group"] = head + (ge.ngroups - 1) * cpl + (cpl - 1)
        out["partial_inner"] = head + (g0 + part // 2) * cpl + 1 % cpl
    nt, wg = ge.ntiles, ge.workgroups

    def in_tile(t, salt):                         # a cell of tile t (its first group when the tile is the partial one)
        return ge.cell(t, salt % u, (salt * 37) % block, salt % cpl) if t < ge.nfull else head + t * ge.tile_groups * cpl + salt % cpl
    if ge.ngroups:
        for b in (0, 1, 63, 64, wg - 1):          # the tile owned by workgroup b in the first round
            if 0 <= b < wg:
                out[f"wg{b}"] = in_tile(b, b + 3)
        if wg > FINALIZE_BLOCK and finalize:      # the finalize kernel's four load slots and their wave boundaries
            for p in (1023, 1024, 2047, 2048, 3071, 3072, wg - 1):
                if p < wg:
                    out[f"partial_word{p}"] = in_tile(p, p)
        if nt > wg:                               # tiles that only a later round of the grid-stride loop reaches
            out["round1"] = in_tile(wg + min(5, nt - wg - 1), 11)
            last = (nt - 1) // wg
            out["round_last"] = in_tile(last * wg, 13)
            out["round_last_end"] = in_tile(nt - 1, 17)
    return out


def faults(ge: Geometry, fine: bool = True) -> dict:
    """What a kernel could leave out of its fold, as boolean arrays over the window's cells (True = dropped).  `fine` = False
    leaves out the families below a tile (slots, lanes, waves, loads): a very long window lists the workgroup-level ones only."""
    body, tile, j, th, k = ge.coords()
    idx = np.arange(ge.n)
    full = body & (tile < ge.nfull)
    out = {}
    if ge.head:
        out["head"] = idx < ge.head
    if ge.n > ge.head + ge.ngroups * ge.cpl:
        out["tail"] = idx >= ge.head + ge.ngroups * ge.cpl
        out["tail_first"] = idx == ge.head + ge.ngroups * ge.cpl     # the tail loop started one cell late
    out["first_cell"], out["last_cell"] = idx == 0, idx == ge.n - 1
    if ge.nfull and fine:
        for s in range(ge.cpl):
            out[f"slot{s}"] = body & (k == s)
        for lane in range(WAVE):
            out[f"lane{lane}"] = body & (th % WAVE == lane)
        for w in range(ge.block // WAVE):
            out[f"wave{w}_lane0"] = body & (th == WAVE * w)
            out[f"wave{w}_lane63"] = body & (th == WAVE * w + 63)
            out[f"wave{w}_tile0"] = body & (th // WAVE == w) & (tile == 0)
        for q in range(ge.u):
            out[f"load{q}"] = full & (j == q)
        out["tile_first"] = full & (j == 0) & (th == 0) & (k == 0)
        out["tile_last"] = full & (j == ge.u - 1) & (th == ge.block - 1) & (k == ge.cpl - 1)
    if ge.ngroups > ge.nfull * ge.tile_groups:
        part = body & (tile == ge.nfull)
        g = (idx - ge.head) // ge.cpl
        out["partial_tile"] = part
        out["partial_first_group"] = part & (g == ge.nfull * ge.tile_groups)
        out["partial_last_group"] = part & (g == ge.ngroups - 1)
        out["partial_inner"] = part & ~out["partial_first_group"] & ~out["partial_last_group"]
    wg, nt = ge.workgroups, ge.ntiles
    if ge.ngroups:
        for b in sorted({0, 1, 63, 64, wg - 1}):
            if 0 <= b < wg and wg > 1:
                out[f"wg{b}"] = body & (tile % wg == b)
        if wg > FINALIZE_BLOCK and ge.finalize:
            for s in range(-(-wg // FINALIZE_BLOCK)):
                out[f"finalize_slot{s}"] = body & ((tile % wg) // FINALIZE_BLOCK == s)
            for p in (1023, 1024, 2047, 2048, 3071, 3072):
                if p < wg:
                    out[f"partial_word{p}"] = body & (tile % wg == p)
        if nt > wg:
            for r in sorted({1, (nt - 1) // wg}):
                out[f"round{r}"] = body & (tile // wg == r)
    return out


def mask_faults(ge: Geometry) -> dict:
    """Places where a kernel could ignore the mask: boolean arrays (True = the cell is folded whatever its mask byte says)."""
    body, _, _, _, k = ge.coords()
    idx = np.arange(ge.n)
    out = {}
    if ge.head:
        out["ignore_mask_head"] = idx < ge.head
    if ge.n > ge.head + ge.ngroups * ge.cpl:
        out["ignore_mask_tail"] = idx >= ge.head + ge.ngroups * ge.cpl
    if ge.ngroups:
        for s in range(ge.cpl):
            out[f"ignore_mask_slot{s}"] = body & (k == s)
    return out


# ---- the windows and the cases the GPU test runs
@dataclass(frozen=True)
class Window:
    name: str
    ge: Geometry
    classes: tuple          # names of the position classes run on this window ("*" = all it has)
    knobs: tuple = ()       # ((knob, value), ...) the window needs


@dataclass
class Case:
    window: Window
    name_min: str
    i_min: int
    name_max: str
    i_max: int
    kind: str = "adjacent"
    masked: bool = False
    extra_hidden: tuple = field(default_factory=tuple)

    def label(self):
        return f"{self.window.name} {'masked ' if self.masked else ''}{self.kind} min@{self.name_min}[{self.i_min}] max@{self.name_max}[{self.i_max}]"


def _pick(classes: dict, wanted) -> list:
    if "*" in wanted:
        return list(classes.items())
    return [(nm, i) for nm, i in classes.items() if any(nm == w or (w.endswith("*") and nm.startswith(w[:-1])) for w in wanted)]


def window_positions(w: Window) -> list:
    ge = w.ge
    if ge.n <= ge.cpl + 1 and not ge.head:
        return [(f"cell{i}", i) for i in range(ge.n)]
    seen, out = set(), []
    for nm, i in _pick(position_classes(ge.n, ge.cell_size, ge.block, ge.u, ge.head, ge.grid, ge.cpg, ge.finalize), w.classes):
        if i not in seen:      # one cell under two names (a partial tile of one group, ...) is run once, under the first
            seen.add(i)
            out.append((nm, i))
    return out


def rotate_cases(w: Window, kind="adjacent", masked=False) -> list:
    """Every position of the window once as the sole minimum and once as the sole maximum: case r plants the minimum at position r
    and the maximum at position r + 1."""
    pos = window_positions(w)
    extra = window_decoys(w.ge) if masked else ()
    if len(pos) == 1:
        return [Case(w, pos[0][0], pos[0][1], "-", None, kind, masked, extra)]
    return [Case(w, pos[r][0], pos[r][1], pos[(r + 1) % len(pos)][0], pos[(r + 1) % len(pos)][1], kind, masked, extra) for r in range(len(pos))]


SMALL_CLASSES = ("first_cell", "last_cell", "tile_first", "tile_last", "partial_*", "tail*", "slot0", "lane63", "wg*")


def min_max_windows(cell_size: int, shape: int) -> list:
    """Windows of the vector kernel under one launch shape, small enough that the grid is one workgroup per tile."""
    block, u = SHAPES[shape]
    cpl = 16 // cell_size
    tile = block * u * cpl
    G = lambda n, head=0: Geometry(n, cell_size, block, u, head)   # noqa: E731
    ws = [Window(f"n={n}", G(n), ("*",)) for n in sorted({1, 2, cpl - 1, cpl, cpl + 1} - {0})]
    ws += [Window("one_tile", G(tile), SMALL_CLASSES), Window("one_workgroup_ragged", G(tile - 3 if cpl > 1 else tile - 1), SMALL_CLASSES),
           Window("two_workgroups", G(tile + cpl), SMALL_CLASSES), Window("two_workgroups_ragged", G(tile + 2 * cpl - 1), SMALL_CLASSES)]
    main_n = 2 * tile + (block * u // 2 + 7) * cpl + (cpl - 1)
    ws.append(Window("main", G(main_n), ("*",)))
    for h in range(1, cpl):   # the window starts cpl - h cells past a 16-byte boundary: h cells are peeled
        ws.append(Window(f"head={h}", G(main_n + h, h), ("head*", "tile_first", "tail*", "partial_last_group")))
    ws.append(Window("66_workgroups", G(65 * tile + 3 * cpl + (cpl - 1)), ("wg*", "first_cell", "last_cell")))
    return ws


def capped_windows(cell_size: int, cus: int) -> list:
    """Default launch shape with the grid capped below the tile count: reduce_bpc = 1 (one workgroup per CU, so later rounds of the
    grid-stride loop exist) and reduce_bpc = 100 (the hard cap of MAX_PARTS workgroups: every load slot of the finalize kernel)."""
    block, u = SHAPES[0]
    cpl = 16 // cell_size
    tile = block * u * cpl
    ws = [Window("rounds", Geometry(2 * cus * tile + 2 * tile + 5 * cpl + (cpl - 1), cell_size, block, u, 0, cus),
                 ("round*", "wg*", "tail*", "last_cell"), (("reduce_bpc", 1),))]
    cap = min(100 * cus, MAX_PARTS)
    ws.append(Window("capped_grid", Geometry(cap * tile + 9 * cpl, cell_size, block, u, 0, cap),
                     ("partial_word*", "wg*", "round*", "last_cell"), (("reduce_bpc", 100),)))
    return ws


def cellwise_window(cell_size: int, cus: int) -> Window:
    """k_min_max_partials_cellwise (unaligned_vector = 0 at an odd offset): one cell per thread, stride 256 x grid, grid <= 8 per CU.
    As a Geometry: 'groups' of one cell, one load in flight."""
    grid = CELLWISE_PER_CU * cus
    n = 2 * grid * CELLWISE_BLOCK + 3 * CELLWISE_BLOCK + 17
    return Window("cellwise", Geometry(n, cell_size, CELLWISE_BLOCK, 1, 0, grid, 1),
                  ("first_cell", "last_cell", "round*", "wg*", "lane0", "lane63", "wave*", "partial_*"), (("unaligned_vector", 0),))


ORDER_CLASSES = ("slot1", "tail0", "head0", "partial_inner")


def order_kind_windows(cell_size: int, shape: int = 0) -> list:
    """The reduced set of positions the order kinds run at: one element slot, the tail, the head and the partial tile."""
    block, u = SHAPES[shape]
    cpl = 16 // cell_size
    tile = block * u * cpl
    n = tile + (block * u // 2 + 7) * cpl + max(cpl - 1, 1)
    head = 1 if cpl > 1 else 0
    return [Window("order", Geometry(n + head, cell_size, block, u, head), ORDER_CLASSES + (("slot0",) if cpl == 1 else ()))]


def case_edits(ct: int, case: Case, block: np.ndarray) -> tuple[dict, dict, tuple]:
    """What a case writes into its window: ({cell index: bits}, {mask index: byte}, (bits of the expected min or None, max or None))."""
    mn, mx, _ = plant_bits(ct, case.kind, block)
    cells, mask = {}, {}
    plants = [p for p, b in ((case.i_min, mn), (case.i_max, mx)) if p is not None and b is not None]
    if case.masked:
        lo, hi = decoy_bits(ct)
        near = [q for p in plants for q in (p - 1, p + 1)]
        for q in near + list(case.extra_hidden):
            if 0 <= q < case.window.ge.n and q not in plants:
                cells[q], mask[q] = (lo if q % 2 else hi), 0
        for p in plants:
            mask[p] = 1
    if mn is not None and case.i_min is not None:
        cells[case.i_min] = mn
    if mx is not None and case.i_max is not None:
        cells[case.i_max] = mx
    return cells, mask, (mn if case.i_min is not None else None, mx if case.i_max is not None else None)


def runs(edits: dict) -> list:
    """{index: value} as [(start, [values...])] over contiguous indices: one small upload per run."""
    out = []
    for i in sorted(edits):
        if out and out[-1][0] + len(out[-1][1]) == i:
            out[-1][1].append(edits[i])
        else:
            out.append((i, [edits[i]]))
    return out


class HostPool:
    """A long field of one type with its masked twin (decoys at every DECOY_STRIDE-th cell, mask byte 0 there); windows are
    slices, plants are written in place and put back.  `base` is the pool index of a 16-byte boundary."""

    def __init__(self, ct: int, n: int, seed: int, kind: str = "adjacent", masked: bool = True):
        self.ct, self.kind = ct, kind
        self.block = _band_block(ct, seed, kind)
        self.cpl = 16 // dtype_of(ct).itemsize
        self.base = self.cpl
        self.plain = field_cells(ct, n + 2 * self.cpl, seed, kind)
        self.hidden = self.plain.copy() if masked else None
        self.mask = hide_decoys(ct, self.hidden) if masked else None

    def offset(self, ge: Geometry) -> int:
        return self.base + 1 if ge.cpg == 1 else self.base - ge.head   # the cell-wise form (cpg 1) runs at an odd cell offset

    def arrays(self, case_or_masked):
        masked = case_or_masked.masked if isinstance(case_or_masked, Case) else case_or_masked
        return (self.hidden, self.mask) if masked else (self.plain, None)

    def poke(self, arr: np.ndarray, off: int, edits: dict) -> dict:
        """Writes the edits (window indices) and returns what undoes them."""
        v = as_bits(arr)
        old = {i: int(v[off + i]) for i in edits}
        for i, b in edits.items():
            v[off + i] = b
        return old


def window_decoys(ge: Geometry) -> tuple:
    """Window-level hidden cells of the masked variant: every head cell and every tail cell (the stride alone may miss them)."""
    tail0 = ge.head + ge.ngroups * ge.cpl
    return tuple(range(ge.head)) + tuple(range(tail0, ge.n))


def min_max_cases(ct: int, shape: int) -> list:
    """Every case of the vector kernel under one launch shape: each window's positions, plain and masked with decoys."""
    out = []
    for w in min_max_windows(dtype_of(ct).itemsize, shape):
        out += rotate_cases(w) + rotate_cases(w, masked=True)
    return out


def capped_cases(ct: int, cus: int) -> list:
    out = []
    for w in capped_windows(dtype_of(ct).itemsize, cus):
        out += rotate_cases(w) + rotate_cases(w, masked=True)
    return out


def cellwise_cases(ct: int, cus: int) -> list:
    w = cellwise_window(dtype_of(ct).itemsize, cus)
    return rotate_cases(w) + rotate_cases(w, masked=True)


def order_cases(ct: int) -> list:
    """Every order kind of the type at the reduced set of positions, plain and (where the decoys lie beyond the plants) masked."""
    out = []
    for kind in kinds_of(ct):
        for w in order_kind_windows(dtype_of(ct).itemsize):
            out += rotate_cases(w, kind)
            if (plant_bits(ct, kind, _band_block(ct, 0, kind))[:2]) != decoy_bits(ct):
                out += rotate_cases(w, kind, masked=True)
    return out


def jit_windows(cus: int, head: int = 0) -> list:
    """Windows of the generated reduce kernel (ec_expr_jit.hip): pairs of cells, 256 threads x 4 pairs per tile, the peeled head cell
    and the odd tail cell folded by lanes 0 and 1 of workgroup 0, the grid capped at 8 workgroups per CU, an atomic join."""
    tile = JIT_BLOCK * JIT_U * 2
    G = lambda n, grid=None: Geometry(n + head, 8, JIT_BLOCK, JIT_U, head, grid, 2, False)   # noqa: E731
    grid = JIT_PER_CU * cus
    return [Window("jit_main", G(2 * tile + 2 * (JIT_BLOCK * JIT_U // 2 + 7) + 1), ("*",)),
            Window("jit_one_tile", G(tile), ("first_cell", "last_cell", "slot*")),
            Window("jit_second_round", G(grid * tile + 2 * tile + 11, grid), ("round*", "wg*", "first_cell", "last_cell"))]


def detect(pool: HostPool, case: Case, drop=None, ignore_mask=None, image=None) -> bool:
    """Does the reference answer of `case` change when the cells `drop` are left out of the fold, or the mask is ignored at
    `ignore_mask`?  The plants are written into the pool's window and put back."""
    ge = case.window.ge
    off = pool.offset(ge)
    cells, mask = pool.arrays(case)
    ce, me, _ = case_edits(pool.ct, case, pool.block)
    old_c = pool.poke(cells, off, ce)
    old_m = pool.poke(mask, off, me) if case.masked else {}
    try:
        a, m = cells[off:off + ge.n], (mask[off:off + ge.n] if case.masked else None)
        if image is not None:      # the cells as an expression program sees them (the oracle's f64 image)
            a = image(a)
        want = fold_min_max(a, m)
        if ignore_mask is not None:
            m = m | ignore_mask.astype(np.uint8)
        return fold_min_max(a, m, None if drop is None else ~drop) != want
    finally:
        pool.poke(cells, off, old_c)
        if case.masked:
            pool.poke(mask, off, old_m)


def undetected(pool: HostPool, cases: list, fine_windows=("main", "order", "jit_main"), image=None) -> tuple[list, int]:
    """Every fault of every window of `cases` against the cases of that window: (names no case of any window detects, how many
    fault names there were).  A fault is looked for in the cases that have a plant (or, for the mask faults, a decoy) inside it."""
    by_window = {}
    for c in cases:
        by_window.setdefault(c.window.name, []).append(c)
    names, found = set(), set()
    for wname, cs in sorted(by_window.items(), key=lambda kv: kv[0] not in fine_windows):
        ge = cs[0].window.ge
        for name, drop in faults(ge, fine=wname in fine_windows).items():
            names.add(name)
            if name in found:
                continue
            hit = [c for c in cs if (c.i_min is not None and drop[c.i_min]) or (c.i_max is not None and drop[c.i_max])]
            if hit and detect(pool, hit[0], drop=drop, image=image):
                found.add(name)
        masked = [c for c in cs if c.masked]
        for name, ign in (mask_faults(ge).items() if masked else ()):
            names.add(name)
            if name not in found and any(detect(pool, c, ignore_mask=ign, image=image) for c in masked[:3]):
                found.add(name)
    return sorted(names - found), len(names)


def expr_kind(ct: int) -> str:
    """The plants an expression program is given: 8-byte integers reach it as f64, so theirs lie wider than the f64 spacing."""
    return "wide" if ct in INT8 else "adjacent"


def later_first_pairs(ge: Geometry) -> list:
    """Two differences (name, i, later) with i < later, where the LATER cell sits in a place a first-difference kernel looks at no
    later than cell i: a higher slot of the same group (the group is walked from its last cell down), a later load of the same
    thread, a lower lane, a lower workgroup in a later round, the tail (workgroup 0) against a tile of a higher workgroup, the body
    against the head.  Built from the geometry; a relation the window does not have is absent."""
    out, cpl = [], ge.cpl
    if ge.nfull:
        t = ge.nfull - 1
        if cpl > 1:
            out.append(("higher_slot_same_group", ge.cell(t, 0, 70 % ge.block, 0), ge.cell(t, 0, 70 % ge.block, cpl - 1)))
        if ge.u > 1:
            out.append(("later_load_same_thread", ge.cell(t, 0, 5, 1 % cpl), ge.cell(t, 1, 5, 0)))
            out.append(("lower_lane_later_load", ge.cell(t, 0, ge.block - 1, 0), ge.cell(t, 1, 0, cpl - 1)))
            out.append(("lower_wave_later_load", ge.cell(t, ge.u - 2, WAVE * (ge.block // WAVE - 1) + 3, 0), ge.cell(t, ge.u - 1, 3, 0)))
    wg, nt = ge.workgroups, ge.ntiles
    if nt > wg and ge.nfull > wg:
        out.append(("lower_workgroup_later_round", ge.cell(wg - 1, 0, 9 % ge.block, 0), ge.cell(wg, 0, 9 % ge.block, 0)))
    body_end = ge.head + ge.ngroups * cpl
    if ge.n > body_end and ge.nfull >= 2:
        out.append(("tail_of_workgroup0_after_workgroup1", ge.cell(1, 0, 11 % ge.block, 0), body_end))
    if ge.head and ge.ngroups:
        out.append(("body_after_head", ge.head - 1, ge.head))
        out.append(("body_after_first_head_cell", 0, ge.head + cpl - 1))
    return out
