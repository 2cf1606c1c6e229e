"""The inputs of the special-operand tests: per cell type a short list of special values, and layouts of the lattice
`specials(lt) x specials(rt)` of operand pairs that put each pair where the kernels treat cells differently.

The kernels work on tiles of pairs of cells: 256 lanes x U pairs per workgroup, U = 2 for the binops (kBinopU, ec_runtime.hpp;
the LDS-staged form: 4 waves x 256 cells, ec_binop_kernels.hpp), the two-level kernel (kFusedU) and the ahead-of-time kernels
(kFixedU), U = 3 for the interpreter (kExprU, ec_expr.hpp; the frame: ec_stream_tile.hpp) — tiles of 1024, 1024, 1024 and 1536
cells.  A lane tests the NaN rule once per pair of cells and a wave repairs behind a ballot; a peeled head cell, the odd tail cell and
the ragged last tile run per-cell code.

  A  `layout_a`: the cross product, row-major, repeated cyclically to 4609 cells: three tiles of the widest kernel and one cell more,
     an odd length that no tile divides — full tiles whose waves hold many NaNs, a ragged tile and a tail cell.
  B  `layout_b`: every pair with a NaN operand or a NaN result planted alone among ordinary finite cells, once at an even and
     once at an odd index, B_STRIDE = 1538 cells apart (one more for the odd ones): any window of 1536 cells — the widest tile,
     wherever it starts — holds at most one special cell, so that cell is the only NaN of its wave, in slot 0 and in slot 1.
  C  `layout_c`: the same pairs as buffers of 1, 2, 3 and 5 cells, and as the first and the last cell of a 7-cell buffer that is read
     one cell into its allocation (head cell, tail cell, ragged tile: per-cell code only).
  T  `chain_values`: ten values per float type for chains, used as T^3 and T^4 (`chain_grid`).
"""
import itertools

import numpy as np

import ieee_ref as R

F64_BITS = [
    0x0000000000000000, 0x8000000000000000,                      # +-0
    0x3FF0000000000000, 0xBFF0000000000000,                      # +-1
    0x7FF0000000000000, 0xFFF0000000000000,                      # +-inf
    0x7FF8000000000001, 0xFFF8000000000000, 0xFFFFFFFFFFFFFFFF,  # quiet NaNs
    0x7FF0000000000001, 0xFFF4000000000002,                      # signalling NaNs
    0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF,                      # +-max
    0x0000000000000001, 0x8000000000000001,                      # +-5e-324
    0x000FFFFFFFFFFFFF, 0x0010000000000000,                      # the largest subnormal, 2^-1022
    0x1E60000000000000,                                          # 2^-537: its square is 5e-324
    0x5FF0000000000000,                                          # 2^512: its square overflows
    0x4340000000000000, 0x3FF0000000000001, 0x3FEFFFFFFFFFFFFF,  # 2^53, 1 + 2^-52, 1 - 2^-53
    0x4008000000000000, 0x3FD5555555555555, 0x3FB999999999999A,  # 3, 1/3, 0.1
    0x7E37E43C8800759C, 0x01A56E1FC2F8F359,                      # 1e300, 1e-300
    0x3FE0000000000000, 0x4000000000000000, 0xC008000000000000,  # 0.5, 2, -3
]
F32_BITS = [
    0x00000000, 0x80000000, 0x3F800000, 0xBF800000, 0x7F800000, 0xFF800000,   # +-0, +-1, +-inf
    0x7FC00001, 0xFFC00000, 0xFFFFFFFF, 0x7F800001,                           # quiet NaNs, a signalling NaN
    0x7F7FFFFF, 0xFF7FFFFF,                                                   # +-max
    0x00000001, 0x80000001, 0x007FFFFF, 0x00800000,                           # +-1e-45, the largest subnormal, 2^-126
    0x4B800000, 0x4B800001,                                                   # 2^24, 2^24 + 2
    0x7F000000, 0x00000400,                                                   # 2^127, a subnormal: products overflow / underflow f32, not f64
    0x3F800001, 0x3F7FFFFF,                                                   # 1 + 2^-23, 1 - 2^-24
    0x40400000, 0x3EAAAAAB, 0x3DCCCCCD, 0x7149F2CA, 0x0DA24260,               # 3, 1/3, 0.1, 1e30, 1e-30
    0x3F000000, 0x40000000, 0xC0400000,                                       # 0.5, 2, -3
]
_AROUND = [2**53, 2**53 + 1, 2**53 + 3, 2**62 + 1, 2**63 - 1025, 2**63 - 1, 2**64 - 1, 2**64 - 1025]  # where `as f64` rounds


def specials(ct: int) -> np.ndarray:
    """The special values of a cell type, as an array of that type."""
    dt = np.dtype(R.NP_DTYPES[ct])
    if ct == R.F64:
        return np.array(F64_BITS, dtype=np.uint64).view(np.float64)
    if ct == R.F32:
        return np.array(F32_BITS, dtype=np.uint32).view(np.float32)
    info = np.iinfo(dt)
    vals = [info.min, info.max, 0, 1, 2, 3, -1, info.max - 1, info.min + 1] + (_AROUND if dt.itemsize == 8 else [])
    mod = 1 << (8 * dt.itemsize)
    seen, out = set(), []
    for v in vals:
        v %= mod  # -1 of an unsigned type is its max; 2^64 - 1 of i64 is -1
        if v not in seen:
            seen.add(v)
            out.append(v)
    return np.array(out, dtype={1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[dt.itemsize]).view(dt)


def background(ct: int, n: int, which: int) -> np.ndarray:
    """n ordinary cells: finite, non-zero, normal, exact in every type; left and right backgrounds differ."""
    i = np.arange(n, dtype=np.int64)
    v = (i % 89) + 2 if which == 0 else (i % 83) + 3
    return v.astype(R.NP_DTYPES[ct])


def lattice(lt: int, rt: int):
    """The cross product, row-major: (l, r) of len(specials(lt)) * len(specials(rt)) cells."""
    a, b = specials(lt), specials(rt)
    return np.repeat(a, len(b)), np.tile(b, len(a))


A_LEN = 3 * 1536 + 1


def layout_a(lt: int, rt: int):
    l, r = lattice(lt, rt)
    assert len(l) <= A_LEN
    return np.resize(l, A_LEN), np.resize(r, A_LEN)


def nan_pairs(lt: int, rt: int) -> np.ndarray:
    """Indices into the lattice of the pairs with a NaN operand or, under any of the four ops, a NaN result."""
    l, r = lattice(lt, rt)
    a, b = R.widen_vec(l), R.widen_vec(r)
    hit = R.nan_vec(a) | R.nan_vec(b)
    for op in range(4):
        hit |= R.nan_vec(R.binop_vec(op, a, b)[0])
    return np.flatnonzero(hit)


def predicted_two_answer_cells(lt: int, rt: int) -> int:
    """From the value lists alone: the lattice cells with two allowed answers, over the four ops — ordered pairs of NaN patterns whose
    quieted widened bits differ, under `+` and under `*`.  36 for f64 x f64: 5 patterns, 25 pairs, 7 of them quieting to the same bits."""
    floats = (R.F32, R.F64)
    qa = [R.quiet(x) for x in R.widen_vec(specials(lt)).tolist() if R.is_nan(x)] if lt in floats else []
    qb = [R.quiet(x) for x in R.widen_vec(specials(rt)).tolist() if R.is_nan(x)] if rt in floats else []
    return 2 * sum(1 for x in qa for y in qb if x != y)


B_STRIDE = 1538


def layout_b(lt: int, rt: int):
    """(l, r, positions): pair j of the k nan_pairs at the even index (j + 1) * B_STRIDE and at the odd one (j + k + 1) * B_STRIDE + 1."""
    l, r = lattice(lt, rt)
    idx = nan_pairs(lt, rt)
    k = len(idx)
    pos = np.concatenate([np.arange(k) * B_STRIDE + B_STRIDE, (np.arange(k) + k) * B_STRIDE + B_STRIDE + 1])
    n = int(pos[-1]) + B_STRIDE + 1
    bl, br = background(lt, n, 0), background(rt, n, 1)
    bl[pos], br[pos] = np.concatenate([l[idx], l[idx]]), np.concatenate([r[idx], r[idx]])
    return bl, br, pos


def layout_b_single(ct: int):
    """(cells, positions): every special of one cell type planted alone as in layout B, for the buffer . scalar kernels."""
    sp = specials(ct)
    k = len(sp)
    pos = np.concatenate([np.arange(k) * B_STRIDE + B_STRIDE, (np.arange(k) + k) * B_STRIDE + B_STRIDE + 1])
    cells = background(ct, int(pos[-1]) + B_STRIDE + 1, 0)
    cells[pos] = np.concatenate([sp, sp])
    return cells, pos


C_SHAPES = [(1, 0), (2, 0), (3, 0), (5, 0), (7, 1)]   # (cells, offset into the allocation)


def layout_c(lt: int, rt: int):
    """One allocation per operand holding every small buffer back to back, and the list of `(start, n)` windows into it: for each pair
    p of nan_pairs buffers of 1, 2, 3 and 5 cells with p in every position in turn (the rest background), and a 7-cell buffer
    one cell into the allocation with p first and last.  Windows start at even cells but for the 7-cell ones, which start odd."""
    l, r = lattice(lt, rt)
    idx = nan_pairs(lt, rt)
    wins, ls, rs, at = [], [], [], 0
    for t, p in enumerate(idx):
        for n, off in C_SHAPES:
            n_alloc = n + off + ((n + off) & 1)
            bl, br = background(lt, n_alloc, 0), background(rt, n_alloc, 1)
            where = [off, off + n - 1] if off else [off + (t % n)]
            bl[where], br[where] = l[p], r[p]
            ls.append(bl)
            rs.append(br)
            wins.append((at + off, n))
            at += n_alloc
    if not wins:
        return background(lt, 2, 0), background(rt, 2, 1), []
    return np.concatenate(ls), np.concatenate(rs), wins


# ---------------------------------------------------------------- chains
T_F64 = [0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000001, 0xFFF4000000000002,
         0x3FF0000000000000, 0xFFEFFFFFFFFFFFFF, 0x0000000000000001, 0x5FF0000000000000]
T_F32 = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFF800002, 0x3F800000, 0xFF7FFFFF, 0x00000001, 0x7F000000]


def chain_values(ct: int) -> np.ndarray:
    """The sub-lattice T of a cell type: floats the ten values above, integers their own specials."""
    if ct == R.F64:
        return np.array(T_F64, dtype=np.uint64).view(np.float64)
    if ct == R.F32:
        return np.array(T_F32, dtype=np.uint32).view(np.float32)
    return specials(ct)


def chain_grid(cts):
    """The cross product of the chain values of the given cell types (T^3, T^4, or a mixed one), one array per operand."""
    vals = [chain_values(ct) for ct in cts]
    grids = np.meshgrid(*[np.arange(len(v)) for v in vals], indexing="ij")
    return [v[g.ravel()] for v, g in zip(vals, grids)]


# the contraction witness: a = k0 = 1 + 2^-30, k1 = -(1 + 2^-29): a * k0 = 1 + 2^-29 + 2^-60 rounds to 1 + 2^-29, so the two rounded
# steps of a * k0 + k1 give +0 where one fused multiply-add gives 2^-60; (a + b) * c is contracted no differently from a product.
WITNESS_A = 1.0 + 2.0 ** -30
WITNESS_K0 = 1.0 + 2.0 ** -30
WITNESS_K1 = -(1.0 + 2.0 ** -29)

# scalars that are special: the f64 list itself
SCALAR_BITS = F64_BITS

OPS = (R.ADD, R.SUB, R.MUL, R.DIV)
OP_TRIPLES = list(itertools.product(OPS, repeat=3))
OP_PAIRS = list(itertools.product(OPS, repeat=2))
FLOAT_PAIRS = [(R.F64, R.F64), (R.F32, R.F32), (R.F32, R.F64), (R.F64, R.F32), (R.F32, R.I16), (R.U8, R.F64), (R.I64, R.F32),
               (R.F64, R.U64)]

S, RG, K = (lambda k: k), (lambda k: 4 + k), (lambda k: 8 + k)
FORMULAS = {  # the ahead-of-time catalogue (csrc/ec_expr_fixed.hpp): streams, steps
    "NDVI": (2, [(R.SUB, S(0), S(1), 0), (R.ADD, S(0), S(1), 1), (R.DIV, RG(0), RG(1), 0)]),
    "add-mul": (3, [(R.ADD, S(0), S(1), 0), (R.MUL, RG(0), S(2), 0)]),
    "EVI": (3, [(R.SUB, S(0), S(1), 0), (R.MUL, RG(0), K(0), 0), (R.MUL, S(1), K(1), 1), (R.ADD, S(0), RG(1), 1),
                (R.MUL, S(2), K(2), 2), (R.SUB, RG(1), RG(2), 1), (R.ADD, RG(1), K(3), 1), (R.DIV, RG(0), RG(1), 0)]),
    "affine": (1, [(R.MUL, S(0), K(0), 0), (R.ADD, RG(0), K(1), 0)]),
}
BY_WIDTH = {1: R.U8, 2: R.I16, 4: R.F32, 8: R.F64}


# ---------------------------------------------------------------- the catalogue formulas
def _bits(x: float) -> int:
    return R.f64_bits(float(x))


EVI_ORDINARY = [_bits(x) for x in (2.5, 6.0, 7.5, 1.0)]
EVI_SPECIAL = [
    [0x7FF0000000000000, _bits(6.0), _bits(7.5), _bits(1.0)],
    [_bits(2.5), 0x7FF8000000000001, _bits(7.5), _bits(1.0)],
    [_bits(2.5), _bits(6.0), 0xFFF4000000000002, 0xFFF0000000000000],
    [0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFFFFFFFFFFFFFFF],
    [0x0000000000000001, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF, 0x5FF0000000000000],
    [0x8000000000000000, 0x0000000000000000, 0x8000000000000000, 0x0000000000000000],
]
# a * k0 + k1: two rounded steps give +0, one fused multiply-add does not.  f64 cells: the witness above; every other width: 3 * (1/3)
# rounds to 1, so 3 * (1/3) - 1 is +0 in two steps and -2^-54 fused.
AFFINE_WITNESS = {8: (WITNESS_A, _bits(WITNESS_K0), _bits(WITNESS_K1)), 4: (3.0, _bits(1 / 3), _bits(-1.0)),
                  2: (3, _bits(1 / 3), _bits(-1.0)), 1: (3, _bits(1 / 3), _bits(-1.0))}
AFFINE_ORDINARY = (_bits(0.0001), _bits(-273.15))
AFFINE_SCALARS = [(k0, k1) for k0 in T_F64 for k1 in T_F64]
# (a + b) * c: 1 + 2^-53 rounds to 1 (a tie, to even) and the product is c; distributed into a * c + b * c with one rounding the 2^-53
# survives and the sum rounds up.  Integer cells have no such triple: their sums and products below 2^53 are exact.
ADDMUL_WITNESS = {8: (1.0, 2.0 ** -53, 1.0 + 2.0 ** -52), 4: (1.0, 2.0 ** -53, 1.0 + 2.0 ** -23)}
FORMULA_LEN = 2 * 1536 + 3   # two tiles of the widest kernel, a ragged tile and an odd tail


def affine_stream(width: int) -> np.ndarray:
    ct = BY_WIDTH[width]
    v = np.concatenate([specials(ct), np.array([AFFINE_WITNESS[width][0]], dtype=R.NP_DTYPES[ct])])
    return np.resize(v, FORMULA_LEN)


def triple_streams(width: int):
    """T^3 of the width's cell type, with the (a + b) * c witness appended where the type has one; repeated to FORMULA_LEN cells."""
    ct = BY_WIDTH[width]
    g = chain_grid([ct] * 3)
    if width in ADDMUL_WITNESS:
        g = [np.concatenate([x, np.array([w], dtype=x.dtype)]) for x, w in zip(g, ADDMUL_WITNESS[width])]
    n = max(FORMULA_LEN, len(g[0]) | 1)
    return [np.resize(x, n) for x in g]
