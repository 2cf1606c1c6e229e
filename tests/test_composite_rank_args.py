"""Every refusal of ec_composite_rank (include/erased_cells.h), each decided before the library asks for a device: this file needs
none.  Only calls that are refused, or that have nothing to do, are made — the pointers are addresses that are never dereferenced.
Also here: that the symbols are exported, the spellings the Python mirror accepts, that the rank table r(c) of the per-cell header
equals the formula for every c (the stand-alone program host/test_composite_rank_cell.cpp checks the compiled table, plain and under
sanitizers), and that the group shape the tests restate (tests/composite_rank_ref.py) is the one the kernels are built with."""
import ctypes as C
import os
import re

import pytest

import composite_rank_ref as R
from host_program import run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED, ARG = 0, 2, 6
L0, L1, L2, DST, M0, M1, DMASK, AUX = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000   # never dereferenced


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    return ec


def arr(ptrs):
    return None if ptrs is None else (C.c_void_p * len(ptrs))(*ptrs)


def rank(L, t=1, layers=(L0, L1, L2), masks=None, k=None, n=1000, num=1, den=2, method=0, min_count=1, dst=DST, dmask=None, aux=None):
    k = len(layers) if k is None else k
    return L.ec_composite_rank(t, arr(layers), arr(masks), k, n, num, den, method, min_count, dst, dmask, aux, None)


SIXTY_FIVE = tuple(0x100000 + 0x1000 * i for i in range(65))

REFUSALS = [
    ("no layers", dict(layers=(L0,), k=0), "EC_COMPOSITE_MAX_LAYERS"),
    ("a negative layer count", dict(k=-1), "EC_COMPOSITE_MAX_LAYERS"),
    ("65 layers", dict(layers=SIXTY_FIVE), "EC_COMPOSITE_MAX_LAYERS"),
    ("den 0", dict(num=0, den=0), "EC_RANK_MAX_DEN"),
    ("den 65536", dict(num=1, den=65536), "EC_RANK_MAX_DEN"),
    ("num above den", dict(num=3, den=2), "num <= den"),
    ("num 2^32 - 1", dict(num=0xffffffff, den=65535), "num <= den"),
    ("method 2", dict(method=2), "ec_rank_method"),
    ("method -1", dict(method=-1), "ec_rank_method"),
    ("min_count 0", dict(min_count=0), "min_count"),
    ("min_count above the layer count", dict(min_count=4), "min_count"),
    ("min_count 2^32 - 1", dict(min_count=0xffffffff), "min_count"),
    ("null layers", dict(layers=None, k=3), "null pointer"),
    ("a null layer", dict(layers=(L0, None, L2)), "layer 1 is a null pointer"),
    ("null dst", dict(dst=None), "null pointer"),
    ("a mask and no dst_mask", dict(masks=(None, M0, None)), "needs dst_mask"),
    ("dst is a layer", dict(dst=L2), "dst is layer 2"),
    ("dst_mask is a mask", dict(masks=(M0, None, M1), dmask=M1), "mask of layer 2"),
    ("aux is a mask", dict(masks=(M0, None, M1), dmask=DMASK, aux=M0), "mask of layer 0"),
    ("dst_mask is dst", dict(dmask=DST), "dst_mask is dst"),
    ("aux is dst", dict(aux=DST), "aux is dst or dst_mask"),
    ("aux is dst_mask", dict(dmask=DMASK, aux=DMASK), "aux is dst or dst_mask"),
]


def test_every_refusal(ec):
    L = ec.lib()
    for what, kw, text in REFUSALS:
        for t in range(R.NT):
            assert L.ec_tune_set(b"no such knob", 0) == ARG   # another text in between: the next one is this call's own
            assert rank(L, t=t, **kw) == ARG, (what, t)
            msg = L.ec_last_error_string().decode()
            assert msg.startswith("ec_composite_rank: ") and text in msg, (what, msg)


def test_the_order_of_the_refusals(ec):
    """layer count, q, method, min_count, (dtype), null pointers, dst_mask, tiles, dst, the mask and aux outputs"""
    L = ec.lib()
    text = lambda: L.ec_last_error_string().decode()
    assert rank(L, k=0, den=0, method=7, min_count=0, t=10, dst=None) == ARG and "EC_COMPOSITE_MAX_LAYERS" in text()
    assert rank(L, den=0, method=7, min_count=0, t=10, dst=None) == ARG and "EC_RANK_MAX_DEN" in text()
    assert rank(L, num=3, den=2, method=7, min_count=0, t=10, dst=None) == ARG and "num <= den" in text()
    assert rank(L, method=7, min_count=0, t=10, dst=None) == ARG and "ec_rank_method" in text()
    assert rank(L, min_count=0, t=10, dst=None) == ARG and "min_count" in text()
    assert rank(L, t=10, dst=None) == UNSUPPORTED
    assert rank(L, dst=None, masks=(M0, M0, M0), n=1 << 62) == ARG and "null pointer" in text()
    assert rank(L, masks=(M0, M0, M0), n=1 << 62, dst=L0) == ARG and "needs dst_mask" in text()
    assert rank(L, n=1 << 62, dst=L0) == ARG and "2^31 - 1 tiles" in text()
    assert rank(L, dst=L0, masks=(M0, M0, M0), dmask=M0) == ARG and "dst is layer 0" in text()
    assert rank(L, masks=(M0, M0, M0), dmask=M0, aux=DST) == ARG and "mask of layer 0" in text()


def test_more_than_2_31_minus_1_tiles(ec):
    L = ec.lib()
    for t in range(R.NT):
        for k in (1, 3, 16, 64):
            layers = SIXTY_FIVE[:k]
            most = (2 ** 31 - 2) * R.tile_cells(t, k)              # this many cells are certainly within 2^31 - 1 tiles
            assert rank(L, t=t, layers=layers, n=(2 ** 31) * R.tile_cells(t, k)) == ARG, (t, k)
            assert "2^31 - 1 tiles" in L.ec_last_error_string().decode()
            # the call is refused by the next check (nothing may be launched from here)
            assert rank(L, t=t, layers=layers, n=most, dst=layers[0]) == ARG and "dst is layer 0" in L.ec_last_error_string().decode(), (t, k)


def test_a_bad_dtype_is_unsupported_type(ec):
    L = ec.lib()
    for bad in (10, 255):
        assert rank(L, t=bad) == UNSUPPORTED
        assert L.ec_last_error_string().decode() == f"ec_composite_rank: bad dtype {bad}"
        assert rank(L, t=bad, n=0) == UNSUPPORTED   # also for an empty stack


def test_an_empty_stack_is_ok_and_launches_nothing(ec):
    L = ec.lib()
    for t in range(R.NT):
        for num, den, method in R.TRIPLES:
            assert rank(L, t=t, n=0, num=num, den=den, method=method) == OK
        assert rank(L, t=t, n=0, layers=None, k=3, dst=None) == OK   # the form the sharded entry point checks with
    assert rank(L, n=0, min_count=4) == ARG    # the checks come first
    assert rank(L, n=0, num=2, den=1) == ARG and rank(L, n=0, method=2) == ARG


def test_symbols_and_the_sharded_form(ec):
    L = ec.lib()
    raw = C.CDLL(ec._ffi.SO_PATH)
    for name in ("ec_composite_rank", "ec_sharded_composite_rank"):
        assert hasattr(raw, name) and name in ec._ffi.SIGNATURES
    assert L.ec_abi_version() == 1
    assert L.ec_sharded_composite_rank(None, 1, None, None, 1, None, 1, 2, 0, 1, None, None, None) == ARG


def test_the_python_spellings(ec):
    from erased_cells_hip import buffer as B
    E = ec._ffi
    assert (E.EC_RANK_LOWER, E.EC_RANK_UPPER, E.EC_RANK_MAX_DEN) == (R.LOWER, R.UPPER, R.MAX_DEN) == (0, 1, 65535)
    assert ec.RANK_METHODS == dict(zip(R.METHOD_NAMES, R.METHODS))
    assert B._rank_args((1, 2), "lower") == (1, 2, 0) and B._rank_args([9, 10], "upper") == (9, 10, 1) and B._rank_args((0, 1), 1) == (0, 1, 1)
    assert B._rank_args(0, "lower") == (0, 1, 0) and B._rank_args(1, "upper") == (1, 1, 1) and B._rank_args((65535, 65535), 0) == (65535, 65535, 0)
    for bad in (0.5, (1, 0), (2, 1), (-1, 2), (1, 65536), (1,), (1, 2, 3), "1/2", None, True, (0.5, 1), 2):
        with pytest.raises(ec.EcError, match="q "):
            B._rank_args(bad, "lower")
    for bad in ("median", "Lower", 2, -1, True, 1.0, None):
        with pytest.raises(ec.EcError, match="method"):
            B._rank_args((1, 2), bad)
    # ec.composite and its spellings stay as they were
    assert ec.COMPOSITE_OPS == {"first": 0, "last": 1, "min": 2, "max": 3, "sum": 4, "mean": 5}
    with pytest.raises(ec.EcError):
        B._composite_op("median")
    from erased_cells_hip.sharded import ShardGroup
    assert callable(ec.composite_rank) and callable(ec.composite_median) and callable(ShardGroup.composite_rank)


def _plan_header():
    return open(os.path.join(ROOT, "erased-cells_amd", "csrc", "ec_composite_rank_cell.hpp")).read()


def test_the_rank_table_of_the_plan_header_is_the_formula():
    """rank_position is restated from its text and evaluated in Python for every c: it must be R.position, which
    test_composite_rank_ref.py holds to the header's inequalities"""
    text = _plan_header()
    m = re.search(r"constexpr uint32_t rank_position\(uint32_t num, uint32_t den, int method, uint32_t c\) \{\s*return method == kRankUpper \? "
                  r"\(num \* \(c - 1\) \+ den - 1\) / den : \(num \* \(c - 1\)\) / den;\s*\}", text)
    assert m, "rank_position changed its form: restate it here"
    assert re.search(r"for \(uint32_t c = 1; c <= uint32_t\(kCompositeMaxLayers\); \+\+c\) t\.r\[c\] = rank_position\(num, den, method, c\);", text)
    assert re.search(r"kRankLower = 0, kRankUpper = 1;", text) and re.search(r"kRankMaxDen = 65535;", text)
    wrap = lambda x: x & 0xffffffff                                  # the header computes in uint32_t
    for num, den, method in R.TRIPLES:
        for c in range(1, 65):
            r = wrap(wrap(num * (c - 1)) + den - 1) // den if method == R.UPPER else wrap(num * (c - 1)) // den
            assert r == R.position(num, den, method, c) and r <= c - 1 <= 63 and num * (c - 1) + den - 1 < 2 ** 32, (num, den, method, c)


def test_the_shape_the_tests_restate_is_the_kernels():
    text = open(os.path.join(ROOT, "erased-cells_amd", "csrc", "ec_composite_rank_kernels.hpp")).read()
    assert re.search(r"constexpr int rank_word_regs\(size_t cell_bytes\) \{ return cell_bytes <= 2 \? 1 : cell_bytes == 4 \? 2 : 3; \}", text)
    g = re.search(r"int g = 16 / int\(cell_bytes\);\s*while \(g > 1 && g \* kb \* rank_word_regs\(cell_bytes\) > (\d+)\) g /= 2;\s*"
                  r"return cell_bytes <= 2 && kb == (\d+) \? (\d+) : g;", text)
    assert g, "rank_group changed its form: restate it in tests/composite_rank_ref.py"
    budget, at_bucket, cells = (int(x) for x in g.groups())
    for t in range(R.NT):
        for k in R.KS:
            size = R.NP[t].itemsize
            want = 16 // size
            while want > 1 and want * R.bucket(k) * (1 if size <= 2 else 2 if size == 4 else 3) > budget:
                want //= 2
            if size <= 2 and R.bucket(k) == at_bucket:
                want = cells
            assert R.group_cells(t, k) == want, (t, k)
    header = open(os.path.join(ROOT, "include", "erased_cells.h")).read()
    assert re.search(r"EC_RANK_LOWER\s*=\s*0\b", header) and re.search(r"EC_RANK_UPPER\s*=\s*1\b", header) and re.search(r"EC_RANK_MAX_DEN\s*=\s*65535\b", header)
    i = header.index("ec_status ec_composite_rank(")
    assert re.search(r"src/[a-z_/]+\.rs:\d+", header[i - 3500:i]), "ec_composite_rank's comment cites the reference"
    assert header.index("ec_status ec_sharded_composite(") < i < header.index("ec_status ec_sharded_composite_rank(")
    assert set(R.KS) >= {b + d for b in (1, 2, 4, 8, 16, 32) for d in (0, 1)} | {63, 64}     # both sides of every bucket edge


@pytest.mark.parametrize("target", ["test_composite_rank_cell", "test_composite_rank_cell_san"])
def test_the_cell_header_alone_and_under_sanitizers(target):
    """erased-cells_amd/host/test_composite_rank_cell.cpp: the per-cell selection of csrc/ec_composite_rank_cell.hpp for every type and
    every K against std::sort of (key, k) pairs — a stand-alone program, built plainly and with -fsanitize=address,undefined"""
    run_host_program(target)
