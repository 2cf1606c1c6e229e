"""Every refusal of ec_distance (include/erased_cells.h) in the stated order, each with its own text and each decided before the
library asks for a device: this file needs none.  ONLY calls that are refused are made — the pointers are addresses that are never
dereferenced, and a call that passed the checks would launch on them where a device is bound.  Also here:
ec_distance_workspace_bytes for legal and refused shapes, the spellings the Python mirror accepts, that the constants the tests restate (tests/distance_cases.py) are the ones the kernels are built with, and the line scans' header alone as a
stand-alone program, built plainly and with the address and undefined-behaviour sanitizers."""
import fractions
import inspect
import os
import re

import pytest

import distance_cases as K
from host_program import run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED, ARG = 0, 2, 6
U32, F64 = 2, 9
MASK, DST, DMASK, WS = 0x10000000, 0x20000000, 0x30000000, 0x40000000   # never dereferenced; 256 MiB apart
MAX_SIDE = 32768


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    return ec


def distance(L, mask=MASK, cols=100, rows=50, max_sq=K.UNLIMITED, out_type=F64, dst=DST, dmask=DMASK, ws=WS):
    return L.ec_distance(mask, cols, rows, max_sq, out_type, dst, dmask, ws, None)


def ws_bytes(cols, rows):
    """the header's layout, restated: g (u16 a cell), then the two stacks (u16 an entry, cols entries a row, rows rounded up to whole
    waves), each padded to 16 bytes"""
    pad = lambda b: (b + 15) // 16 * 16
    stack = pad(-(-rows // K.W) * K.W * cols * 2)
    return pad(cols * rows * 2) + 2 * stack


# in the order of the header: (what, arguments, status, text)
REFUSALS = [
    ("cols 0", dict(cols=0), ARG, "EC_DISTANCE_MAX_SIDE"),
    ("rows 0", dict(rows=0), ARG, "EC_DISTANCE_MAX_SIDE"),
    ("cols above the limit", dict(cols=MAX_SIDE + 1), ARG, "EC_DISTANCE_MAX_SIDE"),
    ("rows above the limit", dict(rows=MAX_SIDE + 1), ARG, "EC_DISTANCE_MAX_SIDE"),
    ("cols 2^32 + 1", dict(cols=(1 << 32) + 1), ARG, "EC_DISTANCE_MAX_SIDE"),
    ("rows 2^63", dict(rows=1 << 63), ARG, "EC_DISTANCE_MAX_SIDE"),
    ("out_type 10 is no cell type", dict(out_type=10), UNSUPPORTED, "bad out_type"),
    ("out_type 255 is no cell type", dict(out_type=255), UNSUPPORTED, "bad out_type"),
    ("out_type u8", dict(out_type=0), ARG, "neither EC_U32 nor EC_F64"),
    ("out_type f32", dict(out_type=8), ARG, "neither EC_U32 nor EC_F64"),
    ("out_type u64", dict(out_type=3), ARG, "neither EC_U32 nor EC_F64"),
    ("null mask", dict(mask=None), ARG, "null mask"),
    ("no output at all", dict(dst=None, dmask=None), ARG, "both NULL"),
    ("an f64 dst at 4 mod 8", dict(dst=DST + 4), ARG, "not aligned"),
    ("a u32 dst at 2 mod 4", dict(out_type=U32, dst=DST + 2), ARG, "not aligned"),
    ("a u32 dst at 1 mod 4", dict(out_type=U32, dst=DST + 1), ARG, "not aligned"),
    ("dst == mask", dict(mask=DST), ARG, "dst overlaps the mask"),
    ("dst's last cell on the mask's first byte", dict(mask=DST + 100 * 50 * 8 - 1), ARG, "dst overlaps the mask"),
    ("dst_mask == mask", dict(dmask=MASK), ARG, "dst_mask overlaps the mask"),
    ("dst_mask's last byte on the mask's first", dict(dmask=MASK - 100 * 50 + 1), ARG, "dst_mask overlaps the mask"),
    ("the workspace's last byte on the mask's first", dict(mask=WS + ws_bytes(100, 50) - 1), ARG, "workspace overlaps the mask"),
    ("dst_mask inside dst", dict(dmask=DST + 8), ARG, "dst_mask overlaps dst"),
    ("the workspace on dst", dict(ws=DST + 16), ARG, "workspace overlaps dst"),
    ("the workspace's last byte on dst_mask's first", dict(dmask=WS + ws_bytes(100, 50) - 1), ARG, "workspace overlaps dst_mask"),
]


def test_every_refusal_with_its_text(ec):
    L = ec.lib()
    for what, kw, status, text in REFUSALS:
        assert L.ec_tune_set(b"no such knob", 0) == ARG   # another text in between: the next one is this call's own
        assert distance(L, **kw) == status, what
        msg = L.ec_last_error_string().decode()
        assert msg.startswith("ec_distance: ") and text in msg, (what, msg)
    texts = {t for _, _, _, t in REFUSALS}
    assert len(texts) == 12   # six steps; the overlaps name their pair


# one representative of each step of the order, first to last
ORDER = [("EC_DISTANCE_MAX_SIDE", dict(cols=0)), ("neither EC_U32 nor EC_F64", dict(out_type=1)), ("null mask", dict(mask=None)),
         ("both NULL", dict(dst=None, dmask=None)), ("not aligned", dict(dst=DST + 4)), ("overlaps", dict(ws=DST + 4 + 16))]


def test_the_order_of_the_refusals(ec):
    """with the mistakes of steps i, i + 1, .. all made at once, the text is step i's.  (A call cannot make every mistake at once — dst is
    null or misaligned — so where two steps want the same argument the later one gives way.)"""
    L = ec.lib()
    for i, (text, _) in enumerate(ORDER):
        kw = {}
        for _, later in reversed(ORDER[i:]):
            kw.update(later)            # the earliest step's arguments win
        assert distance(L, **kw) == ARG
        msg = L.ec_last_error_string().decode()
        assert msg.startswith("ec_distance: ") and text in msg, (text, msg, kw)
    # a value that is no cell type at all is EC_ERR_UNSUPPORTED_TYPE, behind the shape and before the pointers
    assert distance(L, out_type=77, mask=None) == UNSUPPORTED and distance(L, out_type=77, cols=0) == ARG


def test_workspace_bytes(ec):
    L = ec.lib()
    for cols, rows in K.SHAPES + [(MAX_SIDE, MAX_SIDE), (4096, 4096), (16384, 2048), (1, MAX_SIDE), (MAX_SIDE, 1)]:
        got = L.ec_distance_workspace_bytes(cols, rows)
        assert got == ws_bytes(cols, rows) and got % 16 == 0 and got >= 6 * cols * rows, (cols, rows)
    for cols, rows in ((0, 0), (0, 5), (5, 0), (MAX_SIDE + 1, 1), (1, MAX_SIDE + 1), (1 << 40, 1), (1, 1 << 63)):
        assert L.ec_distance_workspace_bytes(cols, rows) == 0, (cols, rows)


def test_the_python_spellings(ec):
    from erased_cells_hip import buffer as B
    assert ec._ffi.EC_DISTANCE_MAX_SIDE == MAX_SIDE and ec._ffi.EC_DISTANCE_UNLIMITED == K.UNLIMITED == 0xFFFFFFFF
    assert callable(ec.Mask.distance) and callable(ec.Mask.within)
    sig = inspect.signature(ec.Mask.distance).parameters
    assert list(sig)[1:] == ["cols", "max_distance", "squared"] and (sig["max_distance"].default, sig["squared"].default) == (None, False)
    assert list(inspect.signature(ec.Mask.within).parameters)[1:] == ["cols", "distance"]
    # max_sq = floor(max_distance^2), exactly
    F = fractions.Fraction
    assert B._max_sq(None) == K.UNLIMITED and B._max_sq(float("inf")) == K.UNLIMITED
    assert (B._max_sq(0), B._max_sq(1), B._max_sq(50), B._max_sq(1.5), B._max_sq(F(3, 2)), B._max_sq(F(7, 5))) == (0, 1, 2500, 2, 2, 1)
    assert B._max_sq(2 ** 0.5) == 2 and B._max_sq(float.fromhex("0x1.6a09e667f3bccp+0")) == 1   # the double above the root of 2, and the one below
    assert B._max_sq(F(141421356237309504880, 10 ** 20)) == 1 and B._max_sq(F(141421356237309504881, 10 ** 20)) == 2
    assert B._max_sq(65535) == 65535 ** 2 and B._max_sq(65536) == K.UNLIMITED and B._max_sq(10 ** 30) == K.UNLIMITED
    assert B._max_sq(F(65535 * 2 + 1, 2)) == 65535 ** 2 + 65535
    for bad in (-1, -0.5, float("nan"), F(-1, 3), True):
        with pytest.raises(ec.EcError, match="greatest distance"):
            B._max_sq(bad)


def test_the_constants_the_tests_restate_are_the_kernels(ec):
    csrc = os.path.join(ROOT, "erased-cells_amd", "csrc")
    text = open(os.path.join(csrc, "ec_distance_line.hpp")).read()

    def const(name):
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(0x[0-9A-Fa-f]+|\d+)u?\s*;", text)
        assert m, name
        return int(m.group(1), 0)

    assert (const("kDistLines"), const("kDistTile"), const("kDistChunk"), const("kDistInf")) == (K.W, K.T, K.CHUNK, K.INF)
    assert const("kDistMaxSide") == MAX_SIDE and const("kDistNone") == K.UNLIMITED
    assert re.search(r"kDistGPitch\s*=\s*kDistTile\s*\+\s*2\s*;", text) and re.search(r"kDistDPitch\s*=\s*kDistTile\s*\+\s*1\s*;", text)
    assert (K.T + 2) % 4 == 2 and (K.T + 1) % 2 == 1          # 33 and 65 dwords a row: odd, so 32 lanes a column-wise access fall on 32 banks
    assert K.W * (K.T + 2) * 2 + K.W * (K.T + 1) * 4 <= 32 * 1024   # both tiles of a workgroup
    kernels = open(os.path.join(csrc, "ec_distance_kernels.hpp")).read()
    assert '#include "ec_distance_line.hpp"' in kernels and "__launch_bounds__(kDistLines)" in kernels
    assert "atomic" not in kernels.replace("No atomics", "") and "asm" not in kernels.replace("no inline assembly", "")
    header = open(os.path.join(ROOT, "include", "erased_cells.h")).read()
    assert re.search(r"EC_DISTANCE_MAX_SIDE\s*=\s*32768\b", header) and re.search(r"#define\s+EC_DISTANCE_UNLIMITED\s+0xFFFFFFFFu", header)
    # the shapes of the GPU tests are around these constants
    assert {K.W - 1, K.W, K.W + 1, K.T - 1, K.T, K.T + 1, 2 * K.T + 1} <= set(K.SIZES)


@pytest.mark.parametrize("target", ["test_distance_line", "test_distance_line_san"])
def test_the_line_header_alone_and_under_sanitizers(target):
    """erased-cells_amd/host/test_distance_line.cpp: the column sweeps and the row scans of csrc/ec_distance_line.hpp alone against
    brute force over every mask up to 4 x 4 and random ones up to 40 x 40 — a stand-alone program, built plainly and with
    -fsanitize=address,undefined"""
    run_host_program(target)
