"""Every refusal of ec_regions (include/erased_cells.h) in the stated order, each with its own text and each decided before the
library asks for a device: this file needs none.  ONLY calls that are refused are made — the pointers are addresses that are never
dereferenced, and a call that passed the checks would launch on them where a device is bound.  Also here:
ec_regions_workspace_bytes for legal and refused shapes, the spellings the Python mirror accepts, that the constants the tests restate
(tests/regions_cases.py) are the ones the kernels are built with, and the per-cell header alone as a stand-alone program, built plainly,
with the address and undefined-behaviour sanitizers, and with the thread sanitizer for the seam unions under threads."""
import inspect
import os
import re

import pytest

import regions_cases as K
from host_program import run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED, ARG = 0, 2, 6
U8, U16, I32, F64 = 0, 1, 6, 9
SRC, SMASK, DST, DMASK, KDEV, WS = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000   # never dereferenced; 256 MiB apart
MAX_SIDE = 32768
N = 100 * 50


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    return ec


def regions(L, t=U16, src=SRC, smask=SMASK, cols=100, rows=50, connectivity=4, numbering=K.DENSE, min_cells=0, dst=DST, dmask=DMASK, k=KDEV, ws=WS):
    return L.ec_regions(t, src, smask, cols, rows, connectivity, numbering, min_cells, dst, dmask, k, ws, None)


def ws_bytes(cols, rows):
    """the header's layout, restated: a parent and a size per cell (u32 each), then one u32 per block of SCAN cells, each padded to 16 bytes"""
    pad = lambda b: (b + 15) // 16 * 16
    n = cols * rows
    return 2 * pad(4 * n) + pad(4 * -(-n // K.SCAN))


# in the order of the header: (what, arguments, status, text)
REFUSALS = [
    ("cols 0", dict(cols=0), ARG, "EC_REGIONS_MAX_SIDE"),
    ("rows 0", dict(rows=0), ARG, "EC_REGIONS_MAX_SIDE"),
    ("cols above the limit", dict(cols=MAX_SIDE + 1), ARG, "EC_REGIONS_MAX_SIDE"),
    ("rows above the limit", dict(rows=MAX_SIDE + 1), ARG, "EC_REGIONS_MAX_SIDE"),
    ("cols 2^32 + 1", dict(cols=(1 << 32) + 1), ARG, "EC_REGIONS_MAX_SIDE"),
    ("rows 2^63", dict(rows=1 << 63), ARG, "EC_REGIONS_MAX_SIDE"),
    ("t 10 is no cell type", dict(t=10), UNSUPPORTED, "bad cell type"),
    ("t 255 is no cell type", dict(t=255), UNSUPPORTED, "bad cell type"),
    ("connectivity 0", dict(connectivity=0), ARG, "neither 4 nor 8"),
    ("connectivity 6", dict(connectivity=6), ARG, "neither 4 nor 8"),
    ("connectivity -4", dict(connectivity=-4), ARG, "neither 4 nor 8"),
    ("numbering 2", dict(numbering=2), ARG, "neither EC_REGIONS_ROOT nor EC_REGIONS_DENSE"),
    ("numbering -1", dict(numbering=-1), ARG, "neither EC_REGIONS_ROOT nor EC_REGIONS_DENSE"),
    ("no input at all", dict(src=None, smask=None), ARG, "src and src_mask are both NULL"),
    ("no output at all", dict(dst=None, dmask=None, k=None), ARG, "all NULL"),
    ("a u16 src at 1 mod 2", dict(src=SRC + 1), ARG, "src is not aligned"),
    ("an f64 src at 4 mod 8", dict(t=F64, src=SRC + 4), ARG, "src is not aligned"),
    ("dst at 2 mod 4", dict(dst=DST + 2), ARG, "dst is not aligned"),
    ("dst at 1 mod 4", dict(dst=DST + 1), ARG, "dst is not aligned"),
    ("n_regions at 4 mod 8", dict(k=KDEV + 4), ARG, "n_regions is not aligned"),
    ("the workspace at 8 mod 16", dict(ws=WS + 8), ARG, "workspace is not aligned"),
    ("dst == src", dict(src=DST), ARG, "dst overlaps src ("),
    ("dst's last cell on src's first byte", dict(src=DST + 4 * N - 2), ARG, "dst overlaps src ("),
    ("dst on src_mask", dict(smask=DST + 4 * N - 1), ARG, "dst overlaps src_mask"),
    ("dst_mask == src_mask", dict(dmask=SMASK), ARG, "dst_mask overlaps src_mask"),
    ("dst_mask's end on src's start", dict(src=DMASK + N - 2, dmask=DMASK + 1), ARG, "dst_mask overlaps src ("),
    ("n_regions inside src", dict(k=SRC + 8), ARG, "n_regions overlaps src ("),
    ("n_regions inside src_mask", dict(k=SMASK + N - 8), ARG, "n_regions overlaps src_mask"),
    ("the workspace's last byte on src's first", dict(src=WS + ws_bytes(100, 50) - 2), ARG, "workspace overlaps src ("),
    ("the workspace's last byte on src_mask's first", dict(smask=WS + ws_bytes(100, 50) - 1), ARG, "workspace overlaps src_mask"),
    ("dst_mask inside dst", dict(dmask=DST + 8), ARG, "dst_mask overlaps dst"),
    ("n_regions inside dst", dict(k=DST + 16), ARG, "n_regions overlaps dst ("),
    ("n_regions inside dst_mask", dict(k=DMASK + 16), ARG, "n_regions overlaps dst_mask"),
    ("the workspace on dst", dict(ws=DST + 16), ARG, "workspace overlaps dst ("),
    ("the workspace's last byte on dst_mask's first", dict(dmask=WS + ws_bytes(100, 50) - 1), ARG, "workspace overlaps dst_mask"),
    ("n_regions inside the workspace", dict(k=WS + 64), ARG, "workspace overlaps n_regions"),
]


def test_every_refusal_with_its_text(ec):
    L = ec.lib()
    for what, kw, status, text in REFUSALS:
        assert L.ec_tune_set(b"no such knob", 0) == ARG   # another text in between: the next one is this call's own
        assert regions(L, **kw) == status, what
        msg = L.ec_last_error_string().decode()
        assert msg.startswith("ec_regions: ") and text in msg, (what, msg)
    assert len({t for _, _, _, t in REFUSALS}) == 24   # eight steps; the misalignments and the overlaps name their argument or pair
    # the mask form: t is not looked at without src, and the refusals behind it still hold
    assert regions(L, t=77, src=None, connectivity=5) == ARG and "neither 4 nor 8" in L.ec_last_error_string().decode()
    assert regions(L, t=77, src=None, dmask=SMASK) == ARG and "dst_mask overlaps src_mask" in L.ec_last_error_string().decode()


# one representative of each step of the order, first to last
ORDER = [("EC_REGIONS_MAX_SIDE", dict(cols=0)), ("bad cell type", dict(t=99)), ("neither 4 nor 8", dict(connectivity=5)),
         ("neither EC_REGIONS_ROOT", dict(numbering=7)), ("both NULL", dict(src=None, smask=None)), ("all NULL", dict(dst=None, dmask=None, k=None)),
         ("not aligned", dict(ws=WS + 4)), ("overlaps", dict(dmask=SMASK))]


def test_the_order_of_the_refusals(ec):
    """with the mistakes of steps i, i + 1, .. all made at once, the text is step i's.  (A bad cell type is only seen with a src, so the
    "no input" mistake of step 5 leaves src in place and takes the mask away while a bad type is being shown.)"""
    L = ec.lib()
    for i, (text, _) in enumerate(ORDER):
        kw = {}
        for _, later in reversed(ORDER[i:]):
            kw.update(later)            # the earliest step's arguments win
        if i <= 1:
            kw["src"] = SRC
        status = regions(L, **kw)
        msg = L.ec_last_error_string().decode()
        assert status == (UNSUPPORTED if i == 1 else ARG) and msg.startswith("ec_regions: ") and text in msg, (text, msg, kw)


def test_workspace_bytes(ec):
    L = ec.lib()
    for cols, rows in K.SHAPES + [(MAX_SIDE, MAX_SIDE), (4096, 4096), (16384, 2048), (3, 5)]:
        got = L.ec_regions_workspace_bytes(cols, rows)
        assert got == ws_bytes(cols, rows) and got % 16 == 0 and got >= 8 * cols * rows, (cols, rows)
    for cols, rows in ((0, 0), (0, 5), (5, 0), (MAX_SIDE + 1, 1), (1, MAX_SIDE + 1), (1 << 40, 1), (1, 1 << 63)):
        assert L.ec_regions_workspace_bytes(cols, rows) == 0, (cols, rows)


def test_the_python_spellings(ec):
    from erased_cells_hip import buffer as B
    E = ec._ffi
    assert (E.EC_REGIONS_MAX_SIDE, E.EC_REGIONS_ROOT, E.EC_REGIONS_DENSE) == (MAX_SIDE, K.ROOT, K.DENSE) == (32768, 0, 1)
    for cls in (ec.CellBuffer, ec.MaskedCellBuffer, ec.Mask):
        sig = inspect.signature(cls.regions).parameters
        assert list(sig)[1:] == ["cols", "connectivity", "min_cells", "numbering"]
        assert (sig["connectivity"].default, sig["min_cells"].default, sig["numbering"].default) == (4, 0, "dense")
    for cls in (ec.MaskedCellBuffer, ec.Mask):
        sig = inspect.signature(cls.sieve).parameters
        assert list(sig)[1:] == ["cols", "min_cells", "connectivity"] and sig["connectivity"].default == 4
    assert not hasattr(ec.CellBuffer, "sieve")     # nothing to invalidate without a mask to carry it: MaskedCellBuffer.sieve
    # refused in Python, before any buffer is made: a numbering that is no name, a min_cells that is no count
    for bad in ("sparse", "", "Dense"):
        with pytest.raises(ec.EcError, match="neither 'root' nor 'dense'"):
            B._regions(None, None, 0, 0, 4, 0, bad, True)
    for bad in (-1, 1.5, 1 << 64, True):
        with pytest.raises(ec.EcError, match="min_cells"):
            B._regions(None, None, 0, 0, 4, bad, "dense", True)


def test_the_constants_the_tests_restate_are_the_kernels(ec):
    csrc = os.path.join(ROOT, "erased-cells_amd", "csrc")
    text = open(os.path.join(csrc, "ec_regions_cell.hpp")).read()

    def const(name):
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(0x[0-9A-Fa-f]+|\d+)u?\s*;", text)
        assert m, name
        return int(m.group(1), 0)

    assert (const("kRegTileW"), const("kRegTileH"), const("kRegScanCells"), const("kRegMaxSide")) == (K.TW, K.TH, K.SCAN, MAX_SIDE)
    assert const("kRegThreads") == 256 and const("kRegSeamLanes") == 64 >= K.TW + K.TH - 1
    assert K.TW * K.TH * 4 <= 64 * 1024 and K.TW * K.TH % const("kRegThreads") == 0 and K.SCAN % const("kRegThreads") == 0
    kernels = open(os.path.join(csrc, "ec_regions_kernels.hpp")).read()
    assert '#include "ec_regions_cell.hpp"' in kernels and "__launch_bounds__(kRegSeamLanes)" in kernels
    # every access to parent[] in the seam kernel goes through the agent-scope words
    seams = kernels[kernels.index("void k_regions_seams"):kernels.index("void k_regions_flatten")]
    assert "RegAgentWords words{parent}" in seams and "parent[" not in seams and "__syncthreads" not in seams
    agent = kernels[kernels.index("struct RegAgentWords"):kernels.index("struct RegPlainWords")]
    assert agent.count("__HIP_MEMORY_SCOPE_AGENT") == 2 and "__hip_atomic_load" in agent and "__hip_atomic_fetch_min" in agent
    header = open(os.path.join(ROOT, "include", "erased_cells.h")).read()
    assert re.search(r"EC_REGIONS_MAX_SIDE\s*=\s*32768\b", header) and re.search(r"EC_REGIONS_ROOT\s*=\s*0\s*,\s*EC_REGIONS_DENSE\s*=\s*1", header)
    # the shapes of the GPU tests are around these constants
    assert {K.TW - 1, K.TW, K.TW + 1, 2 * K.TW + 1} <= set(K.SIZES_W) and {K.TH - 1, K.TH, K.TH + 1, 2 * K.TH + 1} <= set(K.SIZES_H)
    assert any(c * r > 2 * K.SCAN for c, r in K.SMALL)        # roots in more than two blocks of the scan


@pytest.mark.parametrize("target,args", [("test_regions_cell", []), ("test_regions_cell_san", []), ("test_regions_cell_tsan", ["threads"])])
def test_the_cell_header_alone_and_under_sanitizers(target, args):
    """erased-cells_amd/host/test_regions_cell.cpp: the phases of csrc/ec_regions_cell.hpp alone against a flood fill over every mask up
    to 4 x 4 and random rasters up to 40 x 40, with stale loads, and the seam unions from up to 16 threads — a stand-alone program, built
    plainly, with -fsanitize=address,undefined and, for the threads, with -fsanitize=thread"""
    run_host_program(target, *args, timeout=600, passed="checks passed, 0 failed")
