"""Which kernel header may include which, read off the `#include` lines of csrc/*.hpp — no device, nothing compiled.

What every tiled kernel shares (the workgroup, the tile map, the 16-byte slot) lives in ec_tile.hpp, so that a family's kernels
compile against that header and not against another family's: above all not against the widening binop's hot path."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "erased-cells_amd", "csrc")
INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)
# what ec_binop_kernels.hpp keeps for itself: its wave count, the LDS staging, the mask AND, its tile bodies and kernels
BINOP_OWN = re.compile(r"\b(kWavesPerBlock|Staged|kLdsChunks|kLdsWaveCells|mask_and_body\s*\(|binop_\w+_(tile|body)|k_(masked_)?binop\w*)\b")


def headers():
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hpp"))):
        text = open(path).read()
        code = re.sub(r"//[^\n]*", "", text)
        out[os.path.basename(path)] = (set(INCLUDE.findall(text)), code)
    return out


def test_the_shared_header_holds_what_the_families_share():
    tile = open(os.path.join(CSRC, "ec_tile.hpp")).read()
    for name in ("kBlock", "kWave", "load_vec", "two_front_tile", "first_group", "u32x4", "width_cell", "slot_put", "slot_get", "slot_store"):
        assert re.search(r"\b%s\b" % name, tile), name
    assert INCLUDE.findall(tile) == ["ec_device.hpp"], "ec_tile.hpp stands on ec_device.hpp alone"


def test_only_the_binop_units_compile_against_the_binop_kernels():
    h = headers()
    assert "ec_binop_kernels.hpp" in h["ec_binop_tu.hpp"][0]
    for name, (includes, code) in h.items():
        if name == "ec_binop_tu.hpp" or "ec_binop_kernels.hpp" not in includes:
            continue
        assert BINOP_OWN.search(code), f"{name} includes ec_binop_kernels.hpp and uses nothing of the binop's own: include ec_tile.hpp"


def test_the_refusal_header_stands_alone():
    text = open(os.path.join(CSRC, "ec_refusal.hpp")).read()
    assert INCLUDE.findall(text) == [], "ec_refusal.hpp includes no header of the project"
    assert sorted(re.findall(r"^\s*#\s*include\s+<([^>]+)>", text, re.M)) == ["stddef.h", "stdint.h"]


# an interval test of one's own: a predicate over two (pointer, byte count) pairs, or the comparison of two starts with two ends
INTERVAL_TEST = re.compile(r"\bbool\s+\w+\s*\(\s*const\s+void\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*const\s+void\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*\)"
                           r"|\b\w+\s*<\s*\w+\s*\+\s*\w+\s*&&\s*\w+\s*<\s*\w+\s*\+\s*\w+")


def test_the_interval_test_is_defined_once():
    assert len(INTERVAL_TEST.findall(re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "ec_refusal.hpp")).read()))) == 1
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hpp")) + glob.glob(os.path.join(CSRC, "*.hip"))):
        if os.path.basename(path) == "ec_refusal.hpp":
            continue
        found = INTERVAL_TEST.findall(re.sub(r"//[^\n]*", "", open(path).read()))
        assert not found, f"{os.path.basename(path)} tests intervals for itself ({found[0]}): use ecv::overlap of ec_refusal.hpp"


def test_the_focal_kernels_do_not_include_the_window_kernels():
    includes, _ = headers()["ec_focal_kernels.hpp"]
    assert "ec_window_kernels.hpp" not in includes and "ec_tile.hpp" in includes
