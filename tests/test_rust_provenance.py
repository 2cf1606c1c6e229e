"""Provenance of the Rust crate (erased-cells_amd/rust/erased-cells-hip).

The crate keeps the reference's public surface, so parts of it are necessarily the reference's text (erased-cells 0.1.1,
MIT License, Copyright (c) 2023 Astraea, Inc.): trait declarations, signatures, operator-impl headers, the `with_ct!`
table.  Those parts are marked in the source (`// api-surface(<reference file>:<lines>): ...` / `// end api-surface`),
listed in INTEGRATION.md §2, and every file that has one carries the reference's copyright notice.  This test keeps the
three in step and holds the crate to what the round-2 review measured: difflib similarity of each crate file against every
reference file, by characters and by lines, on the non-test parts.  Outside the marked ranges no file may reach 0.6.
The reference itself is not part of this repository: tests/golden/reference_provenance.json records the line count of each
of its source files and, per crate file, the similarity measured for the crate file's exact text (its SHA-256), written by
`python tools/rust_provenance.py --reference DIR --record`.  A crate file whose text has changed since is re-measured that way.
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rust_provenance as rp  # noqa: E402

LIMIT = 0.6
RECORD = json.load(open(rp.RECORD))


def test_markers_are_well_formed_and_cite_the_reference():
    n = 0
    for path in rp.crate_files():
        ranges = rp.marked_ranges(path)  # asserts pairing
        text = open(path).read()
        for a, b, cite, what in ranges:
            n += 1
            assert re.match(r"^src/[a-z_/]+\.rs:\d+-\d+$", cite), f"{path}:{a}: citation {cite!r}"
            assert what.strip(), f"{path}:{a}: no description"
        if ranges:
            head = re.sub(r"\s+", " ", re.sub(r"(?m)^\s*//[/!]?", " ", text[:3000]))  # the notice may wrap over comment lines
            assert "Copyright (c) 2023 Astraea, Inc." in head and "MIT License" in head, \
                f"{os.path.basename(path)} reproduces reference text but does not carry the reference's notice"
    assert n >= 8


def test_integration_md_lists_every_marked_range():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for row in rp.table().split("\n")[2:]:
        assert row in doc, f"INTEGRATION.md §2 PROVENANCE lacks (or has a stale form of) this row — regenerate with " \
                           f"`python tools/rust_provenance.py --table`:\n{row}"
    # and nothing more: every PROVENANCE row of the document is a current one
    current = set(rp.table().split("\n")[2:])
    for line in doc.split("\n"):
        if line.startswith("| `src/") and "api" not in line and re.search(r"\| \d+-\d+ \| `src/", line):
            assert line in current, f"stale PROVENANCE row in INTEGRATION.md:\n{line}"


def test_cited_ranges_exist_in_the_reference():
    counts = RECORD["line_counts"]
    for path in rp.crate_files():
        for a, _b, cite, _ in rp.marked_ranges(path):
            f, lines = cite.split(":")
            lo, hi = (int(x) for x in lines.split("-"))
            assert f in counts, f"{path}:{a}: {cite}: no such reference file"
            assert 1 <= lo <= hi <= counts[f], f"{path}:{a}: {cite}: outside the file"


def test_no_crate_file_resembles_a_reference_file_outside_the_marked_ranges():
    sim = RECORD["similarity"]
    names = [os.path.basename(p) for p in rp.crate_files()]
    assert sorted(sim) == sorted(names), "crate files added or removed since the similarity was recorded: re-measure with " \
                                         "`python tools/rust_provenance.py --reference DIR --record`"
    over = []
    for name in names:
        r = sim[name]
        assert rp.digest(os.path.join(rp.CRATE, name)) == r["sha256"], \
            f"src/{name} changed since its similarity to the reference was recorded: re-measure with " \
            "`python tools/rust_provenance.py --reference DIR --record`"
        if r["marked_ranges_removed"] >= LIMIT:
            over.append(f"{name}: {r['marked_ranges_removed']:.2f} against {r['most_similar_reference_file']} with the marked ranges removed")
    assert not over, "\n".join(over)
