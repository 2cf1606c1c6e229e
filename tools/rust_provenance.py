#!/usr/bin/env python3
"""rust_provenance.py — which lines of the Rust crate are the reference's text, and how similar is the rest?

The crate (erased-cells_amd/rust/erased-cells-hip) keeps the reference's public surface: names, signatures, trait and
operator impl headers, the `with_ct!` table.  Those declarations are necessarily the reference's text; they are marked in
the source with comment pairs

    // api-surface(src/encoding.rs:9-40): what it is
    ...
    // end api-surface

This tool lists the marked ranges (the PROVENANCE table of INTEGRATION.md §2 is its `--table` output) and measures, per
crate file, difflib similarity against every file of the reference — with the marked ranges removed and with them in —
by characters and by lines, on the non-test part of both sides (the measure the round-2 review used).  `--record` keeps
what the tests need of the reference in tests/golden/reference_provenance_zonal_table.json (`RECORD` below): the line count of every reference source
file (for the citations) and, per crate file, its SHA-256 with the similarity measured for exactly that text.

    python tools/rust_provenance.py --table                                  # markdown table of the marked ranges
    python tools/rust_provenance.py --reference DIR --similarity             # DIR: the erased-cells 0.1.1 source tree
    python tools/rust_provenance.py --reference DIR --record                 # rewrite the tests' record
"""
import argparse
import difflib
import glob
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CRATE = os.path.join(ROOT, "erased-cells_amd", "rust", "erased-cells-hip", "src")
# The record is written anew whenever a crate file changes; each writing is a file of its own (reference_provenance.json describes
# the crate before ec_window / ec_window_put entered ffi.rs and the buffer types, reference_provenance_r05.json the crate before
# ec_window_resample did, reference_provenance_resample.json the crate before the band statistics did, reference_provenance_stats.json the crate before
# compare / select did, reference_provenance_compare.json the crate before cast / to_scaled did, reference_provenance_cast.json the crate before
# focal / convolve did, reference_provenance_focal.json the crate before composite did, reference_provenance_composite.json the crate
# before the zonal statistics did, reference_provenance_zonal.json the crate before reclassify did, reference_provenance_reclass.json the crate before
# composite_rank did, reference_provenance_composite_rank.json the crate before focal_rank / focal_majority did, reference_provenance_focal_rank.json the crate before
# distance / within did, reference_provenance_distance.json the crate before regions / sieve did, reference_provenance_regions.json the crate before
# zonal_table / lookup did; all are kept as they were recorded).
RECORD = os.path.join(ROOT, "tests", "golden", "reference_provenance_zonal_table.json")
OPEN = re.compile(r"^\s*// api-surface\(([^)]*)\):\s*(.*)$")
CLOSE = re.compile(r"^\s*// end api-surface\s*$")


def marked_ranges(path):
    """[(first_line, last_line, reference cite, what)] — 1-based, markers included"""
    out, cur = [], None
    for i, line in enumerate(open(path).read().split("\n"), 1):
        m = OPEN.match(line)
        if m:
            assert cur is None, f"{path}:{i}: nested api-surface marker"
            cur = (i, m.group(1), m.group(2))
        elif CLOSE.match(line):
            assert cur is not None, f"{path}:{i}: end marker without a start"
            out.append((cur[0], i, cur[1], cur[2]))
            cur = None
    assert cur is None, f"{path}: unterminated api-surface marker"
    return out


def nontest(text):
    i = text.find("#[cfg(test)]")
    return text[:i] if i >= 0 else text


def without_marked(path):
    lines = open(path).read().split("\n")
    drop = set()
    for a, b, _, _ in marked_ranges(path):
        drop.update(range(a, b + 1))
    return "\n".join(l for i, l in enumerate(lines, 1) if i not in drop)


def line_ratio(a, b):
    return difflib.SequenceMatcher(None, a.splitlines(), b.splitlines(), autojunk=False).ratio()


def char_ratio(a, b):
    return difflib.SequenceMatcher(None, a, b, autojunk=False).ratio()


def best_match(text, refs, exhaustive):
    """(similarity, reference file): max over the reference files of max(char ratio, line ratio).  The character ratio is
    quadratic in the file sizes (minutes for the whole cross product), so unless `exhaustive` it is computed for the
    two reference files with the highest line ratio — the candidates for "the same text" — and the line ratio stands
    for the others."""
    by_lines = sorted(((line_ratio(text, rt), rn) for rn, rt in refs.items()), reverse=True)
    best = by_lines[0]
    for l, rn in (by_lines if exhaustive else by_lines[:2]):
        c = char_ratio(text, refs[rn])
        if max(c, l) > best[0]:
            best = (max(c, l), rn)
    return best


def crate_files():
    return sorted(glob.glob(os.path.join(CRATE, "*.rs")))


def table():
    rows = ["| crate file | lines | reference text it reproduces (erased-cells 0.1.1, MIT, © 2023 Astraea, Inc.) | what |", "|---|---|---|---|"]
    for p in crate_files():
        for a, b, cite, what in marked_ranges(p):
            rows.append(f"| `src/{os.path.basename(p)}` | {a}-{b} | `{cite}` | {what} |")
    return "\n".join(rows)


def digest(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def reference_files(ref_root):
    """{path relative to the reference's root ("src/..."): text} of every Rust source file of the reference"""
    src = os.path.join(ref_root, "src")
    return {os.path.relpath(p, ref_root): open(p).read() for p in sorted(glob.glob(os.path.join(src, "**", "*.rs"), recursive=True))}


def similarities(ref_root, exhaustive=False, with_full=True):
    refs = {os.path.relpath(f, "src"): nontest(t) for f, t in reference_files(ref_root).items()}
    out = []
    for p in crate_files():
        full, stripped = nontest(open(p).read()), nontest(without_marked(p))
        out.append((os.path.basename(p), best_match(stripped, refs, exhaustive), best_match(full, refs, exhaustive) if with_full else (None, None)))
    return out


def record(ref_root):
    """What tests/test_rust_provenance.py holds the crate to, measured against the reference tree at `ref_root`."""
    rec = {"reference": "erased-cells 0.1.1 (MIT License, Copyright (c) 2023 Astraea, Inc.)",
           "line_counts": {f: len(t.split("\n")) for f, t in reference_files(ref_root).items()},
           "similarity": {}}
    for name, (s, rn), _ in similarities(ref_root, with_full=False):
        rec["similarity"][name] = {"sha256": digest(os.path.join(CRATE, name)), "marked_ranges_removed": round(s, 4),
                                   "most_similar_reference_file": rn}
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--similarity", action="store_true")
    ap.add_argument("--record", action="store_true", help=f"rewrite {os.path.relpath(RECORD, ROOT)} from --reference")
    ap.add_argument("--reference", metavar="DIR", help="root of the reference's source tree (erased-cells 0.1.1: Cargo.toml, src/)")
    ap.add_argument("--exhaustive", action="store_true", help="character ratio against every reference file (minutes)")
    a = ap.parse_args()
    if a.table or not (a.similarity or a.record):
        print(table())
    if (a.similarity or a.record) and not (a.reference and os.path.isdir(os.path.join(a.reference, "src"))):
        sys.exit("--similarity and --record need --reference DIR, the reference's source tree")
    if a.similarity:
        print("\n| crate file | most similar reference file, marked ranges removed | with them in |\n|---|---|---|")
        for name, (s, rn), (f, fn) in similarities(a.reference, a.exhaustive):
            print(f"| `src/{name}` | {s:.2f} `{rn}` | {f:.2f} `{fn}` |")
    if a.record:
        record(a.reference)


if __name__ == "__main__":
    main()
