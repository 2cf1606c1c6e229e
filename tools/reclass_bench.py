#!/usr/bin/env python3
"""ec_reclass beside ec_cast of the same type pair: what the search costs (dev tool).

At side² cells (default 16384²), in one process, for (t, dt) = (UInt8, UInt8), (UInt16, UInt8), (Float32, UInt8), (Float64, Float64):
one ec_reclass pass with 4, 32 and 255 breaks spread evenly over the cells' range, unmasked and masked (mask in, nodata, mask
out), against ec_cast(EC_CAST_ROUND) of the same (t, dt) — the call that moves the same value bytes with no table and no search
(for t == dt it is the library's copy).  The masked form moves two more bytes per cell than the cast it stands beside; the
"share of 8 TB/s" column counts them.

Every operand byte comes from HBM: `--sets` (default 2) operand-and-output sets are used in rotation.  Timing is by device
events around whole rotations, after a warm-up of every shape; the per-call figure is the median over the blocks, with the least
and the greatest beside it.  The first 2^20 cells of every unmasked result are checked against numpy.digitize at the end.

    python tools/reclass_bench.py [--side 16384] [--blocks 5] [--min-ms 60] [--sets 2] [--out reclass.md]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "erased-cells_amd", "python"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import erased_cells_hip as ec  # noqa: E402

PEAK_BYTES_PER_S = 8e12
BREAK_COUNTS = (4, 32, 255)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=16384)
    ap.add_argument("--blocks", type=int, default=5, help="timed blocks per entry point (the median is reported)")
    ap.add_argument("--min-ms", type=float, default=60.0, help="least device time of one timed block")
    ap.add_argument("--sets", type=int, default=2, help="operand sets used in rotation")
    ap.add_argument("--out", help="also write the table to this file")
    args = ap.parse_args()
    side, sets = args.side, args.sets
    n = side * side
    torch.cuda.set_device(0)
    ec.init(0)
    L, chk, E = ec.lib(), ec._ffi.check, ec._ffi
    stream = torch.cuda.current_stream().cuda_stream
    ec.set_stream(stream)
    pairs = ((ec.UInt8, ec.UInt8, 0, 255), (ec.UInt16, ec.UInt8, 0, 65535), (ec.Float32, ec.UInt8, 0.0, 1.0), (ec.Float64, ec.Float64, 0.0, 1.0))

    def block(fn, rotations):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rotations):
            for s in range(sets):
                fn(s)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (rotations * sets)  # ms per call

    def measure(fns):
        """(median, least, greatest) ms per call of each of `fns`, alternating block after block"""
        est = {}
        for fn in fns:
            block(fn, 1)   # warm-up of every shape
            est[fn] = block(fn, 1)
        rot = {fn: max(1, int(args.min_ms / (est[fn] * sets)) + 1) for fn in fns}
        t = {fn: [] for fn in fns}
        for _ in range(args.blocks):
            for fn in fns:
                t[fn].append(block(fn, rot[fn]))
        return [(statistics.median(t[fn]), min(t[fn]), max(t[fn])) for fn in fns]

    lines = [f"ec_reclass against ec_cast(EC_CAST_ROUND) of the same type pair, {side}² cells, {sets} sets in rotation", "",
             "| call | breaks | algorithmic B / cell | µs | share of 8 TB/s | spread µs | x ec_cast |", "|---|---|---|---|---|---|---|"]
    worst = (0.0, "")
    for t, dt, lo, hi in pairs:
        name = f"{ec.CT_NAMES[t]} -> {ec.CT_NAMES[dt]}"
        wt, wd = ec.NP_DTYPES[t].itemsize, ec.NP_DTYPES[dt].itemsize
        src, masks, dst, dmask = [], [], [], []
        for s in range(sets):
            if t == ec.Float64:   # the generator has no f64 form: f32 cells widened
                f = ec.CellBuffer.empty(n, ec.Float32)
                chk(L.ec_synth_fill(ec.Float32, f.mem.ptr, n, 0x2E00 + s, 0, lo, hi, stream))
                v = f.convert(ec.Float64)
                del f
            else:
                v = ec.CellBuffer.empty(n, t)
                chk(L.ec_synth_fill(t, v.mem.ptr, n, 0x2E00 + s, 0, lo, hi, stream))
            m = ec.Mask.empty(n)
            chk(L.ec_synth_mask(m.mem.ptr, n, 0x2E10 + s, 0, 30, stream))
            src.append(v)
            masks.append(m)
            dst.append(ec.CellBuffer.empty(n, dt))
            dmask.append(ec.Mask.empty(n))
        integral = ec.NP_DTYPES[t].kind != "f"
        tables = {}
        for nb in BREAK_COUNTS:
            edges = np.linspace(lo, hi, nb + 2)[1:-1]
            breaks = np.unique(np.round(edges)).astype(ec.NP_DTYPES[t]) if integral else edges
            if integral and breaks.size < nb:   # 255 breaks of a u8 raster: 1 .. 255
                breaks = np.arange(1, nb + 1).astype(ec.NP_DTYPES[t])
            values = (np.arange(breaks.size + 1) % 251).astype(ec.NP_DTYPES[dt])
            tables[nb] = (ec.ReclassTable(t, breaks, values), ec.ReclassTable(t, breaks, values, nodata=255), breaks, values)

        def cast(s):
            chk(L.ec_cast(E.EC_CAST_ROUND, t, src[s].mem.ptr, dt, dst[s].mem.ptr, n, stream))

        def reclass(nb, masked):
            tab = tables[nb][1 if masked else 0]

            def fn(s):
                chk(L.ec_reclass(t, src[s].mem.ptr, masks[s].mem.ptr if masked else None, n, dt, tab.mem.ptr, dst[s].mem.ptr,
                                 dmask[s].mem.ptr if masked else None, stream))
            return fn

        fns = [cast] + [reclass(nb, masked) for nb in BREAK_COUNTS for masked in (False, True)]
        ts = measure(fns)
        t_cast = ts[0]

        def row(label, nb, per_cell, tt, ratio):
            share = n * per_cell / (tt[0] * 1e-3) / PEAK_BYTES_PER_S
            return f"| {label} | {nb} | {per_cell} | {tt[0] * 1e3:.1f} | {share:.3f} | {tt[1] * 1e3:.1f}-{tt[2] * 1e3:.1f} | {ratio} |"

        lines.append(row(f"ec_cast {name}", "", wt + wd, t_cast, "1.00"))
        k = 1
        for nb in BREAK_COUNTS:
            for masked in (False, True):
                r = ts[k][0] / t_cast[0]
                label = f"ec_reclass {name}{', masked' if masked else ''}"
                lines.append(row(label, nb, wt + wd + (2 if masked else 0), ts[k], f"{r:.2f}"))
                if r > worst[0]:
                    worst = (r, f"{label}, {nb} breaks")
                k += 1
        for line in lines[-7:]:
            print(line, flush=True)
        # fast and wrong is not fast: the head of every unmasked result against numpy
        head = 1 << 20
        x = ec.buffer._download(src[0].mem, ec.NP_DTYPES[t], head)
        for nb in BREAK_COUNTS:
            reclass(nb, False)(0)
            got = ec.buffer._download(dst[0].mem, ec.NP_DTYPES[dt], head)
            _, _, breaks, values = tables[nb]
            want = values[np.digitize(x.astype(np.float64), breaks.astype(np.float64))]
            assert np.array_equal(got, want), f"ec_reclass {name} with {nb} breaks differs from numpy.digitize"
        del src, masks, dst, dmask, tables
    lines += ["", f"worst ratio: {worst[0]:.2f} x ec_cast ({worst[1]}); every unmasked result's first 2^20 cells equal numpy.digitize"]
    table = "\n".join(lines)
    print()
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
