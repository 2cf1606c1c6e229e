#!/usr/bin/env python3
"""ec_focal / ec_focal_convolve beside the streaming kernels that move the same HBM bytes (dev tool).

A 3 x 3 moving sum reads every cell once from HBM and writes one f64 per cell — the byte mix of ec_convert of the same type to
Float64, which reads every byte once with no reuse between lanes.  If the halo costs nothing but LDS, the two run at the same rate;
the first table says whether they do, beside the spread the same script shows when ec_convert runs against itself (the A/A column:
two separate closures over the same entry point, interleaved like the others).  The second table has the 3 x 3 minimum (W bytes in,
W out) beside ec_window copying the whole raster, the third the radius-7 sum and a 5 x 5 convolution as plain rates.  At side²
cells (default 16384²), in one process: four operand-and-output sets are filled on the device and every entry point runs over
them in rotation, so that no byte of a call is still in the 256 MiB Infinity Cache.  Timing is by device events around whole
rotations, after a warm-up of every shape; the entry points of a row alternate, block after block, and the per-call figure is the
median over the blocks.  Share of peak = algorithmic bytes (every cell read once, every output written once) / time / 8 TB/s.

    python tools/focal_bench.py [--side 16384] [--blocks 5] [--min-ms 40] [--out focal.md]

Counters, in runs of their own with no tracing (one counter set per run):

    rocprofv3 --pmc FETCH_SIZE -d DIR/fetch --output-format csv -- python tools/focal_bench.py --pmc-workload
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d DIR/lds --output-format csv -- python tools/focal_bench.py --pmc-workload
    rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS -d DIR/sq --output-format csv -- python tools/focal_bench.py --pmc-workload
    python tools/focal_bench.py --summarise DIR/fetch DIR/lds DIR/sq

`--pmc-workload` launches, once each at --pmc-side² cells (default 8192²), the sum at radius 1 for u8 / u16 / f32 / f64 cells, the sum
at radius 7 for f32, the radius-1 minimum for u8 and a 5 x 5 convolution of f32 cells; `--summarise` prints, per kernel and counter, the sum over its dispatches'
rows (FETCH_SIZE in KiB, x 2 on gfx950 for streamed reads: tools/pmc_traffic.py) beside the algorithmic input bytes and the
tile's halo factor (TW + 2 rx)(TH + 2 ry) / (TW TH).
"""
import argparse
import csv
import ctypes as C
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "erased-cells_amd", "python"))

PEAK_BYTES_PER_S = 8e12
SETS = 4
TW, TH = 64, 16   # csrc/ec_focal_kernels.hpp
PMC_CASES = [("sum r1 u8", 0, 0, 1, 1), ("sum r1 u16", 1, 0, 1, 2), ("sum r1 f32", 8, 0, 1, 4), ("sum r1 f64", 9, 0, 1, 8), ("sum r7 f32", 8, 0, 7, 4),
             ("min r1 u8", 0, 2, 1, 1), ("convolve 5 x 5 f32", 8, "convolve", 2, 4)]   # (label, cell type, op, radius, cell bytes)


def summarise(dirs, side):
    n = side * side
    per = {}
    for d in dirs:
        for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            with open(path, newline="") as f:
                for r in csv.DictReader(f):
                    if "k_focal" not in r.get("Kernel_Name", ""):
                        continue
                    key = (r["Kernel_Name"].split("(")[0], r["Counter_Name"], r["Dispatch_Id"])
                    per[key] = per.get(key, 0.0) + float(r["Counter_Value"])
    print("| kernel | dispatch | counter | value |", "|---|---|---|---|", sep="\n")
    for (kernel, counter, dispatch), v in sorted(per.items(), key=lambda kv: (int(kv[0][2]), kv[0][1])):
        print(f"| `{kernel}` | {dispatch} | {counter} | {v:.0f} |")
    print(f"\ndispatch order of --pmc-workload at {side}² cells: " + "; ".join(
        f"{label} (input {n * w / 1024:.0f} KiB, halo factor {(TW + 2 * r) * (TH + 2 * r) / (TW * TH):.3f})" for label, _, _, r, w in PMC_CASES))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=16384)
    ap.add_argument("--blocks", type=int, default=5, help="timed blocks per entry point (the median is reported)")
    ap.add_argument("--min-ms", type=float, default=40.0, help="least device time of one timed block")
    ap.add_argument("--out", help="also write the tables to this file")
    ap.add_argument("--pmc-workload", action="store_true", help="launch each counter case once and exit (to run under rocprofv3 --pmc)")
    ap.add_argument("--pmc-side", type=int, default=8192)
    ap.add_argument("--summarise", nargs="+", metavar="DIR", help="read rocprofv3 counter CSVs of --pmc-workload runs")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.pmc_side)

    import torch

    import erased_cells_hip as ec

    side = args.pmc_side if args.pmc_workload else args.side
    n = side * side
    torch.cuda.set_device(0)
    ec.init(0)
    L, chk, E = ec.lib(), ec._ffi.check, ec._ffi
    stream = torch.cuda.current_stream().cuda_stream
    ec.set_stream(stream)

    def fill(ct, seed, lo, hi):
        a = ec.CellBuffer.empty(n, ct)
        chk(L.ec_synth_fill(ct, a.mem.ptr, n, seed, 0, lo, hi, stream))
        return a

    if args.pmc_workload:
        f32 = fill(ec.Float32, 1, -300.0, 300.0)
        src = {0: fill(ec.UInt8, 2, 0, 255), 1: fill(ec.UInt16, 3, 0, 65535), 8: f32, 9: f32.convert(ec.Float64)}
        out = ec.CellBuffer.empty(n, ec.Float64)
        torch.cuda.synchronize()
        w5 = (C.c_double * 25)(*[((i * 7) % 11 - 5) / 16.0 for i in range(25)])
        for label, ct, op, r, _ in PMC_CASES:
            if op == "convolve":
                chk(L.ec_focal_convolve(ct, src[ct].mem.ptr, None, side, side, w5, r, r, 0, out.mem.ptr, None, stream))
            else:
                chk(L.ec_focal(op, ct, src[ct].mem.ptr, None, side, side, r, r, 0, out.mem.ptr, None, stream))
            torch.cuda.synchronize()
        return

    def block(fn, rotations):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rotations):
            for k in range(SETS):
                fn(k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (rotations * SETS)  # ms per call

    def measure(fns):
        """median ms per call of each of `fns`, alternating block after block"""
        est = {}
        for fn in fns:
            block(fn, 1)   # warm-up of every shape
            est[fn] = block(fn, 1)
        rot = {fn: max(1, int(args.min_ms / (est[fn] * SETS)) + 1) for fn in fns}
        t = {fn: [] for fn in fns}
        for _ in range(args.blocks):
            for fn in fns:
                t[fn].append(block(fn, rot[fn]))
        return [(statistics.median(t[fn]), min(t[fn]), max(t[fn])) for fn in fns]

    def share(moved, ms):
        return moved / (ms * 1e-3) / PEAK_BYTES_PER_S

    def focal(op, ct, cells, r, outs):
        def fn(k):
            chk(L.ec_focal(op, ct, cells[k].mem.ptr, None, side, side, r, r, 0, outs[k].mem.ptr, None, stream))
        return fn

    out64 = [ec.CellBuffer.empty(n, ec.Float64) for _ in range(SETS)]
    sources = {"u8": (ec.UInt8, [fill(ec.UInt8, 0xF0 + k, 0, 255) for k in range(SETS)]),
               "u16": (ec.UInt16, [fill(ec.UInt16, 0xF4 + k, 0, 65535) for k in range(SETS)]),
               "f32": (ec.Float32, [fill(ec.Float32, 0xF8 + k, -300.0, 300.0) for k in range(SETS)])}
    lines = [f"ec_focal SUM 3 x 3 beside ec_convert to Float64 on the same byte mix, {side}² cells, unmasked", "",
             "| cells | bytes in / out | ec_convert µs | the same again (A/A) µs | A/A | ec_focal SUM 3 x 3 µs | focal / convert | convert share of 8 TB/s | focal share |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, (ct, cells) in sources.items():
        def convert(k, ct=ct, cells=cells):
            chk(L.ec_convert(ct, cells[k].mem.ptr, ec.Float64, out64[k].mem.ptr, n, stream))

        def convert_again(k, ct=ct, cells=cells):
            chk(L.ec_convert(ct, cells[k].mem.ptr, ec.Float64, out64[k].mem.ptr, n, stream))

        (a, a0, a1), (b, b0, b1), (c, c0, c1) = measure([convert, convert_again, focal(E.EC_FOCAL_SUM, ct, cells, 1, out64)])
        w = ec.size_of(ct)
        lines.append(f"| {name} | {w} / 8 | {a * 1e3:.1f} | {b * 1e3:.1f} | {b / a:.3f} | {c * 1e3:.1f} | {c / a:.3f} | {share(n * (w + 8), a):.3f} | {share(n * (w + 8), c):.3f} |")
        print(lines[-1], f"  (spread: convert {a0 * 1e3:.1f}-{a1 * 1e3:.1f}, again {b0 * 1e3:.1f}-{b1 * 1e3:.1f}, focal {c0 * 1e3:.1f}-{c1 * 1e3:.1f} µs)", flush=True)

    lines += ["", f"ec_focal MIN 3 x 3 beside ec_window copying the whole raster, {side}² cells, unmasked", "",
              "| cells | bytes in / out | ec_window µs | ec_focal MIN 3 x 3 µs | focal / window | window share of 8 TB/s | focal share |", "|---|---|---|---|---|---|---|"]
    for name, (ct, cells) in sources.items():
        w = ec.size_of(ct)
        outs = [ec.CellBuffer(ct, n, o.mem) for o in out64]   # the narrow outputs sit in the front of the f64 ones

        def window(k, ct=ct, cells=cells, outs=outs):
            chk(L.ec_window(ct, cells[k].mem.ptr, None, side, side, 0, 0, side, side, side, side, outs[k].mem.ptr, None, stream))

        (a, a0, a1), (c, c0, c1) = measure([window, focal(E.EC_FOCAL_MIN, ct, cells, 1, outs)])
        lines.append(f"| {name} | {w} / {w} | {a * 1e3:.1f} | {c * 1e3:.1f} | {c / a:.3f} | {share(n * 2 * w, a):.3f} | {share(n * 2 * w, c):.3f} |")
        print(lines[-1], f"  (spread: window {a0 * 1e3:.1f}-{a1 * 1e3:.1f}, focal {c0 * 1e3:.1f}-{c1 * 1e3:.1f} µs)", flush=True)

    lines += ["", f"larger footprints as plain rates, f32 cells, {side}² cells, unmasked", "",
              "| call | taps | µs | cells per second | share of 8 TB/s (12 bytes per cell) |", "|---|---|---|---|---|"]
    ct, cells = sources["f32"]
    w5 = (C.c_double * 25)(*[((i * 7) % 11 - 5) / 16.0 for i in range(25)])

    def conv5(k):
        chk(L.ec_focal_convolve(ct, cells[k].mem.ptr, None, side, side, w5, 2, 2, 0, out64[k].mem.ptr, None, stream))

    for label, fn, taps in (("ec_focal SUM radius 7", focal(E.EC_FOCAL_SUM, ct, cells, 7, out64), 225), ("ec_focal MAX radius 7", focal(E.EC_FOCAL_MAX, ct, cells, 7, [ec.CellBuffer(ct, n, o.mem) for o in out64]), 225),
                            ("ec_focal_convolve 5 x 5", conv5, 25)):
        (a, a0, a1), = measure([fn])
        lines.append(f"| {label} | {taps} | {a * 1e3:.1f} | {n / (a * 1e-3):.3e} | {share(n * 12, a):.3f} |")
        print(lines[-1], f"  (spread {a0 * 1e3:.1f}-{a1 * 1e3:.1f} µs)", flush=True)
    table = "\n".join(lines)
    print()
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
