#!/usr/bin/env python3
"""ec_cast beside ec_mask_from_nodata on the same byte mix, and ec_cast / ec_cast_scaled as a share of the HBM peak (dev tool).

ec_cast Float64 -> UInt8 moves the byte mix of ec_mask_from_nodata on Float64 — 8 bytes in, 1 byte out per cell — and UInt16 ->
UInt8 that of ec_mask_from_nodata on UInt16, so each pair should run at the same rate; the table says whether it does, beside the
spread the same script shows when the baseline kernel runs against itself (the A/A column: two separate closures over the same
entry point, interleaved like the others).  At side² cells (default 16384²), in one process: four operand-and-output sets are
filled on the device and every entry point runs over them in rotation, so that no byte of a call is still in the 256 MiB Infinity
Cache.  Timing is by device events around whole rotations, after a warm-up of every shape; the entry points of a row alternate,
block after block, and the per-call figure is the median over the blocks.  Share of peak = algorithmic bytes (every operand and
mask read once, every output written once) / time / 8 TB/s.

    python tools/cast_bench.py [--side 16384] [--blocks 7] [--min-ms 60] [--baseline-lib OTHER.so] [--out cast.md]

`--baseline-lib`: a second build of the library (e.g. the parent commit's) whose ec_mask_from_nodata and ec_convert are the
baselines, loaded into the same process and interleaved with this build's entry points; without it the baselines are this build's own.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "erased-cells_amd", "python"))

import torch  # noqa: E402

import erased_cells_hip as ec  # noqa: E402

PEAK_BYTES_PER_S = 8e12
SETS = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=16384)
    ap.add_argument("--blocks", type=int, default=7, help="timed blocks per entry point (the median is reported)")
    ap.add_argument("--min-ms", type=float, default=60.0, help="least device time of one timed block")
    ap.add_argument("--baseline-lib", help="another build of the library: its ec_mask_from_nodata / ec_convert are the baselines")
    ap.add_argument("--out", help="also write the tables to this file")
    args = ap.parse_args()
    n = args.side * args.side
    torch.cuda.set_device(0)
    ec.init(0)
    L, chk, E = ec.lib(), ec._ffi.check, ec._ffi
    stream = torch.cuda.current_stream().cuda_stream
    ec.set_stream(stream)
    base = L
    if args.baseline_lib:
        base = C.CDLL(os.path.abspath(args.baseline_lib))
        base.ec_init.argtypes, base.ec_init.restype = [C.c_int32], C.c_int32
        for name in ("ec_mask_from_nodata", "ec_convert"):
            getattr(base, name).restype, getattr(base, name).argtypes = E.SIGNATURES[name]
        assert base.ec_init(0) == 0, "the baseline library did not initialise"

    def fill(ct, seed, lo, hi):
        a = ec.CellBuffer.empty(n, ct)
        chk(L.ec_synth_fill(ct, a.mem.ptr, n, seed, 0, lo, hi, stream))
        return a

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
            block(fn, 2)   # warm-up of every shape
            est[fn] = block(fn, 2)
        rot = {fn: max(2, int(args.min_ms / (est[fn] * SETS)) + 1) for fn in fns}
        t = {fn: [] for fn in fns}
        for _ in range(args.blocks):
            for fn in fns:
                t[fn].append(block(fn, rot[fn]))
        return [(statistics.median(t[fn]), min(t[fn]), max(t[fn])) for fn in fns]

    def share(moved, ms):
        return moved / (ms * 1e-3) / PEAK_BYTES_PER_S

    which = "the baseline build" if args.baseline_lib else "this build"
    lines = [f"ec_cast beside ec_mask_from_nodata of {which} on the same byte mix, {args.side}² cells", "",
             "| cells | bytes in / out | ec_mask_from_nodata µs | the same again (A/A) µs | A/A | ec_cast ROUND -> u8 µs | ROUND / baseline | "
             "ec_cast AS -> u8 µs | AS / baseline | baseline share of 8 TB/s | ROUND share |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    out8 = [ec.CellBuffer.empty(n, ec.UInt8) for _ in range(SETS)]
    f32 = [fill(ec.Float32, 0xCA57 + k, -300.0, 300.0) for k in range(SETS)]
    f64 = [a.convert(ec.Float64) for a in f32]
    u16 = [fill(ec.UInt16, 0xCA58 + k, 0, 65535) for k in range(SETS)]
    for name, ct, cells in (("f64", ec.Float64, f64), ("u16", ec.UInt16, u16)):
        v = ec.CellValue(ct, 0).to_ec()

        def nodata(k):
            st = base.ec_mask_from_nodata(ct, cells[k].mem.ptr, n, C.byref(v), out8[k].mem.ptr, stream)
            assert st == 0, st

        def nodata_again(k):
            st = base.ec_mask_from_nodata(ct, cells[k].mem.ptr, n, C.byref(v), out8[k].mem.ptr, stream)
            assert st == 0, st

        def cast_round(k):
            chk(L.ec_cast(E.EC_CAST_ROUND, ct, cells[k].mem.ptr, ec.UInt8, out8[k].mem.ptr, n, stream))

        def cast_as(k):
            chk(L.ec_cast(E.EC_CAST_AS, ct, cells[k].mem.ptr, ec.UInt8, out8[k].mem.ptr, n, stream))

        (a, a0, a1), (b, b0, b1), (c, c0, c1), (d, d0, d1) = measure([nodata, nodata_again, cast_round, cast_as])
        w = ec.size_of(ct)
        moved = n * (w + 1)
        lines.append(f"| {name} | {w} / 1 | {a * 1e3:.1f} | {b * 1e3:.1f} | {b / a:.3f} | {c * 1e3:.1f} | {c / a:.3f} | {d * 1e3:.1f} | {d / a:.3f} | "
                     f"{share(moved, a):.3f} | {share(moved, c):.3f} |")
        print(lines[-1], f"  (spread: baseline {a0 * 1e3:.1f}-{a1 * 1e3:.1f}, again {b0 * 1e3:.1f}-{b1 * 1e3:.1f}, ROUND {c0 * 1e3:.1f}-{c1 * 1e3:.1f}, "
                         f"AS {d0 * 1e3:.1f}-{d1 * 1e3:.1f} µs)", flush=True)
    del u16, out8

    lines += ["", f"ec_cast and ec_cast_scaled from Float64, beside ec_convert f32 -> f64 of {which}, {args.side}² cells", "",
              "| call | bytes per cell | µs | share of 8 TB/s |", "|---|---|---|---|"]
    out64 = [ec.CellBuffer.empty(n, ec.Float64) for _ in range(SETS)]

    def widen(k):
        st = base.ec_convert(ec.Float32, f32[k].mem.ptr, ec.Float64, out64[k].mem.ptr, n, stream)
        assert st == 0, st
    (a, a0, a1), = measure([widen])
    lines.append(f"| ec_convert f32 -> f64 ({which}) | 12 | {a * 1e3:.1f} | {share(n * 12, a):.3f} |")
    print(lines[-1], f"  (spread {a0 * 1e3:.1f}-{a1 * 1e3:.1f} µs)", flush=True)
    del out64
    out32 = [ec.CellBuffer.empty(n, ec.Float32) for _ in range(SETS)]
    masks = [ec.Mask.empty(n) for _ in range(SETS)]
    for k, m in enumerate(masks):
        chk(L.ec_synth_mask(m.mem.ptr, n, 0xA600 + k, 0, 30, stream))
    nd = ec.CellValue(ec.Int16, -9999).to_ec()

    def to_f32(k):
        chk(L.ec_cast(E.EC_CAST_ROUND, ec.Float64, f64[k].mem.ptr, ec.Float32, out32[k].mem.ptr, n, stream))

    def to_i16(k):   # the 2-byte outputs sit in the front half of the 4-byte ones
        chk(L.ec_cast(E.EC_CAST_ROUND, ec.Float64, f64[k].mem.ptr, ec.Int16, out32[k].mem.ptr, n, stream))

    def scaled_i16(k):
        chk(L.ec_cast_scaled(ec.Float64, f64[k].mem.ptr, None, n, 100.0, 0.0, ec.Int16, None, out32[k].mem.ptr, stream))

    def masked_scaled_i16(k):
        chk(L.ec_cast_scaled(ec.Float64, f64[k].mem.ptr, masks[k].mem.ptr, n, 100.0, 0.0, ec.Int16, C.byref(nd), out32[k].mem.ptr, stream))

    for label, fn, per_cell in (("ec_cast f64 -> f32", to_f32, 12), ("ec_cast ROUND f64 -> i16", to_i16, 10),
                                ("ec_cast_scaled f64 -> i16", scaled_i16, 10), ("ec_cast_scaled f64 -> i16, masked", masked_scaled_i16, 11)):
        (a, a0, a1), = measure([fn])
        lines.append(f"| {label} | {per_cell} | {a * 1e3:.1f} | {share(n * per_cell, a):.3f} |")
        print(lines[-1], f"  (spread {a0 * 1e3:.1f}-{a1 * 1e3:.1f} µs)", flush=True)
    table = "\n".join(lines)
    print()
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
