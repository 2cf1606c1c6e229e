#!/usr/bin/env python3
"""ec_compare_scalar beside ec_mask_from_nodata, and ec_compare / ec_select as a share of the HBM peak (dev tool).

ec_compare_scalar moves the byte mix of ec_mask_from_nodata — W bytes in, 1 byte out per cell — so the two should run at the same
rate; the table says whether they do.  At side² cells (default 16384²), in one process: four operand-and-output sets are filled on
the device and every entry point runs over them in rotation, so that no byte of a call is still in the 256 MiB Infinity Cache
(the smallest set, u8 in and a mask out, is 512 MiB: 1.5 GiB of other bytes pass between two uses of a set).  Timing is by device
events around whole rotations, after a warm-up of every shape; the entry points of a row alternate, block after block, and the
per-call figure is the median over the blocks.  Share of peak = algorithmic bytes (every operand and mask read once, every output
written once) / time / 8 TB/s.

    python tools/compare_bench.py [--side 16384] [--blocks 7] [--min-ms 60] [--baseline-lib OTHER.so] [--out compare.md]

`--baseline-lib`: a second build of the library (e.g. the parent commit's) whose ec_mask_from_nodata is the baseline, loaded into
the same process and interleaved with this build's entry points; without it the baseline is this build's own ec_mask_from_nodata.
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
TYPES = {"u8": ec.UInt8, "u16": ec.UInt16, "f32": ec.Float32, "f64": ec.Float64}
SYNTH = {ec.UInt8: ec.UInt8, ec.UInt16: ec.UInt16, ec.Float32: ec.Float32, ec.Float64: ec.Float32}   # ec_synth_fill writes u8, u16, f32
RANGE = {ec.UInt8: (0, 255), ec.UInt16: (0, 65535), ec.Float32: (-1000.0, 1000.0)}
MIDDLE = {ec.UInt8: 128, ec.UInt16: 32768, ec.Float32: 0.0, ec.Float64: 0.0}   # a scalar about half of the cells are below


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=16384)
    ap.add_argument("--blocks", type=int, default=7, help="timed blocks per entry point (the median is reported)")
    ap.add_argument("--min-ms", type=float, default=60.0, help="least device time of one timed block")
    ap.add_argument("--baseline-lib", help="another build of the library: its ec_mask_from_nodata is the baseline")
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
        base.ec_mask_from_nodata.restype, base.ec_mask_from_nodata.argtypes = E.SIGNATURES["ec_mask_from_nodata"]
        assert base.ec_init(0) == 0, "the baseline library did not initialise"

    def fill(ct, seed):
        src = SYNTH[ct]
        a = ec.CellBuffer.empty(n, src)
        lo, hi = RANGE[src]
        chk(L.ec_synth_fill(src, a.mem.ptr, n, seed, 0, lo, hi, stream))
        return a if src == ct else a.convert(ct)

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
    lines = [f"ec_compare_scalar beside ec_mask_from_nodata of {which}, {args.side}² cells, W bytes in and 1 byte out per cell", "",
             "| cells | ec_mask_from_nodata µs | ec_compare_scalar (<) µs | ec_compare_scalar (!=) µs | < / baseline | != / baseline | baseline share of 8 TB/s | < share |",
             "|---|---|---|---|---|---|---|---|"]
    outs = [ec.Mask.empty(n) for _ in range(SETS)]
    cells_of = {}
    for name, ct in TYPES.items():
        cells = cells_of[name] = [fill(ct, 0xC0DE + k) for k in range(SETS)]
        v = ec.CellValue(ct, MIDDLE[ct]).to_ec()

        def nodata(k):
            st = base.ec_mask_from_nodata(ct, cells[k].mem.ptr, n, C.byref(v), outs[k].mem.ptr, stream)
            assert st == 0, st

        def less(k):
            chk(L.ec_compare_scalar(E.EC_CMP_LT, ct, cells[k].mem.ptr, None, n, C.byref(v), outs[k].mem.ptr, stream))

        def differs(k):
            chk(L.ec_compare_scalar(E.EC_CMP_NE, ct, cells[k].mem.ptr, None, n, C.byref(v), outs[k].mem.ptr, stream))

        (a, a0, a1), (b, b0, b1), (c, c0, c1) = measure([nodata, less, differs])
        moved = n * (ec.size_of(ct) + 1)
        lines.append(f"| {name} | {a * 1e3:.1f} | {b * 1e3:.1f} | {c * 1e3:.1f} | {b / a:.3f} | {c / a:.3f} | {share(moved, a):.3f} | {share(moved, b):.3f} |")
        print(lines[-1], f"  (spread: baseline {a0 * 1e3:.1f}-{a1 * 1e3:.1f}, < {b0 * 1e3:.1f}-{b1 * 1e3:.1f}, != {c0 * 1e3:.1f}-{c1 * 1e3:.1f} µs)", flush=True)
        if name == "f32":
            del cells_of["f32"]   # not used below: give the memory back

    lines += ["", f"ec_compare and ec_select, {args.side}² cells", "", "| call | bytes per cell | µs | share of 8 TB/s |", "|---|---|---|---|"]
    second = {"u16": [fill(ec.UInt16, 0xD00D + k) for k in range(SETS)], "f64": [fill(ec.Float64, 0xD00D + k) for k in range(SETS)]}
    f32 = [fill(ec.Float32, 0xF00D + k) for k in range(SETS)]
    sels = [ec.Mask.empty(n) for _ in range(SETS)]
    for k, m in enumerate(sels):
        chk(L.ec_synth_mask(m.mem.ptr, n, 0xA500 + k, 0, 50, stream))
    for label, lt, l, rt, r in (("ec_compare u16 < u16", ec.UInt16, cells_of["u16"], ec.UInt16, second["u16"]),
                                ("ec_compare u8 < f32", ec.UInt8, cells_of["u8"], ec.Float32, f32),
                                ("ec_compare f64 < f64", ec.Float64, cells_of["f64"], ec.Float64, second["f64"])):
        def compare(k):
            chk(L.ec_compare(E.EC_CMP_LT, lt, l[k].mem.ptr, None, rt, r[k].mem.ptr, None, n, outs[k].mem.ptr, stream))
        (a, a0, a1), = measure([compare])
        per_cell = ec.size_of(lt) + ec.size_of(rt) + 1
        lines.append(f"| {label} | {per_cell} | {a * 1e3:.1f} | {share(n * per_cell, a):.3f} |")
        print(lines[-1], f"  (spread {a0 * 1e3:.1f}-{a1 * 1e3:.1f} µs)", flush=True)
    del f32
    for name in ("u16", "f64"):
        ct = TYPES[name]
        a_, b_ = cells_of[name], second[name]
        dst = [ec.CellBuffer.empty(n, ct) for _ in range(SETS)]

        def select(k):
            chk(L.ec_select(ct, a_[k].mem.ptr, b_[k].mem.ptr, sels[k].mem.ptr, n, dst[k].mem.ptr, stream))
        (a, a0, a1), = measure([select])
        per_cell = 3 * ec.size_of(ct) + 1
        lines.append(f"| ec_select {name} | {per_cell} | {a * 1e3:.1f} | {share(n * per_cell, a):.3f} |")
        print(lines[-1], f"  (spread {a0 * 1e3:.1f}-{a1 * 1e3:.1f} µs)", flush=True)
        del dst
    table = "\n".join(lines)
    print()
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
