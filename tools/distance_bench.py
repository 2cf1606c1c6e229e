#!/usr/bin/env python3
"""ec_distance at 4096², 16384² and a 16384 x 2048 strip (dev tool): target densities 50 %, 1 % and a single target; f64, u32 and the
mask-only form; the workspace from the library's pool.  Beside each time the byte floor of the call (the mask read, g written by the
down sweep, read and written by the up sweep and read by the row scan, one stack entry pair written and read per cell, the output
written) at 8 TB/s.  Two mask sets alternate; timing is by device events around a block of calls after a warm-up call, the figure
is the median of `--blocks` blocks, the spread the least and the greatest.  At 4096² the same raster goes through
scipy.ndimage.distance_transform_edt once (one CPU thread) and `within(cols, 7)` is set beside seven chained `dilate((1, 1))` and one
`dilate((7, 7))` — they compute different shapes.  The two kernels of a call are told apart by a kernel trace of this tool
(`--trace`: one call per configuration, in the order printed), not here.

    python tools/distance_bench.py [--blocks 5] [--calls 3] [--sides 64] [--workspace caller] [--out profiles/distance/distance_times.md] [--trace]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "erased-cells_amd", "python"))

PEAK_BYTES_PER_S = 8e12
SHAPES = ((4096, 4096), (16384, 16384), (16384, 2048))   # (cols, rows)
DENSITIES = (("50 %", 50), ("1 %", 1), ("single", None))
FORMS = (("f64", 9, True, True), ("u32", 2, True, True), ("mask only", 2, False, True))


def seven_dilations(mask, cols):
    for _ in range(7):
        mask = mask.dilate(cols, (1, 1))
    return mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed block")
    ap.add_argument("--sides", type=int, nargs="+", help="square rasters of these sides instead of the three shapes (a small one times the call's fixed cost)")
    ap.add_argument("--workspace", choices=("pool", "caller"), default="pool", help="the library's pool, or one block of the caller's")
    ap.add_argument("--out")
    ap.add_argument("--trace", action="store_true", help="one call per configuration and nothing else: for a kernel trace")
    args = ap.parse_args()

    import numpy as np
    import torch

    import erased_cells_hip as ec

    torch.cuda.set_device(0)
    ec.init(0)
    L, chk = ec.lib(), ec._ffi.check
    stream = torch.cuda.current_stream().cuda_stream
    ec.set_stream(stream)
    lines = []

    def say(text=""):
        lines.append(text)
        print(text, flush=True)

    def masks_of(cols, rows, pct):
        n = cols * rows
        out = []
        for k in range(2):
            if pct is None:
                m = ec.Mask.fill(n, False)
                m.put((rows // 3) * cols + (2 * cols) // 3 + k, True)
            else:
                m = ec.Mask.empty(n)
                chk(L.ec_synth_mask(m.mem.ptr, n, 0xD157 + k, 0, 100 - pct, stream))   # set where the hash % 100 >= 100 - pct
            out.append(m)
        return out

    def timed(fn):
        fn(0)
        torch.cuda.synchronize()
        t = []
        for _ in range(args.blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for c in range(args.calls):
                fn(c % 2)
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) / args.calls)
        return statistics.median(t), min(t), max(t)

    shapes = [(s, s) for s in args.sides] if args.sides else SHAPES
    say(f"ec_distance, workspace: {args.workspace}; ms per call: median of {args.blocks} blocks of {args.calls} calls (least - greatest); floor = algorithmic bytes at 8 TB/s")
    say()
    say("| cols x rows | targets | form | ms | floor ms | time / floor | Mcells/s |")
    say("|---|---|---|---|---|---|---|")
    for cols, rows in shapes:
        n = cols * rows
        dst = ec.CellBuffer.empty(n, ec.Float64)
        dm = ec.Mask.empty(n)
        block = ec.CellBuffer.empty(L.ec_distance_workspace_bytes(cols, rows), ec.UInt8) if args.workspace == "caller" else None
        ws = block.mem.ptr if block else None
        for dname, pct in DENSITIES:
            masks = masks_of(cols, rows, pct)
            for fname, ct, values, want_mask in FORMS:
                def call(k, ct=ct, values=values, masks=masks):
                    chk(L.ec_distance(masks[k].mem.ptr, cols, rows, 0xFFFFFFFF if values else 49, ct, dst.mem.ptr if values else None, dm.mem.ptr, ws, stream))
                if args.trace:
                    call(0)
                    torch.cuda.synchronize()
                    say(f"| {cols} x {rows} | {dname} | {fname} | traced |")
                    continue
                med, lo, hi = timed(call)
                cell = (8 if ct == 9 else 4) if values else 0
                floor_bytes = n * (1 + 2 + 4 + 2 + 8 + cell + 1)   # mask; g down; g up (read, write); g rows; s, t written and read; values; mask bytes
                floor = floor_bytes / PEAK_BYTES_PER_S * 1e3
                say(f"| {cols} x {rows} | {dname} | {fname} | {med:.2f} ({lo:.2f} - {hi:.2f}) | {floor:.3f} | {med / floor:.0f} | {n / med / 1e3:.0f} |")
            if (cols, rows) == (4096, 4096) and not args.trace:
                from scipy import ndimage
                host = masks[0].to_numpy().reshape(rows, cols)
                t0 = time.perf_counter()
                ref = ndimage.distance_transform_edt(host == 0) if host.any() else None
                cpu = time.perf_counter() - t0
                got = masks[0].distance(cols).buffer().to_numpy().reshape(rows, cols)
                same = ref is not None and bool(np.array_equal(np.rint(ref ** 2), np.rint(got ** 2)))
                say(f"| 4096 x 4096 | {dname} | scipy.ndimage.distance_transform_edt, one CPU thread | {cpu * 1e3:.0f} | | | {n / cpu / 1e6:.0f} | squared distances equal: {same}")
        if not args.trace:
            m = masks_of(cols, rows, 1)
            rows_ = []
            for name, fn in (("within(cols, 7)", lambda k: m[k].within(cols, 7)),
                             ("7 x dilate((1, 1))", lambda k: seven_dilations(m[k], cols)),
                             ("dilate((7, 7))", lambda k: m[k].dilate(cols, (7, 7)))):
                med, lo, hi = timed(fn)
                rows_.append(f"{name} {med:.2f} ms ({lo:.2f} - {hi:.2f})")
            say(f"| {cols} x {rows} | 1 % | " + " ; ".join(rows_) + " |")
        del dst, dm, block
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
