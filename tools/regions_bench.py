#!/usr/bin/env python3
"""ec_regions at 4096² and 16384² on u8 class rasters (dev tool): `all` (one class), `random59` (two classes, the one at the percolation
threshold), three-class random and a spiral (one path of width 1 from the corner to the centre, its root in tile 0); both
connectivities, DENSE numbering, without a sieve and with min_cells = 20; labels, mask bytes and K out; the workspace from the
library's pool.  Beside each time the byte floor of the call, taken as 1 B read + 5 B written per cell at 8 TB/s.  Timing is by device
events around a block of calls after a warm-up call, the figure is the median of `--blocks` blocks, the spread the least and the
greatest.  At 4096² the same raster goes through scipy.ndimage.label once per class (one CPU thread).  The kernels of a call are told
apart by a kernel trace of this tool (`--trace`: one call per configuration, in the order printed), not here.

    python tools/regions_bench.py [--blocks 5] [--calls 3] [--sides 4096 16384] [--out profiles/regions/regions_times.md] [--trace]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "erased-cells_amd", "python"))

PEAK_BYTES_PER_S = 8e12
PATTERNS = ("all", "random59", "random3", "spiral")


def spiral(np, side):
    """the rings of even index, each opened below its top-left corner and tied to the next one inside it: one path, 4-connected"""
    i = np.arange(side, dtype=np.int32)
    edge = np.minimum(i, side - 1 - i)
    m = np.empty((side, side), np.uint8)
    for at in range(0, side, 1024):
        m[at:at + 1024] = np.minimum(edge[at:at + 1024, None], edge[None, :]) % 2 == 0
    for r in range(0, (side - 1) // 2 - 1, 2):
        m[r + 1, r] = 0
        m[r + 2, r + 1] = 1
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed block")
    ap.add_argument("--sides", type=int, nargs="+", default=[4096, 16384])
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

    def raster(side, pattern):
        n = side * side
        buf = ec.CellBuffer.empty(n, ec.UInt8)
        if pattern == "all":
            one = ec.CellValue(ec.UInt8, 1).to_ec()
            chk(L.ec_fill(ec.UInt8, buf.mem.ptr, n, ctypes.byref(one), stream))
        elif pattern == "random59":
            chk(L.ec_synth_mask(buf.mem.ptr, n, 0x5E59, 0, 41, stream))      # 1 where the hash % 100 >= 41
        elif pattern == "random3":
            chk(L.ec_synth_fill(ec.UInt8, buf.mem.ptr, n, 0xC1A5, 0, 0.0, 2.0, stream))
        else:
            buf = ec.CellBuffer.from_vec(spiral(np, side).ravel())
        return buf

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(args.blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _c in range(args.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) / args.calls)
        return statistics.median(t), min(t), max(t)

    say(f"ec_regions, u8 classes, DENSE, labels + mask bytes + K, workspace: {args.workspace}; ms per call: median of {args.blocks} blocks of {args.calls} calls "
        "(least - greatest); floor = 1 B read + 5 B written per cell at 8 TB/s")
    say()
    say("| side | pattern | connectivity | min_cells | K | ms | floor ms | time / floor | Mcells/s |")
    say("|---|---|---|---|---|---|---|---|---|")
    for side in args.sides:
        n = side * side
        dst, dm, k = ec.CellBuffer.empty(n, ec.Int32), ec.Mask.empty(n), ec.CellBuffer.empty(1, ec.UInt64)
        floor = n * 6 / PEAK_BYTES_PER_S * 1e3
        block = ec.CellBuffer.empty(L.ec_regions_workspace_bytes(side, side), ec.UInt8) if args.workspace == "caller" else None
        ws = block.mem.ptr if block else None
        for pattern in PATTERNS:
            src = raster(side, pattern)
            for c in (4, 8):
                for min_cells in (0, 20):
                    def call(c=c, min_cells=min_cells):
                        chk(L.ec_regions(ec.UInt8, src.mem.ptr, None, side, side, c, 1, min_cells, dst.mem.ptr, dm.mem.ptr, k.mem.ptr, ws, stream))
                    if args.trace:
                        call()
                        torch.cuda.synchronize()
                        say(f"| {side} | {pattern} | {c} | {min_cells} | traced |")
                        continue
                    med, lo, hi = timed(call)
                    kept = int(k.to_numpy()[0])
                    say(f"| {side} | {pattern} | {c} | {min_cells} | {kept} | {med:.2f} ({lo:.2f} - {hi:.2f}) | {floor:.3f} | {med / floor:.0f} | {n / med / 1e3:.0f} |")
            if side == 4096 and not args.trace:
                from scipy import ndimage
                host = src.to_numpy().reshape(side, side)
                t0 = time.perf_counter()
                count = sum(ndimage.label(host == v)[1] for v in np.unique(host))
                cpu = time.perf_counter() - t0
                call(4, 0)
                torch.cuda.synchronize()
                say(f"| 4096 | {pattern} | 4 | 0 | {count} | scipy.ndimage.label per class, one CPU thread: {cpu * 1e3:.0f} | | | {n / cpu / 1e6:.0f} | K equal: {count == int(k.to_numpy()[0])}")
            del src
        del dst, dm, k, block
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
