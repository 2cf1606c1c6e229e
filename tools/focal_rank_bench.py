#!/usr/bin/env python3
"""ec_focal_rank (the median) and ec_focal_majority beside ec_focal MIN at the same radius and cell type (dev tool).

ec_focal MIN moves the same bytes through the same stage — every cell read once from HBM, the halo from LDS, one cell of the same type
written — so it is the floor the sort sits on: the ratio to it is what the sorting network costs.  At side² cells (default 8192²) for
u8, u16 and f32 cells, 3 x 3, 5 x 5 and 7 x 7 footprints (the 16-, 32- and 64-word networks), unmasked and masked.  In one process:
four operand-and-output sets are filled on the device and every entry point runs over them in rotation, so that no byte of a call
is still in the 256 MiB Infinity Cache.  Timing is by device events around whole rotations, after a warm-up of every shape; the
entry points of a row alternate, block after block, and the per-call figure is the median over the blocks, the spread its least and
greatest block.  Fraction of the byte roofline = algorithmic bytes (every cell and mask byte read once, every output cell and mask
byte written once) / time / 8 TB/s.

    python tools/focal_rank_bench.py [--side 8192] [--blocks 5] [--min-ms 40] [--out profiles/focal/focal_rank.md]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "erased-cells_amd", "python"))

PEAK_BYTES_PER_S = 8e12
SETS = 4
RADII = (1, 2, 3)   # 3 x 3, 5 x 5, 7 x 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=8192)
    ap.add_argument("--blocks", type=int, default=5, help="timed blocks per entry point (the median is reported)")
    ap.add_argument("--min-ms", type=float, default=40.0, help="least device time of one timed block")
    ap.add_argument("--out", help="also write the table to this file")
    args = ap.parse_args()

    import torch

    import erased_cells_hip as ec

    side = args.side
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
        """(median, least, greatest) ms per call of each of `fns`, alternating block after block"""
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

    # the masks: a u8 fill of 0 .. 255 compared with 25 — about nine cells in ten valid, holes everywhere
    masks = [fill(ec.UInt8, 0xA0 + k, 0, 255).compare(">=", 25) for k in range(SETS)]
    out_masks = [ec.Mask.empty(n) for _ in range(SETS)]
    sources = {"u8": (ec.UInt8, [fill(ec.UInt8, 0xF0 + k, 0, 255) for k in range(SETS)]),
               "u16": (ec.UInt16, [fill(ec.UInt16, 0xF4 + k, 0, 65535) for k in range(SETS)]),
               "f32": (ec.Float32, [fill(ec.Float32, 0xF8 + k, -300.0, 300.0) for k in range(SETS)])}
    lines = [f"ec_focal_rank 1/2 LOWER (the median) and ec_focal_majority beside ec_focal MIN, {side}² cells; times are medians of {args.blocks} blocks "
             f"of at least {args.min_ms:.0f} ms over {SETS} rotating operand sets, (least - greatest) behind them", "",
             "| cells | footprint | masked | ec_focal MIN µs | median µs | majority µs | median Gcells/s | majority Gcells/s | median / MIN | majority / MIN | "
             "MIN share of 8 TB/s | median share | majority share |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, (ct, cells) in sources.items():
        w = ec.size_of(ct)
        outs = [ec.CellBuffer.empty(n, ct) for _ in range(SETS)]
        for r in RADII:
            for masked in (False, True):
                sm = [m.mem.ptr if masked else None for m in masks]
                dm = [m.mem.ptr if masked else None for m in out_masks]

                def floor(k, ct=ct, cells=cells, outs=outs, r=r, sm=sm, dm=dm):
                    chk(L.ec_focal(E.EC_FOCAL_MIN, ct, cells[k].mem.ptr, sm[k], side, side, r, r, 0, outs[k].mem.ptr, dm[k], stream))

                def median(k, ct=ct, cells=cells, outs=outs, r=r, sm=sm, dm=dm):
                    chk(L.ec_focal_rank(ct, cells[k].mem.ptr, sm[k], side, side, r, r, 1, 2, E.EC_RANK_LOWER, 0, outs[k].mem.ptr, dm[k], stream))

                def majority(k, ct=ct, cells=cells, outs=outs, r=r, sm=sm, dm=dm):
                    chk(L.ec_focal_majority(ct, cells[k].mem.ptr, sm[k], side, side, r, r, 0, outs[k].mem.ptr, dm[k], stream))

                (a, a0, a1), (b, b0, b1), (c, c0, c1) = measure([floor, median, majority])
                moved = n * (2 * w + (2 if masked else 0))
                share = lambda ms: moved / (ms * 1e-3) / PEAK_BYTES_PER_S
                us = lambda t, t0, t1: f"{t * 1e3:.1f} ({t0 * 1e3:.1f} - {t1 * 1e3:.1f})"
                lines.append(f"| {name} | {2 * r + 1} x {2 * r + 1} | {'yes' if masked else 'no'} | {us(a, a0, a1)} | {us(b, b0, b1)} | {us(c, c0, c1)} | "
                             f"{n / (b * 1e-3) / 1e9:.2f} | {n / (c * 1e-3) / 1e9:.2f} | {b / a:.2f} | {c / a:.2f} | {share(a):.3f} | {share(b):.3f} | {share(c):.3f} |")
                print(lines[-1], flush=True)
    table = "\n".join(lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
