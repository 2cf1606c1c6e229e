#!/usr/bin/env python3
"""ec_stats_device against ec_min_max_keys on the same buffers (dev tool): what the moments cost on top of min/max.

For each cell type asked for (default u8 u16 u32 f32 f64) at side² cells (default 16384²), masked and unmasked, in one process:
four operand sets (cells and mask each) are filled on the device and both entry points run over them in rotation, so every byte
of every call comes from HBM and not from the Infinity Cache the previous call left warm.  Timing is by device events around whole
rotations, after a warm-up of every shape; the two entry points alternate, block after block, and the per-call figure is the
median over the blocks.  ec_min_max_keys is the baseline because it reads exactly the same bytes; the stats kernel does strictly
more arithmetic on them, so a ratio below 1 would be noise.  Share of peak = (cell bytes + mask bytes) / time / 8 TB/s.

    python tools/bench_stats.py [--side 16384] [--types u8 u16 u32 f32 f64] [--blocks 7] [--min-ms 60] [--bpc 0] [--out stats.md]

Under `rocprofv3 --kernel-trace --stats -- python tools/bench_stats.py --types u8 --blocks 2` the same loop gives per-kernel times
(k_stats_partials / k_stats_finalize against k_min_max_partials / k_min_max_finalize).  `--bpc 1` / `--bpc 2` halve and quarter
the waves resident per CU: a kernel short of bytes in flight slows down in proportion, one bound by instruction issue does not.
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
TYPES = {"u8": ec.UInt8, "u16": ec.UInt16, "u32": ec.UInt32, "f32": ec.Float32, "f64": ec.Float64,
         "i8": ec.Int8, "i16": ec.Int16, "i32": ec.Int32, "u64": ec.UInt64, "i64": ec.Int64}
# ec_synth_fill writes u8, u16 and f32; the other types are converted from the nearest of those
SYNTH = {ec.UInt8: ec.UInt8, ec.UInt16: ec.UInt16, ec.Float32: ec.Float32, ec.UInt32: ec.UInt16, ec.Float64: ec.Float32,
         ec.Int8: None, ec.Int16: ec.UInt8, ec.Int32: ec.UInt16, ec.UInt64: ec.UInt16, ec.Int64: ec.UInt16}
RANGE = {ec.UInt8: (0, 255), ec.UInt16: (0, 65535), ec.Float32: (-1000.0, 1000.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=16384)
    ap.add_argument("--types", nargs="+", default=["u8", "u16", "u32", "f32", "f64"], choices=sorted(TYPES))
    ap.add_argument("--blocks", type=int, default=7, help="timed blocks per entry point (the median is reported)")
    ap.add_argument("--min-ms", type=float, default=60.0, help="least device time of one timed block")
    ap.add_argument("--out", help="also write the table to this file")
    ap.add_argument("--bpc", type=int, default=0, help="reduce_bpc for both entry points (workgroups per CU; 0: as many as are resident)")
    args = ap.parse_args()
    n = args.side * args.side
    torch.cuda.set_device(0)
    ec.init(0)
    L, chk = ec.lib(), ec._ffi.check
    stream = torch.cuda.current_stream().cuda_stream
    ec.set_stream(stream)
    chk(L.ec_prepare_stream(stream))
    chk(L.ec_tune_set(b"reduce_bpc", args.bpc))
    keys = ec.DeviceMem(16)
    rec = ec.DeviceMem(64)

    def fill(ct, seed):
        src = SYNTH[ct]
        if src is None:
            raise SystemExit("no device-side generator for this type")
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

    lines = [f"| type | masked | ec_min_max_keys µs | ec_stats_device µs | ratio | min/max share of 8 TB/s | stats share of 8 TB/s |",
             "|---|---|---|---|---|---|---|"]
    for name in args.types:
        ct = TYPES[name]
        size = ec.size_of(ct)
        cells = [fill(ct, 0xBE00 + k) for k in range(SETS)]
        masks = [ec.Mask.empty(n) for _ in range(SETS)]
        for k, m in enumerate(masks):
            chk(L.ec_synth_mask(m.mem.ptr, n, 0xA500 + k, 0, 10, stream))
        for masked in (False, True):
            def min_max(k):
                chk(L.ec_min_max_keys(ct, cells[k].mem.ptr, masks[k].mem.ptr if masked else None, n, keys.ptr, stream))

            def stats(k):
                chk(L.ec_stats_device(ct, cells[k].mem.ptr, masks[k].mem.ptr if masked else None, n, rec.ptr, stream))

            # warm-up of both shapes, then size the blocks from a first estimate
            est = {}
            for fn in (min_max, stats):
                block(fn, 2)
                est[fn] = block(fn, 2)
            rot = {fn: max(2, int(args.min_ms / (est[fn] * SETS)) + 1) for fn in (min_max, stats)}
            t = {min_max: [], stats: []}
            for _ in range(args.blocks):  # alternating: drift of the clocks hits both alike
                for fn in (min_max, stats):
                    t[fn].append(block(fn, rot[fn]))
            a, b = statistics.median(t[min_max]), statistics.median(t[stats])
            moved = n * size + (n if masked else 0)
            share = lambda ms: moved / (ms * 1e-3) / PEAK_BYTES_PER_S  # noqa: E731
            lines.append(f"| {name} | {'yes' if masked else 'no'} | {a * 1e3:.1f} | {b * 1e3:.1f} | {b / a:.3f} | {share(a):.3f} | {share(b):.3f} |")
            print(lines[-1], f"  (spread min/max {min(t[min_max]) * 1e3:.1f}-{max(t[min_max]) * 1e3:.1f}, stats {min(t[stats]) * 1e3:.1f}-{max(t[stats]) * 1e3:.1f} µs)",
                  flush=True)
        del cells, masks
        torch.cuda.synchronize()
    table = "\n".join(lines)
    print()
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
