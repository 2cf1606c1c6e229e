#!/usr/bin/env python3
"""ec_composite_rank beside ec_composite MAX on the same stack: what the selection costs (dev tool).

At side² cells (default 16384²), in one process: the lower median (1/2 LOWER) of K masked layers with aux, against ec_composite MAX of
the same stack with the same outputs — the call that moves the same bytes ((cell + 1) K in, cell + 2 out) and is one compare per
layer, so the ratio is the price of the selection.  UInt16 at K = 4, 8, 16, 32, 64; Float32 and Float64 at K = 8 and 32.

Every operand byte comes from HBM: the smallest stack here is 3 GiB, twelve times the Infinity Cache, so one operand set is used.
Timing is by device events around whole blocks, after a warm-up of every shape; the two calls alternate block after block, and the
per-call figure is the median over the blocks, with the least and the greatest beside it.  The first 2^20 cells of every median are
checked against tests/composite_rank_ref.py at the end.

    python tools/composite_rank_bench.py [--side 16384] [--blocks 5] [--min-ms 60] [--out composite_rank.md]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "erased-cells_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import composite_rank_ref as R  # noqa: E402
import erased_cells_hip as ec  # noqa: E402

PEAK_BYTES_PER_S = 8e12
CASES = ((ec.UInt16, (4, 8, 16, 32, 64), 0, 65535), (ec.Float32, (8, 32), 0.0, 1.0), (ec.Float64, (8, 32), 0.0, 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=16384)
    ap.add_argument("--blocks", type=int, default=5, help="timed blocks per entry point (the median is reported)")
    ap.add_argument("--min-ms", type=float, default=60.0, help="least device time of one timed block")
    ap.add_argument("--out", help="also write the table to this file")
    args = ap.parse_args()
    n = args.side * args.side
    torch.cuda.set_device(0)
    ec.init(0)
    L, chk, E = ec.lib(), ec._ffi.check, ec._ffi
    stream = torch.cuda.current_stream().cuda_stream
    ec.set_stream(stream)

    def block(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls  # ms per call

    def measure(fns):
        """(median, least, greatest) ms per call of each of `fns`, alternating block after block"""
        est = {}
        for fn in fns:
            block(fn, 1)   # warm-up of every shape
            est[fn] = block(fn, 1)
        calls = {fn: max(1, int(args.min_ms / est[fn]) + 1) for fn in fns}
        t = {fn: [] for fn in fns}
        for _ in range(args.blocks):
            for fn in fns:
                t[fn].append(block(fn, calls[fn]))
        return [(statistics.median(t[fn]), min(t[fn]), max(t[fn])) for fn in fns]

    lines = [f"ec_composite_rank 1/2 LOWER against ec_composite MAX on the same masked stack, both with aux, {args.side}² cells", "",
             "| cells | K | bucket | cells per lane | algorithmic B / cell | MAX µs | share of 8 TB/s | spread µs | median µs | share of 8 TB/s | spread µs | x MAX |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    worst = (0.0, "")
    for t, heights, lo, hi in CASES:
        name, w = ec.CT_NAMES[t], ec.NP_DTYPES[t].itemsize
        layers, masks = [], []
        for k in range(max(heights)):
            if t == ec.Float64:   # the generator has no f64 form: f32 cells widened
                f = ec.CellBuffer.empty(n, ec.Float32)
                chk(L.ec_synth_fill(ec.Float32, f.mem.ptr, n, 0x3A00 + k, 0, lo, hi, stream))
                v = f.convert(ec.Float64)
                del f
            else:
                v = ec.CellBuffer.empty(n, t)
                chk(L.ec_synth_fill(t, v.mem.ptr, n, 0x3A00 + k, 0, lo, hi, stream))
            m = ec.Mask.empty(n)
            chk(L.ec_synth_mask(m.mem.ptr, n, 0x3B00 + k, 0, 30, stream))
            layers.append(v)
            masks.append(m)
        dst, dmask, aux = ec.CellBuffer.empty(n, t), ec.Mask.empty(n), ec.CellBuffer.empty(n, ec.UInt8)
        for k in heights:
            lp = (C.c_void_p * k)(*[b.mem.ptr for b in layers[:k]])
            mp = (C.c_void_p * k)(*[m.mem.ptr for m in masks[:k]])

            def comp_max():
                chk(L.ec_composite(E.EC_COMPOSITE_MAX, t, lp, mp, k, n, 1, dst.mem.ptr, dmask.mem.ptr, aux.mem.ptr, stream))

            def median():
                chk(L.ec_composite_rank(t, lp, mp, k, n, 1, 2, E.EC_RANK_LOWER, 1, dst.mem.ptr, dmask.mem.ptr, aux.mem.ptr, stream))

            t_max, t_med = measure([comp_max, median])
            per_cell = (w + 1) * k + w + 2
            share = lambda tt: n * per_cell / (tt[0] * 1e-3) / PEAK_BYTES_PER_S
            ratio = t_med[0] / t_max[0]
            g = R.group_cells(t, k)
            lines.append(f"| {name} | {k} | {R.bucket(k)} | {g} | {per_cell} | {t_max[0] * 1e3:.0f} | {share(t_max):.3f} | {t_max[1] * 1e3:.0f}-{t_max[2] * 1e3:.0f} | {t_med[0] * 1e3:.0f} | "
                         f"{share(t_med):.3f} | {t_med[1] * 1e3:.0f}-{t_med[2] * 1e3:.0f} | {ratio:.2f} |")
            print(lines[-1], flush=True)
            if ratio > worst[0]:
                worst = (ratio, f"{name}, K = {k}")
            # fast and wrong is not fast: the head of the median against the reference file
            head = 1 << 20
            median()
            got = [ec.buffer._download(dst.mem, ec.NP_DTYPES[t], head), ec.buffer._download(dmask.mem, np.dtype(np.uint8), head),
                   ec.buffer._download(aux.mem, np.dtype(np.uint8), head)]
            hl = [ec.buffer._download(b.mem, ec.NP_DTYPES[t], head) for b in layers[:k]]
            hm = [ec.buffer._download(m.mem, np.dtype(np.uint8), head) for m in masks[:k]]
            want = R.composite_rank(t, hl, hm, 1, 2, R.LOWER, 1)
            assert R.same_cells(got[0], want[0]).all() and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), \
                f"ec_composite_rank {name}, K = {k} differs from tests/composite_rank_ref.py"
        del layers, masks, dst, dmask, aux
    lines += ["", f"worst ratio: {worst[0]:.2f} x ec_composite MAX ({worst[1]}); every median's first 2^20 cells equal tests/composite_rank_ref.py"]
    table = "\n".join(lines)
    print()
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
