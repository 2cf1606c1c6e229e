#!/usr/bin/env python3
"""ec_composite as a share of the HBM peak, beside the chain of ec_masked_select calls it replaces (dev tool).

At side² cells (default 16384²) of UInt16 layers with masks, in one process: FIRST, MAX and MEAN over K = 8 layers, then over K = 4
and K = 16 to see how the rate moves with the batch loop.  The yardstick is the FIRST composite built the way a caller had to build
it before: K - 1 ec_masked_select calls (`or_else`, cloud fill), each re-reading and re-writing the running result and its mask, on
the same inputs, interleaved with the one-pass call block after block.  ec_masked_select is the parent commit's code unchanged;
`--baseline-lib` takes it from another build all the same.

Every operand byte comes from HBM: one set of K = 8 layers with masks is 6 GiB, far more than the 256 MiB Infinity Cache, and `--sets`
(default 2) such sets and outputs are used in rotation.  Timing is by device events around whole rotations, after a warm-up of every
shape; the per-call figure is the median over the blocks.  Share of peak = algorithmic bytes / time / 8 TB/s, with algorithmic bytes
per cell K * (w + 1) + result + mask [+ aux]: every layer and mask read once, every output written once.  For the chain the bytes it
moves are counted the same way from its entry points' streams: per call 2 w + 3 read, w + 1 written.

    python tools/composite_bench.py [--side 16384] [--blocks 7] [--min-ms 60] [--sets 2] [--baseline-lib OTHER.so] [--out composite.md]
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
KS = (8, 4, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=16384)
    ap.add_argument("--blocks", type=int, default=7, help="timed blocks per entry point (the median is reported)")
    ap.add_argument("--min-ms", type=float, default=60.0, help="least device time of one timed block")
    ap.add_argument("--sets", type=int, default=2, help="operand-and-output sets used in rotation")
    ap.add_argument("--baseline-lib", help="another build of the library: its ec_masked_select is the chain's")
    ap.add_argument("--out", help="also write the tables to this file")
    args = ap.parse_args()
    n, sets = args.side * args.side, args.sets
    torch.cuda.set_device(0)
    ec.init(0)
    L, chk, E = ec.lib(), ec._ffi.check, ec._ffi
    stream = torch.cuda.current_stream().cuda_stream
    ec.set_stream(stream)
    base = L
    if args.baseline_lib:
        base = C.CDLL(os.path.abspath(args.baseline_lib))
        base.ec_init.argtypes, base.ec_init.restype = [C.c_int32], C.c_int32
        base.ec_masked_select.restype, base.ec_masked_select.argtypes = E.SIGNATURES["ec_masked_select"]
        assert base.ec_init(0) == 0, "the baseline library did not initialise"
    ct, w, kmax = ec.UInt16, 2, max(KS)

    layers, masks = [], []
    for s in range(sets):
        ls, ms = [], []
        for k in range(kmax):
            a, m = ec.CellBuffer.empty(n, ct), ec.Mask.empty(n)
            chk(L.ec_synth_fill(ct, a.mem.ptr, n, 0xC0A0 + 64 * s + k, 0, 0, 65535, stream))
            chk(L.ec_synth_mask(m.mem.ptr, n, 0xC0B0 + 64 * s + k, 0, 40, stream))   # 40 % of every layer is cloud
            ls.append(a)
            ms.append(m)
        layers.append(ls)
        masks.append(ms)
    out16 = [ec.CellBuffer.empty(n, ct) for _ in range(sets)]
    out64 = [ec.CellBuffer.empty(n, ec.Float64) for _ in range(sets)]
    omask = [ec.Mask.empty(n) for _ in range(sets)]
    aux = [ec.CellBuffer.empty(n, ec.UInt8) for _ in range(sets)]
    lp = [(C.c_void_p * kmax)(*[a.mem.ptr for a in layers[s]]) for s in range(sets)]
    mp = [(C.c_void_p * kmax)(*[m.mem.ptr for m in masks[s]]) for s in range(sets)]

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
        """median ms per call of each of `fns`, alternating block after block"""
        est = {}
        for fn in fns:
            block(fn, 2)   # warm-up of every shape
            est[fn] = block(fn, 2)
        rot = {fn: max(2, int(args.min_ms / (est[fn] * sets)) + 1) for fn in fns}
        t = {fn: [] for fn in fns}
        for _ in range(args.blocks):
            for fn in fns:
                t[fn].append(block(fn, rot[fn]))
        return [(statistics.median(t[fn]), min(t[fn]), max(t[fn])) for fn in fns]

    def share(per_cell, ms):
        return n * per_cell / (ms * 1e-3) / PEAK_BYTES_PER_S

    def one_pass(op, k, with_aux):
        sums = op in (E.EC_COMPOSITE_SUM, E.EC_COMPOSITE_MEAN)

        def fn(s):
            chk(L.ec_composite(op, ct, lp[s], mp[s], k, n, 1, (out64 if sums else out16)[s].mem.ptr, omask[s].mem.ptr,
                               aux[s].mem.ptr if with_aux else None, stream))
        return fn, k * (w + 1) + (8 if sums else w) + 1 + (1 if with_aux else 0)

    def chain(k):
        """the FIRST composite as a caller built it before: out = L0.or_else(L1) ... or_else(L(k-1)), the running result patched in place"""
        def fn(s):
            a, am = layers[s][0].mem.ptr, masks[s][0].mem.ptr
            for j in range(1, k):
                st = base.ec_masked_select(ct, a, am, layers[s][j].mem.ptr, masks[s][j].mem.ptr, am, n, out16[s].mem.ptr, omask[s].mem.ptr, stream)
                assert st == 0, st
                a, am = out16[s].mem.ptr, omask[s].mem.ptr
        return fn, (k - 1) * ((2 * w + 3) + (w + 1))

    which = "the baseline build" if args.baseline_lib else "this build (the parent's code, unchanged)"
    lines = [f"ec_composite over K UInt16 layers with masks, {args.side}² cells, {sets} sets in rotation; the chain is K - 1 ec_masked_select calls of {which}", "",
             "| K | call | algorithmic B / cell | µs | share of 8 TB/s | spread µs | chain / one pass |", "|---|---|---|---|---|---|---|"]
    for k in KS:
        first, b_first = one_pass(E.EC_COMPOSITE_FIRST, k, False)
        first_aux, b_first_aux = one_pass(E.EC_COMPOSITE_FIRST, k, True)
        mx, b_max = one_pass(E.EC_COMPOSITE_MAX, k, True)
        mean, b_mean = one_pass(E.EC_COMPOSITE_MEAN, k, True)
        ch, b_chain = chain(k)
        res = measure([first, ch, first_aux, mx, mean])
        t_first, t_chain = res[0][0], res[1][0]
        for label, per_cell, (t, lo, hi) in (("FIRST", b_first, res[0]), (f"chain of {k - 1} ec_masked_select", b_chain, res[1]),
                                             ("FIRST + aux", b_first_aux, res[2]), ("MAX + aux", b_max, res[3]), ("MEAN + aux", b_mean, res[4])):
            ratio = f"{t_chain / t_first:.2f}" if label == "FIRST" else ""
            lines.append(f"| {k} | {label} | {per_cell} | {t * 1e3:.1f} | {share(per_cell, t):.3f} | {lo * 1e3:.1f}-{hi * 1e3:.1f} | {ratio} |")
            print(lines[-1], flush=True)
    # faster and different is not faster: the chain and the one pass agree on the last set
    s = sets - 1
    chain(KS[0])[0](s)
    ch_cells, ch_mask = out16[s].to_numpy().copy(), omask[s].to_numpy().copy()
    one_pass(E.EC_COMPOSITE_FIRST, KS[0], False)[0](s)
    same = bool((out16[s].to_numpy()[ch_mask != 0] == ch_cells[ch_mask != 0]).all() and (omask[s].to_numpy() == ch_mask).all())
    lines += ["", f"FIRST over K = {KS[0]} equals the chain on every valid cell and in the mask: {same}"]
    table = "\n".join(lines)
    print()
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")
    assert same, "the one-pass FIRST composite and the chain of ec_masked_select disagree"


if __name__ == "__main__":
    main()
