#!/usr/bin/env python3
"""ec_zonal_stats_device beside its floor and beside the route it replaces (dev tool).

At side² cells (default 16384²) of UInt16 values with a mask and a UInt8 zone raster, in one process:

  1. one zonal pass over 256 coherent zones (blocks of side / 16 cells squared) against ec_stats_device on the same value and mask
     bytes — the zonal pass reads one byte per cell more, so that is its floor;
  2. one zonal pass against the status quo, n_zones x (ec_compare_scalar of the zone raster under the mask + masked
     ec_stats_device), for n_zones = 4, 32 and 256 (the same blocks, merged);
  3. the adversarial raster, zones[i] = hash(i) % 256 (every wave slot holds about 64 distinct ids), against the coherent one.

Every operand byte comes from HBM: one set is 1 GiB, and `--sets` (default 2) sets are used in rotation.  Timing is by device
events around whole rotations, after a warm-up of every shape; the per-call figure is the median over the blocks, with the
least and the greatest beside it.  Share of peak = algorithmic bytes / time / 8 TB/s, every input byte read once.  The chain's
records and the zonal pass's are compared byte for byte at the end (UInt16 is the exact kind).

    python tools/zonal_bench.py [--side 16384] [--blocks 7] [--min-ms 60] [--sets 2] [--out zonal.md]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "erased-cells_amd", "python"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import erased_cells_hip as ec  # noqa: E402

PEAK_BYTES_PER_S = 8e12
ZONE_COUNTS = (4, 32, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=16384)
    ap.add_argument("--blocks", type=int, default=7, help="timed blocks per entry point (the median is reported)")
    ap.add_argument("--min-ms", type=float, default=60.0, help="least device time of one timed block")
    ap.add_argument("--sets", type=int, default=2, help="operand sets used in rotation")
    ap.add_argument("--out", help="also write the tables to this file")
    args = ap.parse_args()
    side, sets = args.side, args.sets
    n = side * side
    torch.cuda.set_device(0)
    ec.init(0)
    L, chk, E = ec.lib(), ec._ffi.check, ec._ffi
    stream = torch.cuda.current_stream().cuda_stream
    ec.set_stream(stream)
    ct, zt = ec.UInt16, ec.UInt8

    # 256 zones as a 16 x 16 grid of blocks; 32 and 4 zones merge neighbouring ids
    step = max(1, side // 16)
    rows = (np.minimum(np.arange(side) // step, 15) * 16).astype(np.uint8)
    z256 = (rows[:, None] + np.minimum(np.arange(side) // step, 15).astype(np.uint8)[None, :]).ravel()
    coherent = {256: z256, 32: z256 // 8, 4: z256 // 64}
    values, masks, zones, hashed = [], [], {k: [] for k in ZONE_COUNTS}, []
    for s in range(sets):
        v, m, h = ec.CellBuffer.empty(n, ct), ec.Mask.empty(n), ec.CellBuffer.empty(n, zt)
        chk(L.ec_synth_fill(ct, v.mem.ptr, n, 0x20A0 + s, 0, 0, 65535, stream))
        chk(L.ec_synth_mask(m.mem.ptr, n, 0x20B0 + s, 0, 30, stream))
        chk(L.ec_synth_fill(zt, h.mem.ptr, n, 0x20C0 + s, 0, 0, 255, stream))
        values.append(v)
        masks.append(m)
        hashed.append(h)
        for k in ZONE_COUNTS:
            zones[k].append(ec.CellBuffer.from_vec(coherent[k]))
    recs = [ec.DeviceMem(256 * 64) for _ in range(sets)]
    work = [ec.DeviceMem(L.ec_zonal_workspace_bytes(256)) for _ in range(sets)]
    zmask = [ec.Mask.empty(n) for _ in range(sets)]
    chain_recs = [ec.DeviceMem(256 * 64) for _ in range(sets)]

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

    def zonal(raster, k):
        def fn(s):
            chk(L.ec_zonal_stats_device(ct, values[s].mem.ptr, masks[s].mem.ptr, zt, raster[s].mem.ptr, n, k, recs[s].ptr, work[s].ptr, stream))
        return fn

    def whole(s):
        chk(L.ec_stats_device(ct, values[s].mem.ptr, masks[s].mem.ptr, n, recs[s].ptr, stream))

    def chain(k):
        """the parent's route: per zone, the cells of the zone as a mask (under the values' mask), then the masked statistics"""
        ids = [ec.CellValue(zt, z).to_ec() for z in range(k)]

        def fn(s):
            for z in range(k):
                chk(L.ec_compare_scalar(E.EC_CMP_EQ, zt, zones[k][s].mem.ptr, masks[s].mem.ptr, n, C.byref(ids[z]), zmask[s].mem.ptr, stream))
                chk(L.ec_stats_device(ct, values[s].mem.ptr, zmask[s].mem.ptr, n, chain_recs[s].ptr + 64 * z, stream))
        return fn

    def share(per_cell, ms):
        return n * per_cell / (ms * 1e-3) / PEAK_BYTES_PER_S

    def row(label, per_cell, t, ratio=""):
        return f"| {label} | {per_cell} | {t[0] * 1e3:.1f} | {share(per_cell, t[0]):.3f} | {t[1] * 1e3:.1f}-{t[2] * 1e3:.1f} | {ratio} |"

    lines = [f"ec_zonal_stats_device, UInt16 values with a mask and a UInt8 zone raster, {side}² cells, {sets} sets in rotation", ""]
    head = ["| call | algorithmic B / cell | µs | share of 8 TB/s | spread µs | ratio |", "|---|---|---|---|---|---|"]

    z_coh, z_hash = zonal(zones[256], 256), zonal(hashed, 256)
    t_coh, t_whole, t_hash = measure([z_coh, whole, z_hash])
    lines += ["1. against ec_stats_device (the floor: one byte per cell less), and 3. the adversarial raster", ""] + head
    lines.append(row("zonal, 256 coherent zones", 4, t_coh, f"{t_coh[0] / t_whole[0]:.2f} x ec_stats_device"))
    lines.append(row("ec_stats_device, masked", 3, t_whole))
    lines.append(row("zonal, zones[i] = hash(i) % 256", 4, t_hash, f"{t_hash[0] / t_coh[0]:.2f} x the coherent raster"))
    for line in lines[-3:]:
        print(line, flush=True)

    lines += ["", "2. against n_zones x (ec_compare_scalar + masked ec_stats_device)", ""] + head
    for k in ZONE_COUNTS:
        one, ch = zonal(zones[k], k), chain(k)
        t_one, t_chain = measure([one, ch])
        lines.append(row(f"zonal, {k} zones", 4, t_one, f"chain / one pass {t_chain[0] / t_one[0]:.1f}"))
        lines.append(row(f"chain of {k} x (compare_scalar + stats)", k * (1 + 1 + 1 + 2 + 1), t_chain))
        for line in lines[-2:]:
            print(line, flush=True)
        # faster and different is not faster: the same records, byte for byte
        s = sets - 1
        one(s)
        ch(s)
        a, b = np.empty(k * 64, np.uint8), np.empty(k * 64, np.uint8)
        chk(L.ec_download(a.ctypes.data, recs[s].ptr, k * 64, stream))
        chk(L.ec_download(b.ctypes.data, chain_recs[s].ptr, k * 64, stream))
        same = bool((a == b).all())
        lines.append(f"| records of the one pass == records of the chain, {k} zones: {same} | | | | | |")
        assert same, f"the zonal pass and the chain disagree at {k} zones"
    table = "\n".join(lines)
    print()
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
