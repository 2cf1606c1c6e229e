#!/usr/bin/env python3
"""What tools/zonal_bench.py and tools/zonal_table_bench.py leave out of a comparison of two builds of the zonal families (dev tool).

One process times the library EC_HIP_LIB names (default: the tree's), so two builds are compared by running it by turns:

  1. 1-byte values: ec_zonal_stats_device and ec_zonal_table_device on UInt8 values with a mask at side² cells (default 16384²),
     UInt8 zones, 256 coherent zones (16 x 16 blocks) and zones[i] = hash(i) % 256, and Int32 zones of 4096 square blocks for the
     table call — the other two tools time UInt16 and Float64 values only, and the kernels of 1-byte values (16 cells a group) are
     the ones with the most registers.  Device events around blocks of calls after a warm-up; median, least and greatest block.
  2. the host cost of a call: n = 1024 cells of UInt16 with a mask, 16 UInt8 zones, a 16-cell Float64 table; the two device forms,
     the two synchronous forms and the two gathers; 200 warm-up calls, then 9 blocks of back-to-back calls on the default stream
     with one ec_stream_sync per block, wall time over calls.  At this size the figure is host and queue together.

    EC_HIP_LIB=<library> python tools/zonal_frame_bench.py [--side 16384] [--blocks 5] [--calls 5]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "erased-cells_amd", "python"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import erased_cells_hip as ec  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=16384)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    side = args.side
    n = side * side
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
        return e0.elapsed_time(e1) / calls

    # 1. 1-byte values with a mask
    u8, msk = ec.CellBuffer.empty(n, ec.UInt8), ec.Mask.empty(n)
    chk(L.ec_synth_fill(ec.UInt8, u8.mem.ptr, n, 0x20A0, 0, 0, 255, stream))
    chk(L.ec_synth_mask(msk.mem.ptr, n, 0x20B0, 0, 30, stream))
    step = max(1, side // 16)
    idx = np.minimum(np.arange(side) // step, 15).astype(np.uint8)
    coherent = ec.CellBuffer.from_vec(((idx * 16)[:, None] + idx[None, :]).ravel())
    hashed = ec.CellBuffer.empty(n, ec.UInt8)
    chk(L.ec_synth_fill(ec.UInt8, hashed.mem.ptr, n, 0x20C0, 0, 0, 255, stream))
    b64 = np.arange(side) // max(1, side // 64)
    blocks4096 = ec.CellBuffer.from_vec((b64[:, None] * 64 + b64[None, :]).astype(np.int32).ravel())
    out = ec.DeviceMem(4096 * 64)
    ws_lds = ec.DeviceMem(L.ec_zonal_workspace_bytes(256))
    ws_tab = ec.DeviceMem(L.ec_zonal_table_workspace_bytes(ec.UInt8, 4096))

    def stats(zones):
        return lambda: chk(L.ec_zonal_stats_device(ec.UInt8, u8.mem.ptr, msk.mem.ptr, zones.ct, zones.mem.ptr, n, 256, out.ptr, ws_lds.ptr, stream))

    def table(zones, nz):
        return lambda: chk(L.ec_zonal_table_device(ec.UInt8, u8.mem.ptr, msk.mem.ptr, zones.ct, zones.mem.ptr, n, nz, out.ptr, ws_tab.ptr, stream))

    rows = (("ec_zonal_stats_device, u8 masked, 256 coherent zones", stats(coherent)), ("ec_zonal_stats_device, u8 masked, hash(i) % 256", stats(hashed)),
            ("ec_zonal_table_device, u8 masked, 256 coherent zones", table(coherent, 256)), ("ec_zonal_table_device, u8 masked, hash(i) % 256", table(hashed, 256)),
            ("ec_zonal_table_device, u8 masked, 4096 block zones (i32)", table(blocks4096, 4096)))
    for _, fn in rows:
        block(fn, 1)
    t = {name: [] for name, _ in rows}
    for _ in range(args.blocks):
        for name, fn in rows:
            t[name].append(block(fn, args.calls))
    for name, _ in rows:
        print(f"BYTE | {name} | {statistics.median(t[name]):.3f} ms | {min(t[name]):.3f}-{max(t[name]):.3f}", flush=True)

    # 2. the host cost of a call
    m, nz = 1024, 16
    rng = np.random.default_rng(7)
    v = ec.CellBuffer.from_vec(rng.integers(0, 65535, m).astype(np.uint16))
    z = ec.CellBuffer.from_vec(rng.integers(0, nz, m).astype(np.uint8))
    vm = ec.Mask.new(rng.integers(0, 2, m).astype(bool))
    tab = ec.CellBuffer.from_vec(np.arange(nz, dtype=np.float64))
    dst, dm = ec.CellBuffer.empty(m, ec.Float64), ec.Mask.empty(m)
    recs = ec.DeviceMem(nz * 64)
    ws1, ws2 = ec.DeviceMem(L.ec_zonal_workspace_bytes(nz)), ec.DeviceMem(L.ec_zonal_table_workspace_bytes(ec.UInt16, nz))
    host = (E.EcStats * nz)()
    calls = {
        "ec_zonal_stats_device": lambda: L.ec_zonal_stats_device(ec.UInt16, v.mem.ptr, vm.mem.ptr, ec.UInt8, z.mem.ptr, m, nz, recs.ptr, ws1.ptr, stream),
        "ec_zonal_table_device": lambda: L.ec_zonal_table_device(ec.UInt16, v.mem.ptr, vm.mem.ptr, ec.UInt8, z.mem.ptr, m, nz, recs.ptr, ws2.ptr, stream),
        "ec_zonal_stats_compute": lambda: L.ec_zonal_stats_compute(ec.UInt16, v.mem.ptr, vm.mem.ptr, ec.UInt8, z.mem.ptr, m, nz, host, stream),
        "ec_zonal_table_compute": lambda: L.ec_zonal_table_compute(ec.UInt16, v.mem.ptr, vm.mem.ptr, ec.UInt8, z.mem.ptr, m, nz, host, stream),
        "ec_zonal_broadcast": lambda: L.ec_zonal_broadcast(ec.UInt8, z.mem.ptr, m, nz, ec.Float64, tab.mem.ptr, dst.mem.ptr, dm.mem.ptr, stream),
        "ec_zonal_lookup": lambda: L.ec_zonal_lookup(ec.UInt8, z.mem.ptr, m, nz, ec.Float64, tab.mem.ptr, dst.mem.ptr, dm.mem.ptr, stream),
    }
    for name, fn in calls.items():
        per = 300 if "compute" in name else 2000
        for _ in range(200):
            chk(fn())
        chk(L.ec_stream_sync(stream))
        took = []
        for _ in range(9):
            t0 = time.perf_counter()
            for _ in range(per):
                fn()
            chk(L.ec_stream_sync(stream))
            took.append((time.perf_counter() - t0) / per * 1e6)
        chk(fn())
        print(f"HOSTCOST | {name} | {statistics.median(took):.3f} us | {min(took):.3f}-{max(took):.3f}", flush=True)


if __name__ == "__main__":
    main()
