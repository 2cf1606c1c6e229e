#!/usr/bin/env python3
"""ec_zonal_table_device and ec_zonal_lookup beside the calls they replace or extend (dev tool).

At side² cells (default 16384²), UInt16 values with a mask and Float64 values without, in one process:

  1. the table call on the dense labels ec_regions gives a SPECKLED class raster (three classes drawn per square block, the
     blocks' equal neighbours merging into irregular patches, and single cells flipped at random: the patches of a land-cover map)
     at three speckle settings whose K, as found, lie near 4096, 65536 and 10^6; on the labels of a raster of square blocks
     alternating between two classes (K exactly 4096, 65536, 2^20); and on uniformly random ids below K (torch.randint: what
     hash(i) % K gives — every cell another id);
  2. the route it replaces, timed on the speckled labels near K = 4096 and on the 4096 block labels: (K + 1) / 256 chunks x
     (labels - 256 c as Float64, cast back to Int32, ec_zonal_stats_device at 256 zones) — `--only-old-route` runs this section
     alone, in a process of its own whose EC_HIP_LIB names the library it is timed on (the parent commit's build: the names that
     library does not export are left unbound);
  3. K = 256: the table call against ec_zonal_stats_device on the coherent and on the adversarial raster of profiles/zonal/zonal.md
     (ec_synth_fill ids);
  4. the two contention extremes: one zone for every cell, and every cell its own zone (side 4096: K = n = 2^24), with the integer
     atomics' byte rate (8 bytes per atomic issued by a lane flush) at the latter;
  5. ec_zonal_lookup against ec_zonal_broadcast at 256 zones, and against its own byte floor at 2^20.

Timing is by device events around whole blocks of calls, after a warm-up of every shape, the calls of a comparison by turns; the
per-call figure is the median over the blocks with the least and the greatest beside it.

    python tools/zonal_table_bench.py [--side 16384] [--blocks 3] [--out zonal_table.md] [--only-old-route]
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

PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=16384)
    ap.add_argument("--blocks", type=int, default=3, help="timed blocks per call (the median is reported)")
    ap.add_argument("--calls", type=int, default=3, help="calls per timed block")
    ap.add_argument("--only-old-route", action="store_true", help="section 2 alone: run it with EC_HIP_LIB at the parent's library")
    ap.add_argument("--out")
    args = ap.parse_args()
    side = args.side
    n = side * side
    torch.cuda.set_device(0)
    if args.only_old_route:   # a library from before the table family: bind what it exports
        raw = C.CDLL(ec._ffi.SO_PATH)
        for name in [k for k in ec._ffi.SIGNATURES if not hasattr(raw, k)]:
            del ec._ffi.SIGNATURES[name]
    ec.init(0)
    L, chk, E = ec.lib(), ec._ffi.check, ec._ffi
    stream = torch.cuda.current_stream().cuda_stream
    ec.set_stream(stream)
    lines = []

    def say(line=""):
        lines.append(line)
        print(line, flush=True)

    def block(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    def measure(fns, calls=None):
        """(median, least, greatest) ms per call of each of `fns`, block after block by turns"""
        calls = calls or args.calls
        for fn in fns:
            block(fn, 1)
        t = {fn: [] for fn in fns}
        for _ in range(args.blocks):
            for fn in fns:
                t[fn].append(block(fn, calls))
        return [(statistics.median(t[fn]), min(t[fn]), max(t[fn])) for fn in fns]

    def fmt(t):
        return f"{t[0]:.2f} ms ({t[1]:.2f}-{t[2]:.2f})"

    u16, f64, msk = ec.CellBuffer.empty(n, ec.UInt16), ec.CellBuffer.empty(n, ec.Float64), ec.Mask.empty(n)
    chk(L.ec_synth_fill(ec.UInt16, u16.mem.ptr, n, 0x20A0, 0, 0, 65535, stream))
    torch.manual_seed(0x20A1)
    t64 = torch.randn(n, dtype=torch.float64, device="cuda") * 1e3 + 1e6   # ec_synth_fill has no Float64
    chk(L.ec_copy(f64.mem.ptr, t64.data_ptr(), n * 8, stream))
    torch.cuda.synchronize()
    del t64
    chk(L.ec_synth_mask(msk.mem.ptr, n, 0x20B0, 0, 30, stream))

    def block_labels(k):
        """dense Int32 labels 1 .. k of a raster of k square blocks, from ec_regions of a class raster that alternates block by block"""
        per_side = int(round(k ** 0.5))
        b = side // per_side
        idx = np.arange(side) // b
        classes = ((idx[:, None] + idx[None, :]) % 2).astype(np.uint8).ravel()
        labels, found = ec.CellBuffer.from_vec(classes).regions(side)
        assert found == per_side * per_side, (found, k)
        return labels.buffer()

    SPECKLE = ((512, 1.2e-5), (128, 2.0e-4), (32, 3.0e-3))   # (block side, share of cells flipped): K near 4096, 65536, 10^6

    def speckled_labels(b, share):
        """(Int32 labels, K) of a class raster of three classes drawn per b x b block with single cells flipped at random"""
        g = torch.Generator(device="cuda")
        g.manual_seed(0x5EC0 + b)
        coarse = torch.randint(0, 3, (side // b, side // b), dtype=torch.uint8, device="cuda", generator=g)
        cls = coarse.repeat_interleave(b, 0).repeat_interleave(b, 1).reshape(-1)
        flip = torch.rand(n, device="cuda", generator=g) < share
        cls = torch.where(flip, (cls + 1) % 3, cls).contiguous()
        src = ec.CellBuffer.empty(n, ec.UInt8)
        chk(L.ec_copy(src.mem.ptr, cls.data_ptr(), n, stream))
        torch.cuda.synchronize()
        labels, found = src.regions(side)
        return labels.buffer(), int(found)

    def hashed(k):
        z = ec.CellBuffer.empty(n, ec.Int32)
        t = torch.randint(0, k, (n,), dtype=torch.int32, device="cuda")   # every cell another id: what hash(i) % K gives
        chk(L.ec_copy(z.mem.ptr, t.data_ptr(), n * 4, stream))
        torch.cuda.synchronize()
        return z

    def table_call(ct, vals, mask, zones, nz):
        ws = ec.DeviceMem(L.ec_zonal_table_workspace_bytes(ct, nz))
        out = ec.DeviceMem(nz * 64)

        def fn():
            chk(L.ec_zonal_table_device(ct, vals.mem.ptr, mask.mem.ptr if mask is not None else None, zones.ct, zones.mem.ptr, n, nz, out.ptr, ws.ptr, stream))
        fn.keep = (ws, out)
        return fn

    def old_call(ct, vals, mask, zones, nz):
        ws = ec.DeviceMem(L.ec_zonal_workspace_bytes(nz))
        out = ec.DeviceMem(nz * 64)

        def fn():
            chk(L.ec_zonal_stats_device(ct, vals.mem.ptr, mask.mem.ptr if mask is not None else None, zones.ct, zones.mem.ptr, n, nz, out.ptr, ws.ptr, stream))
        fn.keep = (ws, out)
        return fn

    say(f"zonal table family, {side}² cells; u16 values with a mask (30 % hidden), f64 values without")
    say()
    if args.only_old_route:
        shifted, ids = ec.CellBuffer.empty(n, ec.Float64), ec.CellBuffer.empty(n, ec.Int32)
        old = old_call(ec.UInt16, u16, msk, ids, 256)
        say("2. the route the table call replaces: (K + 1) / 256 chunks x (labels - 256 c, cast to Int32, ec_zonal_stats_device at 256 zones), u16 masked")
        for name, (labels, k) in (("speckled labels", speckled_labels(*SPECKLE[0])), ("block labels", (block_labels(4096), 4096))):
            chunks = (k + 1 + 255) // 256

            def route():
                for c in range(chunks):
                    v = ec.CellValue(ec.Int32, 256 * c).to_ec()
                    chk(L.ec_binop_scalar(ec.SUB, ec.Int32, labels.mem.ptr, n, C.byref(v), shifted.mem.ptr, stream))
                    chk(L.ec_cast(E.EC_CAST_AS, ec.Float64, shifted.mem.ptr, ec.Int32, ids.mem.ptr, n, stream))
                    old()
            t, = measure([route], calls=1)
            say(f"| {name}, K = {k}, {chunks} chunks | {fmt(t)} | {t[0] / chunks:.2f} ms per chunk |")
    else:
        say("1. the table call (ms per call; init, pass A, pass B for f64, finalize)")
        say("| K | zones | u16 masked | f64 |")
        say("|---|---|---|---|")
        for j, k in enumerate((4096, 65536, 1 << 20)):
            spk, found = speckled_labels(*SPECKLE[j])
            for name, zones, nz in ((f"speckled labels of ec_regions (blocks of {SPECKLE[j][0]}, {SPECKLE[j][1]:g} flipped)", spk, found + 1),
                                    ("block labels of ec_regions", block_labels(k), k + 1), ("random ids below K", hashed(k), k)):
                a, b = measure([table_call(ec.UInt16, u16, msk, zones, nz), table_call(ec.Float64, f64, None, zones, nz)])
                say(f"| {nz - 1 if 'labels' in name else nz} | {name} | {fmt(a)} | {fmt(b)} |")
                del zones
            del spk
        say()
        say("3. K = 256 against ec_zonal_stats_device (u16 masked, u8 zones)")
        step = max(1, side // 16)
        rows = (np.minimum(np.arange(side) // step, 15) * 16).astype(np.uint8)
        coherent = ec.CellBuffer.from_vec((rows[:, None] + np.minimum(np.arange(side) // step, 15).astype(np.uint8)[None, :]).ravel())
        adversarial = ec.CellBuffer.empty(n, ec.UInt8)
        chk(L.ec_synth_fill(ec.UInt8, adversarial.mem.ptr, n, 0x20C0, 0, 0, 255, stream))
        say("| raster | table call | ec_zonal_stats_device | table / old |")
        say("|---|---|---|---|")
        for name, zones in (("coherent, 16 x 16 blocks", coherent), ("zones[i] = hash(i) % 256", adversarial)):
            a, b = measure([table_call(ec.UInt16, u16, msk, zones, 256), old_call(ec.UInt16, u16, msk, zones, 256)])
            say(f"| {name} | {fmt(a)} | {fmt(b)} | {a[0] / b[0]:.2f} |")
        say()
        say("4. contention extremes (u16 masked, Int32 zones)")
        one = ec.CellBuffer.from_vec(np.zeros(n, dtype=np.int32))
        a, b = measure([table_call(ec.UInt16, u16, msk, one, 1), table_call(ec.Float64, f64, None, one, 1)])
        say(f"| one zone for every cell | u16 masked {fmt(a)} | f64 {fmt(b)} |")
        del one
        m = min(n, 1 << 24)
        own = ec.CellBuffer.from_vec(np.arange(m, dtype=np.int32))
        ws, out = ec.DeviceMem(L.ec_zonal_table_workspace_bytes(ec.UInt16, m)), ec.DeviceMem(m * 64)
        ws8 = ec.DeviceMem(L.ec_zonal_table_workspace_bytes(ec.Float64, m))

        def own_u16():
            chk(L.ec_zonal_table_device(ec.UInt16, u16.mem.ptr, None, ec.Int32, own.mem.ptr, m, m, out.ptr, ws.ptr, stream))

        def own_f64():
            chk(L.ec_zonal_table_device(ec.Float64, f64.mem.ptr, None, ec.Int32, own.mem.ptr, m, m, out.ptr, ws8.ptr, stream))
        a, b = measure([own_u16, own_f64])
        say(f"| every cell its own zone, K = n = {m} | u16 {fmt(a)} | f64 {fmt(b)} |")
        say(f"| integer atomics at that extreme: u16 issues 5 per cell (count, two keys, sum, the squares' low limb; a zero addend is skipped): "
            f"{5 * 8 * m / (a[0] * 1e-3) / 1e12:.3f} TB/s of atomic bytes over the whole call's time, a lower bound of their own rate |")
        del own, ws, ws8, out
        say()
        say("5. ec_zonal_lookup (f64 table, Int32 zones, with the mask)")
        dst, dm = ec.CellBuffer.empty(n, ec.Float64), ec.Mask.empty(n)
        z256, zbig = hashed(256), hashed(1 << 20)
        t256, tbig = ec.CellBuffer.from_vec(np.arange(256, dtype=np.float64)), ec.CellBuffer.from_vec(np.arange(1 << 20, dtype=np.float64))

        def lk(z, t):
            return lambda: chk(L.ec_zonal_lookup(ec.Int32, z.mem.ptr, n, t.n, ec.Float64, t.mem.ptr, dst.mem.ptr, dm.mem.ptr, stream))

        def bc():
            chk(L.ec_zonal_broadcast(ec.Int32, z256.mem.ptr, n, 256, ec.Float64, t256.mem.ptr, dst.mem.ptr, dm.mem.ptr, stream))
        a, b, c = measure([lk(z256, t256), bc, lk(zbig, tbig)], calls=5)
        floor = n * 13 / PEAK * 1e3
        say(f"| 256 zones: lookup {fmt(a)} | broadcast {fmt(b)} | lookup / broadcast {a[0] / b[0]:.2f} |")
        say(f"| 2^20 zones, hash(i) ids: lookup {fmt(c)} | byte floor (4 + 8 + 1 B per cell at 8 TB/s) {floor:.2f} ms | {c[0] / floor:.1f} x the floor |")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
