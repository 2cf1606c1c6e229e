#!/usr/bin/env python3
"""Throughput of the window kernels, the resampling ones included, against the library's contiguous copy (dev tool).

For u8, u16, f32 and f64 on a side² source (default 16384²), interleaved in one process, HIP-event timed behind an untimed clock ramp,
over rotating operand sets (every set is touched once per rotation, so no operand is served from the Infinity Cache by the previous use):

  (a) ec_window of the centred (side/2)² window
  (b) ec_convert with identical source and destination type (the library's contiguous copy) over (side/2)² contiguous cells
  (c) the per-row ec_copy loop a caller needed before ec_window: side/2 launches
  (d) ec_window_put of the same tile
  (e) ec_window of the whole raster at half size (nearest neighbour, 2x down)
  (f) ec_window_resample, Average, of the whole raster at half size (2x down):    2² W + W = 5 W bytes per output cell of W bytes
  (g) ec_window_resample, Average, of the whole raster at quarter size (4x down): 4² W + W = 17 W bytes per output cell
  (h) ec_window_resample, Bilinear, of the centred window at twice its size (2x up): W / 4 + W bytes per output cell (four output cells
      share one cell of the window; each reads four)

GB/s counts the bytes the call must move: read + written cells for (a)-(d); for (e) the written cells plus the 128-byte lines of the source
it touches (every line of every sampled row: half the raster); for (f)-(h) every cell of the window once plus the written cells, as stated.

    python tools/window_bench.py [side] > window.md
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "erased-cells_amd", "python"))

import torch  # noqa: E402

import erased_cells_hip as ec  # noqa: E402

PEAK_GBS = 8000.0


def main():
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    half = side // 2
    x0 = y0 = half // 2
    torch.cuda.set_device(0)
    ec.init(0)
    L = ec.lib()
    stream = torch.cuda.current_stream().cuda_stream
    ec.set_stream(stream)
    chk = ec._ffi.check

    def timed(fn, sets, min_ms=40.0):
        """ms per call of fn(k), k rotating over the operand sets; ramp first, then whole rotations until min_ms has passed"""
        for k in range(max(2 * sets, 8)):
            fn(k % sets)
        torch.cuda.synchronize()
        rounds, total, calls = 1, 0.0, 0
        while calls == 0 or total < min_ms:  # at least one rotation: row (c) asks for no minimum
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(rounds):
                for k in range(sets):
                    fn(k)
            e1.record()
            torch.cuda.synchronize()
            total += e0.elapsed_time(e1)
            calls += rounds * sets
            rounds *= 2
        return total / calls

    print(f"Window kernels, source {side}x{side}, window {half}x{half} at ({x0}, {y0}), one MI355X, HIP-event timed, rotating operand sets, "
          f"peak {PEAK_GBS:.0f} GB/s\n")
    print("| cells | case | ms/call | GB/s | frac of peak | vs (b) |")
    print("|---|---|---:|---:|---:|---:|")
    for ct, name in ((ec.UInt8, "u8"), (ec.UInt16, "u16"), (ec.Float32, "f32"), (ec.Float64, "f64")):
        cell = ec.NP_DTYPES[ct].itemsize
        n_src, n_win = side * side, half * half
        # enough sets that a rotation exceeds the 256 MiB Infinity Cache several times over
        sets = max(2, min(6, (4 << 30) // (n_src * cell)))
        srcs, tiles, flats = [], [], []
        for k in range(sets):
            s = ec.CellBuffer.empty(n_src, ct)
            chk(L.ec_synth_fill(ec.UInt8, s.mem.ptr, n_src * cell, 0x51DE + k, 0, 0.0, 255.0, stream))
            srcs.append(s)
            tiles.append(ec.CellBuffer.empty(n_win, ct))
            flats.append(ec.CellBuffer.empty(n_win, ct))
        small = [ec.CellBuffer.empty(n_win, ct) for _ in range(sets)]
        quarter = side // 4
        tiny = [ec.CellBuffer.empty(quarter * quarter, ct) for _ in range(sets)]
        ups = [ec.CellBuffer.empty(n_src, ct) for _ in range(sets)]  # the (side/2)² window at twice its size: side² cells

        def win(k):
            chk(L.ec_window(ct, srcs[k].mem.ptr, None, side, side, x0, y0, half, half, half, half, tiles[k].mem.ptr, None, stream))

        def copy(k):
            chk(L.ec_convert(ct, srcs[k].mem.ptr, ct, flats[k].mem.ptr, n_win, stream))

        def rows(k):
            for r in range(half):
                chk(L.ec_copy(flats[k].mem.ptr + r * half * cell, srcs[k].mem.ptr + ((y0 + r) * side + x0) * cell, half * cell, stream))

        def put(k):
            chk(L.ec_window_put(ct, tiles[k].mem.ptr, None, half, half, srcs[k].mem.ptr, None, side, side, x0, y0, stream))

        def down(k):
            chk(L.ec_window(ct, srcs[k].mem.ptr, None, side, side, 0, 0, side, side, half, half, small[k].mem.ptr, None, stream))

        def avg2(k):
            chk(L.ec_window_resample(ec._ffi.EC_RESAMPLE_AVERAGE, ct, srcs[k].mem.ptr, None, side, side, 0, 0, side, side, half, half,
                                     small[k].mem.ptr, None, stream))

        def avg4(k):
            chk(L.ec_window_resample(ec._ffi.EC_RESAMPLE_AVERAGE, ct, srcs[k].mem.ptr, None, side, side, 0, 0, side, side, quarter, quarter,
                                     tiny[k].mem.ptr, None, stream))

        def up2(k):
            chk(L.ec_window_resample(ec._ffi.EC_RESAMPLE_BILINEAR, ct, srcs[k].mem.ptr, None, side, side, x0, y0, half, half, side, side,
                                     ups[k].mem.ptr, None, stream))

        moved = 2 * n_win * cell
        # (e): every second row is sampled; of such a row every 128-byte line holds a sampled cell unless cells are 128 bytes apart
        down_bytes = n_win * cell + half * side * cell
        results = {}
        for rep in range(2):  # interleaved: a .. h, then again
            for key, fn, nbytes, mn in (("a", win, moved, 40.0), ("b", copy, moved, 40.0), ("c", rows, moved, 0.0), ("d", put, moved, 40.0),
                                        ("e", down, down_bytes, 40.0), ("f", avg2, 5 * n_win * cell, 40.0),
                                        ("g", avg4, 17 * quarter * quarter * cell, 40.0), ("h", up2, (n_win + n_src) * cell, 40.0)):
                ms = timed(fn, sets, mn)
                results.setdefault(key, []).append((ms, nbytes))
        label = {"a": "(a) ec_window, centred window", "b": "(b) ec_convert T->T, contiguous", "c": f"(c) {half} x ec_copy, one per row",
                 "d": "(d) ec_window_put, same tile", "e": "(e) ec_window, whole raster 2x down",
                 "f": "(f) ec_window_resample Average, whole raster 2x down, 5 W B/cell",
                 "g": "(g) ec_window_resample Average, whole raster 4x down, 17 W B/cell",
                 "h": "(h) ec_window_resample Bilinear, centred window 2x up, 1.25 W B/cell"}
        b_ms = min(ms for ms, _ in results["b"])
        for key in "abcdefgh":
            for ms, nbytes in results[key]:
                gbs = nbytes / (ms * 1e-3) / 1e9
                rel = f"{b_ms / ms:.3f}" if key in "acd" else ""
                print(f"| {name} | {label[key]} | {ms:.4f} | {gbs:.0f} | {gbs / PEAK_GBS:.3f} | {rel} |", flush=True)
        del srcs, tiles, flats, small, tiny, ups
        ec.synchronize()


if __name__ == "__main__":
    main()
