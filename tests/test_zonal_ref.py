"""tests/zonal_ref.py — the reference the GPU tests of the zonal statistics use — held to cells worked out by hand, to
stats_ref over the whole raster when every cell is in zone 0, and to numpy.bincount for the counts and the integer sums.
No GPU."""
import math

import numpy as np

import stats_ref as R
import zonal_ref as Z

NAN = math.nan
# twelve cells, three zones, one foreign id (255) and one NaN under a cleared mask byte
CELLS = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, NAN, 10.0, 11.0, 12.0]
ZONES = [0, 0, 1, 1, 2, 2, 0, 255, 1, 2, 1, 0]
MASK = [1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1]


def test_twelve_cells_by_hand():
    assert Z.members(ZONES, 3, MASK) == [[0, 1, 6, 11], [2, 3, 10], [4, 5, 9]]
    assert Z.members(ZONES, 3) == [[0, 1, 6, 11], [2, 3, 8, 10], [4, 5, 9]]
    recs = Z.records(R.F64, CELLS, ZONES, 3, MASK)
    # the pivot is the first cell of the RASTER in every record: d = x - 1
    assert [r["pivot"] for r in recs] == [1.0, 1.0, 1.0]
    assert [(r["count"], r["min"], r["max"]) for r in recs] == [(4, 1.0, 12.0), (3, 3.0, 11.0), (3, 5.0, 10.0)]
    assert [(r["s1"], r["s2"]) for r in recs] == [(0 + 1 + 6 + 11, 0 + 1 + 36 + 121), (2 + 3 + 10, 4 + 9 + 100), (4 + 5 + 9, 16 + 25 + 81)]
    st = Z.stats(R.F64, CELLS, ZONES, 3, MASK)
    assert [(s["count"], s["sum"], s["mean"]) for s in st] == [(4, 22.0, 5.5), (3, 18.0, 6.0), (3, 21.0, 7.0)]
    assert st[0]["stddev"] == math.sqrt((20.25 + 12.25 + 2.25 + 42.25) / 4.0)
    # without the mask the NaN reaches zone 1 and no other
    open_ = Z.records(R.F64, CELLS, ZONES, 3)
    assert math.isnan(open_[1]["s1"]) and math.isnan(open_[1]["s2"]) and open_[1]["count"] == 4
    assert (open_[0]["s1"], open_[2]["s1"]) == (18.0, 18.0)
    # the foreign cell's 8.0 is nowhere; a fourth zone is empty and holds the call's pivot
    four = Z.records(R.F64, CELLS, ZONES, 4, MASK)
    hi, lo = R.sentinels(R.F64)
    assert (four[3]["count"], four[3]["min"], four[3]["max"], four[3]["s1"], four[3]["s2"], four[3]["pivot"]) == (0, hi, lo, 0.0, 0.0, 1.0)
    assert sum(r["count"] for r in four) == 10


def test_the_pivot_is_the_first_cell_whatever_its_mask_byte_or_zone():
    cells, zones = [100.0, 101.0, 103.0], [7, 0, 0]           # the first cell is foreign
    r = Z.records(R.F64, cells, zones, 1)[0]
    assert (r["pivot"], r["count"], r["s1"], r["s2"]) == (100.0, 2, 4.0, 10.0)
    r = Z.records(R.F64, cells, [0, 0, 0], 1, [0, 1, 1])[0]    # ... or hidden
    assert (r["pivot"], r["count"], r["s1"], r["s2"]) == (100.0, 2, 4.0, 10.0)
    r = Z.records(R.F32, [math.inf, 1.0, 2.0], [5, 0, 0], 1)[0]  # not finite: 0.0
    assert (r["pivot"], r["s1"], r["s2"]) == (0.0, 3.0, 5.0)
    assert [r["pivot"] for r in Z.records(R.I64, [], [], 3)] == [0.0, 0.0, 0.0]
    assert all(r["kind"] == 0 and "pivot" not in r for r in Z.records(R.U8, [1, 2], [0, 1], 2))


def test_negative_and_out_of_range_ids_belong_to_no_zone():
    zones = [-1, 0, 1, 2, -2**31, 2**31 - 1, 1]
    assert Z.members(zones, 2) == [[1], [2, 6]]
    assert Z.zone_of(3, zones, 3, None, 7) == 2 and Z.zone_of(3, zones, 2, None, 7) is None   # `<`, not `<=`
    assert Z.zone_of(6, zones, 2, None, 6) is None                                             # i < n
    assert Z.zone_of(1, zones, 2, [1, 0, 1, 1, 1, 1, 1], 7) is None


def test_every_cell_in_zone_zero_is_the_whole_raster():
    rng = np.random.default_rng(0x20A)
    for dtype, cells in ((R.I16, rng.integers(-2**15, 2**15, 500).tolist()), (R.U32, rng.integers(0, 2**32, 500).tolist()),
                         (R.F64, (rng.integers(-512, 513, 500) + 10**9).astype(np.float64).tolist()),
                         (R.U64, (rng.integers(-512, 513, 500) + 10**9).tolist())):
        mask = (rng.integers(0, 3, 500) > 0).astype(np.uint8).tolist()
        for mk in (None, mask):
            for nz in (1, 4):
                got = Z.stats(dtype, cells, [0] * 500, nz, mk)
                assert got[0] == R.stats(dtype, cells, mk)
                rec = Z.records(dtype, cells, [0] * 500, nz, mk)
                whole = R.record(dtype, cells, mk)
                assert rec[0] == whole
                assert all(r["count"] == 0 for r in rec[1:])


def test_counts_and_integer_sums_against_bincount():
    rng = np.random.default_rng(0x20B)
    n, nz = 5000, 37
    cells = rng.integers(-2**15, 2**15, n)
    zones = rng.integers(-3, nz + 3, n)
    mask = (rng.integers(0, 4, n) > 0)
    for mk in (None, mask):
        keep = (zones >= 0) & (zones < nz) & (mask if mk is not None else True)
        counts = np.bincount(zones[keep], minlength=nz)
        sums = np.bincount(zones[keep], weights=cells[keep].astype(np.float64), minlength=nz)   # exact: |sum| < 2^53
        sqs = np.bincount(zones[keep], weights=cells[keep].astype(np.float64) ** 2, minlength=nz)
        recs = Z.records(R.I16, cells.tolist(), zones.tolist(), nz, None if mk is None else mk.astype(np.uint8).tolist())
        assert [r["count"] for r in recs] == counts.tolist()
        assert [r["sum"] for r in recs] == [int(s) for s in sums]
        assert [r["sq"] for r in recs] == [int(s) for s in sqs]


def test_broadcast_by_hand():
    out, mask = Z.broadcast([0, 2, 3, -1, 1, 255], [10.5, 20.5, 30.5], 3)
    assert out == [10.5, 30.5, 0, 0, 20.5, 0] and mask == [1, 1, 0, 0, 1, 0]
    assert Z.broadcast([], [1], 1) == ([], [])


def test_launch_constants():
    assert Z.tile(R.U8) == 16384 and Z.tile(R.F64) == 2048 and Z.cpl(R.U16) == 8
    assert Z.broadcast_cpl(R.U8, R.I32) == 4 and Z.broadcast_tile(R.F64, R.U8) == 1024
    assert [Z.workspace_bytes(k) for k in (0, 1, 256, 257)] == [0, 4096 * 48, 256 * 4096 * 48, 0]
