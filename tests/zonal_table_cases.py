"""The inputs of tests/test_gpu_zonal_table.py, built without a device, so that tests/test_zonal_table_faults.py can show on the
very same arrays that each modelled mistake changes the reference's answer.  Also the reference records as bytes."""
import math
import struct

import numpy as np

import stats_ref as R
import zonal_ref as Z
import zonal_table_ref as ZT
from test_gpu_stats import NP, random_cells, random_mask
from test_gpu_zonal import ZNP, zone_ids

QUIET_NAN = 0x7FF8000000000000
BIG_K = [65535, 65536, 65537, 2**20 + 1]
N_ZONES = [1, 256, 257, 4097] + BIG_K
PATTERNS = ["constant", "modulo", "runs37", "alternating", "edges", "own"]


def f64_bits(x):
    return QUIET_NAN if math.isnan(x) else struct.unpack("<Q", struct.pack("<d", x))[0]


def record_bytes(ref):
    """A reference record as the 64 bytes of its ec_moments (a NaN sum is the rule's quiet NaN)."""
    dt = ref["dtype"]
    head = struct.pack("<Qqqii", ref["count"], ~R.order_key(dt, ref["min"]), R.order_key(dt, ref["max"]), ref["kind"], dt)
    if ref["kind"] == 0:
        body = struct.pack("<qQQ", ref["sum"], ref["sq"] & (2**64 - 1), ref["sq"] >> 64)
    else:
        body = struct.pack("<QQQ", f64_bits(ref["pivot"]), f64_bits(ref["s1"]), f64_bits(ref["s2"]))
    return head + body + struct.pack("<Q", 0)


def table_bytes(refs):
    return b"".join(record_bytes(r) for r in refs)


def sparse_table_bytes(found, empty, n_zones):
    """n_zones records: `empty` everywhere but at the zones of `found`"""
    out = np.tile(np.frombuffer(record_bytes(empty), dtype=np.uint8), n_zones).reshape(n_zones, 64)
    for z, r in found.items():
        out[z] = np.frombuffer(record_bytes(r), dtype=np.uint8)
    return out.tobytes()


def ids(pattern, n, nz, zt, seed=0):
    """test_gpu_zonal.zone_ids and "own": every cell its own zone (K = n)"""
    if pattern == "own":
        assert n <= nz and n - 1 <= Z.ZONE_RANGE[zt][1]
        return np.arange(n, dtype=np.int64).astype(ZNP[zt])
    return zone_ids(pattern, n, nz, zt, seed)


# ---------------------------------------------------------------- the planted f64 raster
BIG70 = 2.0**70
HAND = [  # (what, the zone's deviations: the raster's pivot is 0.0)
    ("one cell of 2^70 with a thousand of 1.5: the small ones truncate to 0", [BIG70] + [1.5] * 1000),
    ("the same with 2^8 * 1.5: kept, as one unit each", [BIG70] + [384.0] * 1000),
    ("cancellation: the tiny survives only as its truncation", [2.0**80, -2.0**80, 2.0**20 + 3.0]),
    ("subnormals only: k = 0, exact", [15e-324, -5e-324, 2.0**-1060, 2.0**-1030]),
    ("an overflowing w", [1e200, -1e200, 3e199]),
    ("a NaN", [1.0, math.nan, 2.0]),
    ("+inf", [1.0, math.inf, 2.0**900]),
    ("-inf", [-math.inf, 5.0]),
    ("both infinities", [math.inf, 3.0, -math.inf]),
    ("a NaN among infinities", [math.inf, math.nan, -math.inf]),
    ("empty", []),
    ("five cells near 2^71: |T| passes 2^64", [BIG70 * 1.9] * 5 + [-3.0]),
    ("negative deviations truncate toward zero", [BIG70, -BIG70] + [-384.5] * 7 + [383.9] * 3),
    ("small deviations: w's unit lies below d's", [2.0**-20] + [1.5 * 2.0**-45] * 1000),
]


def planted_raster(zt=R.I32, seed=0x71A7):
    """(cells, zones, mask, n_zones): an f64 raster whose first cell is 0.0 under a foreign id (pivot 0.0), the HAND zones' cells
    scattered over it, a general zone (standard_normal * 1e3 + 1e6), and decoys — NaN, an infinity and 1e300 under cleared mask
    bytes and under foreign ids, some INSIDE the hand zones' ids (hidden) — that must reach no maximum, flag or sum."""
    rng = np.random.default_rng(seed)
    nz = len(HAND) + 1
    general = (rng.standard_normal(1500) * 1e3 + 1e6).tolist()
    cells, zones, mask = [], [], []
    for z, (_, d) in enumerate(HAND):
        cells += d
        zones += [z] * len(d)
        mask += [1] * len(d)
        cells += [math.nan, math.inf, 1e300]          # hidden in this very zone
        zones += [z] * 3
        mask += [0] * 3
    cells += general
    zones += [nz - 1] * len(general)
    mask += [1] * len(general)
    foreign = [nz, -1] if zt == R.I32 else [nz, Z.ZONE_RANGE[zt][1]]
    for k in range(40):                                # shown, but of no zone
        cells.append([math.nan, -math.inf, 1e300, 2.0**1000][k % 4])
        zones.append(foreign[k % 2])
        mask.append(1)
    order = rng.permutation(len(cells))
    cells = [0.0] + [cells[i] for i in order]
    zones = [nz] + [zones[i] for i in order]
    mask = [1] + [mask[i] for i in order]
    return np.array(cells, dtype=np.float64), np.array(zones, dtype=np.int64).astype(ZNP[zt]), np.array(mask, dtype=np.uint8), nz


def general_raster(n, nz, zt, seed=0x6E4):
    rng = np.random.default_rng(seed)
    cells = rng.standard_normal(n) * 1e3 + 1e6
    zones = zone_ids("random", n, nz, zt, seed=seed + 2)
    return cells, zones, random_mask(n, seed + 1)


def kind0_cases():
    """(ct, zt, masked, nz, pattern, n, offset, seed): every integer value type, the three zone types, masked and not"""
    types = [t for t in range(10) if R.KIND[t] == 0]
    combos = [(zt, m) for zt in Z.ZONE_TYPES for m in (False, True)]
    counts = [1, 256, 257, 4097]
    for k, ct in enumerate(types):
        zt, masked = combos[k % 6]
        nz = counts[k % 4]
        yield ct, zt, masked, nz, ["runs37", "modulo", "edges"][k % 3], 2 * ZT.tile(ct) + 5, (0, 1, 3)[k % 3], 0x7AB0 + k


def kind1_exact_cases():
    """(ct, zt, masked, nz, pattern, n, offset, seed): cells BASE + r with 0 < |r| <= 512, whose deviations span fewer than 63 bits"""
    for k, (ct, zt, masked, nz, pattern) in enumerate([(R.U64, R.U8, True, 256, "runs37"), (R.I64, R.U16, False, 257, "modulo"),
                                                       (R.F32, R.I32, True, 4097, "edges"), (R.F64, R.U16, False, 1, "constant"),
                                                       (R.F64, R.I32, True, 257, "alternating")]):
        yield ct, zt, masked, nz, pattern, 2 * ZT.tile(ct) + 5, (1, 3, 0)[k % 3], 0x7AC0 + k


def arrays(ct, zt, nz, pattern, n, offset, seed):
    """the pool of a case: offset + n cells, mask bytes and ids; the call sees [offset:]"""
    pool = n + offset
    return random_cells(ct, pool, seed), random_mask(pool, seed + 1), ids(pattern, pool, nz, zt)


def big_k_case(nz, zt, ct, seed):
    """a few thousand cells whose ids include 0, K - 1 and K (foreign); u16 ids reach what the type holds"""
    n = 3000 + nz % 7
    rng = np.random.default_rng(seed)
    hi = min(nz, Z.ZONE_RANGE[zt][1])
    z = rng.integers(0, hi, size=n, endpoint=True)
    z[[1, 2, 3, 4, 5, 6]] = [0, min(nz - 1, hi), hi, 0, min(nz - 1, hi), nz - 1 - 65536 if nz - 1 - 65536 >= 0 else 0]
    if zt == R.I32:
        z[7] = -1
    return random_cells(ct, n, seed + 1), random_mask(n, seed + 2), z.astype(ZNP[zt])


LOOKUP_PAIRS = ((R.U8, R.I32), (R.I16, R.U16), (R.F32, R.U8), (R.F64, R.I32), (R.U64, R.U16))   # (cell type of the table, zone type)
LOOKUP_ZONES = [1, 256, 257, 4097, 65537]


def lookup_arrays(ct, zt, nz, pool):
    """(ids, table) of a lookup case: random ids from -1 (Int32) to nz — nz itself is foreign — clipped to what zt holds, with 0,
    nz - 1, nz and the type's maximum in front"""
    rng = np.random.default_rng(0xB0 + ct + nz)
    lo, hi = Z.ZONE_RANGE[zt]
    zones = np.clip(rng.integers(-1 if zt == R.I32 else 0, nz, size=pool, endpoint=True), lo, hi).astype(ZNP[zt])
    zones[:4] = np.clip([0, nz - 1, nz, hi], lo, hi).astype(ZNP[zt])
    return zones, random_cells(ct, nz, 0xB1 + ct)
