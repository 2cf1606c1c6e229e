"""tests/zonal_table_ref.py held to: a scalar transcription of the header's rule on the bits of a double (the arithmetic the
kernels do: exponent and fraction fields, shifts, two limbs, one cut to 53 bits); zonal_ref.records for the exact integer kind;
stats_ref's exact sums wherever the deviations span fewer than 63 bits; the header's error bound on general data; and hand-worked
zones.  No device, nothing from the library."""
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

import stats_ref as R
import zonal_ref as Z
import zonal_table_cases as K
import zonal_table_ref as ZT

FRAC = (1 << 52) - 1
INF = 0x7FF0000000000000


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ---------------------------------------------------------------- the header, on bits
def t_unit_shift(max_bits):
    exp = max_bits >> 52
    length = (max_bits & FRAC).bit_length() if exp == 0 else exp + 52
    return max(length - 63, 0)


def t_trunc(d, k):
    b = bits(d)
    exp = (b >> 52) & 0x7FF
    mant = (b & FRAC) | (1 << 52) if exp else b & FRAC
    up = (exp - 1 if exp else 0) - k
    mag = mant << up if up >= 0 else mant >> -up
    assert mag < 2**63
    return -mag if b >> 63 else mag


def t_round(T, e):
    """T * 2^e with one cut to 53 bits, ties to even, as the finalize lane does it on two words"""
    if T == 0:
        return 0.0
    mag = abs(T)
    drop = max(mag.bit_length() - 53, 0)
    q = mag >> drop
    rest, half = mag & ((1 << drop) - 1), (1 << drop) >> 1
    if drop and (rest > half or (rest == half and q & 1)):
        q += 1
    try:
        r = math.ldexp(float(q), e + drop)  # exact: a multiple of 2^-1074 of at most 53 bits, or an overflow
    except OverflowError:
        r = math.inf
    return -r if T < 0 else r


def t_sums(d):
    """the header's s1, s2 through limbs: every t split as lo + hi * 2^32, the words added apart"""
    mx = max((bits(x) & ~(1 << 63) for x in d), default=0)
    if mx > INF:
        return math.nan, math.nan
    if mx == INF:
        pos, neg = math.inf in d, -math.inf in d
        return (math.nan if pos and neg else math.inf if pos else -math.inf), math.inf

    def limb_sum(values, k):
        lo = hi = 0
        for v in values:
            t = t_trunc(v, k)
            lo += t & 0xFFFFFFFF
            hi += t >> 32
        assert lo < 2**64 and -2**63 <= hi < 2**63
        return lo + (hi << 32)
    k1 = t_unit_shift(mx)
    s1 = t_round(limb_sum(d, k1), k1 - 1074)
    dmax = struct.unpack("<d", struct.pack("<Q", mx))[0]
    wmax = bits(dmax * dmax)
    if wmax >= INF:
        return s1, math.inf
    k2 = t_unit_shift(wmax)
    return s1, t_round(limb_sum([x * x for x in d], k2), k2 - 1074)


def same(a, b):
    return bits(a) == bits(b) or (math.isnan(a) and math.isnan(b))


def random_zone(rng, spread):
    m = int(rng.integers(1, 40))
    e = rng.integers(-spread, spread, size=m, endpoint=True)
    return [math.ldexp(float(x), int(k)) for x, k in zip(rng.standard_normal(m), e)]


@pytest.mark.parametrize("spread", [0, 20, 40, 100, 500, 1000])
def test_the_reference_is_the_headers_arithmetic(spread):
    rng = np.random.default_rng(0x5EED + spread)
    for _ in range(300):
        d = random_zone(rng, spread)
        got, want = ZT.sums(d), t_sums(d)
        assert same(got[0], want[0]) and same(got[1], want[1]), (d, got, want)


def test_the_hand_zones_in_both_arithmetics():
    for what, d in K.HAND:
        got, want = ZT.sums(d), t_sums(d)
        assert same(got[0], want[0]) and same(got[1], want[1]), (what, got, want)


# ---------------------------------------------------------------- hand-worked zones
def test_hand_worked_zones():
    hand = dict((w.split(":")[0], ZT.sums(d)) for w, d in K.HAND)
    # unit 2^8 (L = 1074 + 71 = 1145, k = 1082): 1.5 truncates to 0; w's unit is 2^78: 2.25 truncates to 0
    assert hand["one cell of 2^70 with a thousand of 1.5"] == (2.0**70, 2.0**140)
    # 384 = 1.5 units: one unit, 256, each; 384^2 = 147456 is below w's unit
    assert hand["the same with 2^8 * 1.5"] == (2.0**70 + 256000.0, 2.0**140)
    # unit 2^18: 2^20 + 3 survives as 2^20; w: unit 2^98, the tiny's square 2^40 + .. truncates to 0
    assert hand["cancellation"] == (2.0**20, 2.0**161)
    sub = [15e-324, -5e-324, 2.0**-1060, 2.0**-1030]
    assert hand["subnormals only"] == (float(R.exact_sum(sub)), 0.0) and ZT.unit_shift(sub) == 0
    s1, s2 = hand["an overflowing w"]
    # 1e200 < 2^665: unit 2^(665 + 1074 - 63 - 1074) = 2^602; 3e199's last bit is 2^610: a multiple of the unit, exact
    assert s2 == math.inf and s1 == 3e199 and ZT.unit_shift([1e200]) - 1074 == 602
    assert all(math.isnan(x) for x in hand["a NaN"]) and all(math.isnan(x) for x in hand["a NaN among infinities"])
    assert hand["+inf"] == (math.inf, math.inf) and hand["-inf"] == (-math.inf, math.inf)
    assert math.isnan(hand["both infinities"][0]) and hand["both infinities"][1] == math.inf
    assert hand["empty"] == (0.0, 0.0) and bits(hand["empty"][0]) == 0
    # T = 5 * 1.9 * 2^62 - 0 passes 2^64: the -3.0 is below the unit 2^8
    assert hand["five cells near 2^71"][0] == 5 * 1.9 * 2.0**70
    # toward zero, not toward -infinity: -384.5 -> -256, 383.9 -> +256
    assert hand["negative deviations truncate toward zero"][0] == -7 * 256 + 3 * 256
    # d's unit is 2^-82, w's 2^-102: 2.25 * 2^-90 is 9216 of those, and none of d's
    assert hand["small deviations"] == (2.0**-20 + 1500 * 2.0**-45, 2.0**-40 + 2250 * 2.0**-90)


def test_a_tie_rounds_to_even_once():
    # T = 2^53 + 1 in units of 1 (k = 0 would need subnormals; scale instead): 2^62 + 2^9 at unit 2^-1074 + k
    d = [2.0**70, 2.0**17]          # unit 2^8: T = 2^62 + 2^9, 63 bits: cut 10 bits, rest = 2^9 = half, q even -> down
    assert ZT.sums(d)[0] == 2.0**70
    d = [2.0**70, 2.0**18, 2.0**17]  # q odd -> up
    assert ZT.sums(d)[0] == 2.0**70 + 2.0**19


# ---------------------------------------------------------------- against the older references
def test_kind0_records_are_zonal_refs():
    for ct, zt, masked, nz, pattern, n, off, seed in K.kind0_cases():
        if nz > Z.MAX_ZONES:
            continue
        cells, mask, zones = K.arrays(ct, zt, nz, pattern, n, off, seed)
        mk = mask[off:].tolist() if masked else None
        assert ZT.records(ct, cells[off:].tolist(), zones[off:].tolist(), nz, mk) == Z.records(ct, cells[off:].tolist(), zones[off:].tolist(), nz, mk)


def test_exact_sums_where_the_deviations_span_fewer_than_63_bits():
    seen = 0
    for ct, zt, masked, nz, pattern, n, off, seed in K.kind1_exact_cases():
        cells, mask, zones = K.arrays(ct, zt, nz, pattern, n, off, seed)
        refs = ZT.records(ct, cells[off:].tolist(), zones[off:].tolist(), nz, mask[off:].tolist() if masked else None)
        for r in refs:
            if r["count"]:
                assert all(ZT.units(x) % (1 << r["k1"]) == 0 and ZT.units(x * x) % (1 << r["k2"]) == 0 for x in r["d"])   # multiples of the unit
                assert r["s1"] == float(r["s1_exact"]) and r["s2"] == float(r["s2_exact"])
                seen += 1
    assert seen > 100


def test_the_error_bound_on_general_data():
    """|s1 - sum d| < m * 2^(k - 1074) + 1/2 ulp(s1), and the same for s2 over the rounded squares; and that bound is at least 2^9
    times tighter than (m + 1) u sum|d|."""
    cells, zones, mask = K.general_raster(2 * ZT.tile(R.F64) + 5, 37, R.U8)
    u = Fraction(1, 2**53)
    for mk in (None, mask.tolist()):
        for r in ZT.records(R.F64, cells.tolist(), zones.tolist(), 37, mk):
            m = r["count"]
            assert m > 10
            for s, exact, k, terms in ((r["s1"], r["s1_exact"], r["k1"], r["d"]), (r["s2"], r["s2_exact"], r["k2"], [x * x for x in r["d"]])):
                unit = Fraction(2)**(k - 1074)
                bound = m * unit + Fraction(math.ulp(s)) / 2
                assert abs(Fraction(s) - exact) < bound
                old = (m + 1) * u * sum(abs(Fraction(x)) for x in terms)
                assert m * unit * 2**9 <= old, (float(m * unit), float(old))   # the truncation's share; the last rounding is any sum's


def test_the_planted_raster_reaches_every_class():
    cells, zones, mask, nz = K.planted_raster()
    refs = ZT.records(R.F64, cells.tolist(), zones.tolist(), nz, mask.tolist())
    assert refs[0]["pivot"] == 0.0 and len(refs) == len(K.HAND) + 1
    for z, (what, d) in enumerate(K.HAND):
        assert refs[z]["count"] == len(d), what
        s = ZT.sums(d)
        assert same(refs[z]["s1"], s[0]) and same(refs[z]["s2"], s[1]), what   # whatever the order the cells were scattered in
    g = refs[nz - 1]
    assert g["count"] == 1500 and g["s1"] == float(g["s1_exact"])
    # without the mask the hidden NaN reaches every hand zone
    assert all(math.isnan(r["s1"]) for r in ZT.records(R.F64, cells.tolist(), zones.tolist(), nz, None)[:len(K.HAND)])


def test_record_bytes_and_sparse_tables():
    cells, mask, zones = K.big_k_case(65537, R.I32, R.F64, 5)
    found, empty = ZT.sparse_records(R.F64, cells.tolist(), zones.tolist(), 65537, mask.tolist())
    assert 0 in found and 65536 in found and 65537 not in found and -1 not in found and empty["count"] == 0
    raw = K.sparse_table_bytes(found, empty, 65537)
    assert len(raw) == 65537 * 64 and raw[64 * 65536:] == K.record_bytes(found[65536]) and len(K.record_bytes(empty)) == 64
    assert ZT.workspace_bytes(R.F64, 2**24) == 2**24 * 80 < 2**32 and ZT.workspace_bytes(R.U8, 2**24) == 2**24 * 48
    assert ZT.workspace_bytes(R.F64, 0) == ZT.workspace_bytes(R.F64, 2**24 + 1) == ZT.workspace_bytes(10, 4) == 0
