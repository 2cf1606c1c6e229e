"""The zonal entry points write what the header says and nothing else — wherever it sits — and leave their inputs alone.

tests/test_gpu_zonal.py is strict about values, but its outputs are fresh aligned blocks.  Here every call goes through the C ABI
with pointers into guarded arenas (tests/arena.py):

  * `moments_dev` gets exactly n_zones x 64 bytes: the arena is pre-filled with the complement of the expected records between
    random guards and starts on every 8-byte residue mod 64;
  * the workspace is written to ec_zonal_workspace_bytes(n_zones) bytes at the most: its guards are compared byte for byte
    (what the payload holds afterwards is scrap);
  * ec_zonal_broadcast writes exactly n cells and n mask bytes, `dst` on every cell-aligned residue mod 16, the mask on every residue,
    under both settings of "unaligned_vector";
  * the value raster, its mask, the zone raster and the table sit in operand arenas that are compared byte for byte, guards included;
  * a refused call writes nothing: the arenas still hold their before-image."""
import numpy as np
import pytest

import stats_ref as R
import zonal_ref as Z
from arena import GUARD, Arena, operand
from test_gpu_stats import NAMES, NP, random_cells, random_mask
from test_gpu_zonal import ZNP, zone_ids

pytestmark = pytest.mark.gpu

OK, UNSUPPORTED, ARG = 0, 2, 6


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def pack(ec, ref):
    """A reference record as the 64 bytes of its ec_moments."""
    rec = ec._ffi.EcMoments()
    dt = ref["dtype"]
    rec.count, rec.kind, rec.dtype, rec.reserved = ref["count"], ref["kind"], dt, 0
    rec.keys2[0], rec.keys2[1] = ~R.order_key(dt, ref["min"]), R.order_key(dt, ref["max"])
    if ref["kind"] == 0:
        rec.u.i.sum, rec.u.i.sq_lo, rec.u.i.sq_hi = ref["sum"], ref["sq"] & (2**64 - 1), ref["sq"] >> 64
    else:
        rec.u.f.pivot, rec.u.f.s1, rec.u.f.s2 = ref["pivot"], ref["s1"], ref["s2"]
    return bytes(rec)


def guards_unchanged(arena, what):
    got = arena.image()
    assert np.array_equal(got[:arena.lo], arena.before[:arena.lo]), f"{what}: bytes in front of the payload were written"
    assert np.array_equal(got[arena.lo + arena.nbytes:], arena.before[arena.lo + arena.nbytes:]), f"{what}: bytes behind the payload were written"


@pytest.mark.parametrize("ct,zt,nz,masked", [(R.U8, R.U8, 3, True), (R.I32, R.U16, 5, False), (R.F64, R.I32, 2, True), (R.U16, R.U8, 1, False)],
                         ids=["u8-u8", "i32-u16", "f64-i32", "u16-one-zone"])
def test_records_and_workspace_stay_inside_their_blocks(ec, ct, zt, nz, masked):
    L = ec.lib()
    T, cpl = Z.tile(ct), Z.cpl(ct)
    ws_bytes = L.ec_zonal_workspace_bytes(nz)
    single = multi = 0
    for j, n in enumerate([0, 1, cpl + 1, T - 1, T + 1, 3 * T + cpl + 1]):
        cells, mask, zones = random_cells(ct, n, 40 + j), random_mask(n, 50 + j), zone_ids("runs37", n, nz + 1, zt)   # id nz: foreign
        refs = Z.records(ct, cells.tolist(), zones.tolist(), nz, mask.tolist() if masked else None)
        exp = np.frombuffer(b"".join(pack(ec, r) for r in refs), dtype=np.uint8)
        pa, za = operand(ec, cells, offset_cells=j % 2, seed=j), operand(ec, zones, offset_cells=(j + 1) % 3, seed=10 + j)
        ma = operand(ec, mask, offset_cells=j % 2, seed=20 + j) if masked else None
        for k, arm in enumerate((dict(), dict(unaligned_vector=0))):
            off = 8 * ((2 * j + k) % 8)
            out = Arena(exp.nbytes, GUARD, off, 3 * j + k, ec).expect(exp)
            ws = Arena(ws_bytes, GUARD, 16 * (j % 4), 7 * j + k, ec).hold(np.zeros(ws_bytes, np.uint8))
            with ec.tuned(**arm):
                st = L.ec_zonal_stats_device(ct, pa.ptr, ma.ptr if ma else None, zt, za.ptr, n, nz, out.ptr, ws.ptr, ec.stream())
            assert st == OK, L.ec_last_error_string()
            what = (NAMES[ct], NAMES[zt], "n", n, arm, "offset", off)
            out.check(exp, f"records {what}")
            guards_unchanged(ws, f"workspace {what}")
            if 0 < n <= Z.BLOCK:
                single += 1
                ws.check_unchanged(f"workspace of a one-workgroup grid {what}")   # the workgroup writes the records itself
            elif n > 2 * T:
                multi += 1
        for a in (pa, za, ma):
            if a is not None:
                a.check_unchanged(f"an input, n = {n}")
    assert single and multi


@pytest.mark.parametrize("arm", [dict(), dict(unaligned_vector=0)], ids=["default", "cellwise-when-unaligned"])
@pytest.mark.parametrize("ct,zt", [(R.U8, R.I32), (R.I16, R.U8), (R.F32, R.U16), (R.F64, R.U8), (R.U64, R.I32)], ids=["u8-i32", "i16-u8", "f32-u16", "f64-u8", "u64-i32"])
def test_broadcast_writes_n_cells_and_n_mask_bytes(ec, ct, zt, arm):
    L = ec.lib()
    nz, sz = 100, Z.SIZE[ct]
    T, cpl = Z.broadcast_tile(ct, zt), Z.broadcast_cpl(ct, zt)
    assert GUARD > T * sz
    table = random_cells(ct, nz, 60 + ct)
    ta = operand(ec, table, seed=61)
    with ec.tuned(**arm):
        for j, n in enumerate(sorted({1, cpl - 1, cpl, cpl + 1, T - 1, T, T + 1, T + cpl + 1} - {0})):
            zones = zone_ids("random", n, nz, zt, seed=70 + j)
            zones[::7] = Z.ZONE_RANGE[zt][1]
            cells, mask = Z.broadcast(zones.tolist(), table.tolist(), nz)
            exp, em = np.array(cells, dtype=NP[ct]), np.array(mask, dtype=np.uint8)
            za = operand(ec, zones, offset_cells=j % 3, seed=80 + j)
            for off in range(0, 16, sz):
                moff = (5 * off + j) % 16
                dst = Arena(exp.nbytes, GUARD, off, 7 * off + j, ec).expect(exp)
                dmask = Arena(n, GUARD, moff, 11 * off + j, ec).expect(em) if (off // sz) % 3 != 2 else None
                st = L.ec_zonal_broadcast(zt, za.ptr, n, nz, ct, ta.ptr, dst.ptr, dmask.ptr if dmask else None, ec.stream())
                assert st == OK, L.ec_last_error_string()
                what = (NAMES[ct], NAMES[zt], "n", n, "offsets", off, moff)
                dst.check(exp, f"dst {what}")
                if dmask:
                    dmask.check(em, f"dst_mask {what}")
            za.check_unchanged(f"zones, n = {n}")
    ta.check_unchanged("the table")


def test_a_refused_call_writes_nothing(ec):
    L, s = ec.lib(), ec.stream()
    ct, zt, n, nz = R.U16, R.U8, 1000, 4
    cells, mask, zones = random_cells(ct, n, 90), random_mask(n, 91), zone_ids("runs37", n, nz, zt)
    pa, ma, za = operand(ec, cells, seed=1), operand(ec, mask, seed=2), operand(ec, zones, seed=3)
    out = Arena(nz * 64, GUARD, 8, 4, ec).hold(np.zeros(nz * 64, np.uint8))
    ws = Arena(L.ec_zonal_workspace_bytes(nz), GUARD, 0, 5, ec).hold(np.zeros(L.ec_zonal_workspace_bytes(nz), np.uint8))
    table = operand(ec, np.arange(nz, dtype=np.float64), seed=6)
    dst = Arena(n * 8, GUARD, 8, 7, ec).hold(np.zeros(n * 8, np.uint8))
    dmask = Arena(n, GUARD, 3, 8, ec).hold(np.zeros(n, np.uint8))
    dev = lambda t=ct, p=pa.ptr, m=ma.ptr, z_t=zt, z=za.ptr, nn=n, k=nz, o=out.ptr, w=ws.ptr: L.ec_zonal_stats_device(t, p, m, z_t, z, nn, k, o, w, s)
    bc = lambda z_t=zt, z=za.ptr, nn=n, k=nz, t=R.F64, tb=table.ptr, d=dst.ptr, dm=dmask.ptr: L.ec_zonal_broadcast(z_t, z, nn, k, t, tb, d, dm, s)
    refused = [dev(k=0), dev(k=257), dev(k=-1), dev(p=None), dev(z=None), dev(o=None), dev(w=None), dev(nn=2**32 + 1),
               dev(o=pa.ptr), dev(o=za.ptr + n - 1), dev(o=ma.ptr), dev(w=pa.ptr), dev(w=za.ptr), dev(w=ma.ptr + n - 1), dev(o=ws.ptr), dev(w=out.ptr - 64),
               bc(k=0), bc(k=257), bc(z=None), bc(tb=None), bc(d=None), bc(d=za.ptr), bc(d=table.ptr), bc(dm=za.ptr), bc(dm=table.ptr), bc(dm=dst.ptr)]
    assert refused == [ARG] * len(refused)
    assert [dev(t=10), dev(z_t=R.U32), dev(z_t=R.F32), bc(t=255), bc(z_t=R.I8)] == [UNSUPPORTED] * 5
    assert bc(nn=0) == OK   # nothing to do
    for arena in (pa, ma, za, out, ws, table, dst, dmask):
        arena.check_unchanged("a refused call")
