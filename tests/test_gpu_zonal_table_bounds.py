"""The zonal table entry points write what the header says and nothing else — wherever it sits — and leave their inputs alone.

tests/test_gpu_zonal_table.py is strict about values, but its outputs are fresh aligned blocks.  Here every call goes through the C
ABI with pointers into guarded arenas (tests/arena.py):

  * `moments_dev` gets exactly n_zones x 64 bytes: the arena is pre-filled with the complement of the expected records between
    random guards and starts on every 16-byte residue mod 64;
  * the workspace is written to ec_zonal_table_workspace_bytes(t, n_zones) bytes at the most: its guards are compared byte for byte
    (what the payload holds afterwards is scrap);
  * ec_zonal_lookup writes exactly n cells and n mask bytes at every size around its tile, `dst` on every cell-aligned residue
    mod 16, the mask on every residue, under both settings of "unaligned_vector";
  * the value raster, its mask, the zone raster and the table sit in operand arenas that are compared byte for byte, guards included;
  * a refused call writes nothing: the arenas still hold their before-image."""
import numpy as np
import pytest

import stats_ref as R
import zonal_ref as Z
import zonal_table_cases as K
import zonal_table_ref as ZT
from arena import GUARD, Arena, operand
from test_gpu_stats import NAMES, NP, random_cells, random_mask

pytestmark = pytest.mark.gpu

OK, UNSUPPORTED, ARG = 0, 2, 6


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def guards_unchanged(arena, what):
    got = arena.image()
    assert np.array_equal(got[:arena.lo], arena.before[:arena.lo]), f"{what}: bytes in front of the payload were written"
    assert np.array_equal(got[arena.lo + arena.nbytes:], arena.before[arena.lo + arena.nbytes:]), f"{what}: bytes behind the payload were written"


@pytest.mark.parametrize("ct,zt,nz,masked", [(R.U8, R.U8, 3, True), (R.I32, R.U16, 300, False), (R.F64, R.I32, 257, True), (R.U16, R.U8, 1, False),
                                             (R.F32, R.U16, 1000, True)], ids=["u8-u8", "i32-u16", "f64-i32", "u16-one-zone", "f32-u16"])
def test_records_and_workspace_stay_inside_their_blocks(ec, ct, zt, nz, masked):
    L = ec.lib()
    T, cpl = ZT.tile(ct), ZT.cpl(ct)
    ws_bytes = L.ec_zonal_table_workspace_bytes(ct, nz)
    assert ws_bytes == ZT.workspace_bytes(ct, nz)
    for j, n in enumerate([0, 1, cpl + 1, T - 1, T + 1, 3 * T + cpl + 1]):
        cells, mask = random_cells(ct, n, 40 + j), random_mask(n, 50 + j)
        zones = K.ids("runs37", n, min(nz + 1, Z.ZONE_RANGE[zt][1] + 1), zt)   # id nz: foreign
        refs = ZT.records(ct, cells.tolist(), zones.tolist(), nz, mask.tolist() if masked else None)
        exp = np.frombuffer(K.table_bytes(refs), dtype=np.uint8)
        pa, za = operand(ec, cells, offset_cells=j % 2, seed=j), operand(ec, zones, offset_cells=(j + 1) % 3, seed=10 + j)
        ma = operand(ec, mask, offset_cells=j % 2, seed=20 + j) if masked else None
        for k, arm in enumerate((dict(), dict(unaligned_vector=0))):
            off = 16 * ((2 * j + k) % 4)
            out = Arena(exp.nbytes, GUARD, off, 3 * j + k, ec).expect(exp)
            ws = Arena(ws_bytes, GUARD, 16 * (j % 4), 7 * j + k, ec).hold(np.zeros(ws_bytes, np.uint8))
            with ec.tuned(**arm):
                st = L.ec_zonal_table_device(ct, pa.ptr, ma.ptr if ma else None, zt, za.ptr, n, nz, out.ptr, ws.ptr, ec.stream())
            assert st == OK, L.ec_last_error_string()
            what = (NAMES[ct], NAMES[zt], "n", n, arm, "offset", off)
            out.check(exp, f"records {what}")
            guards_unchanged(ws, f"workspace {what}")
        for a in (pa, za, ma):
            if a is not None:
                a.check_unchanged(f"an input, n = {n}")


@pytest.mark.parametrize("arm", [dict(), dict(unaligned_vector=0)], ids=["default", "cellwise-when-unaligned"])
@pytest.mark.parametrize("ct,zt", [(R.U8, R.I32), (R.I16, R.U8), (R.F32, R.U16), (R.F64, R.U8), (R.U64, R.I32)], ids=["u8-i32", "i16-u8", "f32-u16", "f64-u8", "u64-i32"])
def test_lookup_writes_n_cells_and_n_mask_bytes(ec, ct, zt, arm):
    L = ec.lib()
    nz, sz = 1000 if zt != R.U8 else 100, Z.SIZE[ct]
    T, cpl = Z.broadcast_tile(ct, zt), Z.broadcast_cpl(ct, zt)
    assert GUARD > T * sz
    table = random_cells(ct, nz, 60 + ct)
    ta = operand(ec, table, seed=61)
    with ec.tuned(**arm):
        for j, n in enumerate(sorted({1, cpl - 1, cpl, cpl + 1, T - 1, T, T + 1, T + cpl + 1} - {0})):
            zones = K.zone_ids("random", n, nz, zt, seed=70 + j)
            zones[::7] = Z.ZONE_RANGE[zt][1]
            cells, mask = ZT.lookup(zones.tolist(), table.tolist(), nz)
            exp, em = np.array(cells, dtype=NP[ct]), np.array(mask, dtype=np.uint8)
            za = operand(ec, zones, offset_cells=j % 3, seed=80 + j)
            for off in range(0, 16, sz):
                moff = (5 * off + j) % 16
                dst = Arena(exp.nbytes, GUARD, off, 7 * off + j, ec).expect(exp)
                dmask = Arena(n, GUARD, moff, 11 * off + j, ec).expect(em) if (off // sz) % 3 != 2 else None
                st = L.ec_zonal_lookup(zt, za.ptr, n, nz, ct, ta.ptr, dst.ptr, dmask.ptr if dmask else None, ec.stream())
                assert st == OK, L.ec_last_error_string()
                what = (NAMES[ct], NAMES[zt], "n", n, "offsets", off, moff)
                dst.check(exp, f"dst {what}")
                if dmask:
                    dmask.check(em, f"dst_mask {what}")
            za.check_unchanged(f"zones, n = {n}")
    ta.check_unchanged("the table")


def test_a_refused_call_writes_nothing(ec):
    L, s = ec.lib(), ec.stream()
    ct, zt, n, nz = R.F64, R.U16, 1000, 300
    cells, mask, zones = random_cells(ct, n, 90), random_mask(n, 91), K.ids("runs37", n, nz, zt)
    pa, ma, za = operand(ec, cells, seed=1), operand(ec, mask, seed=2), operand(ec, zones, seed=3)
    out = Arena(nz * 64, GUARD, 16, 4, ec).hold(np.zeros(nz * 64, np.uint8))
    wsb = L.ec_zonal_table_workspace_bytes(ct, nz)
    ws = Arena(wsb, GUARD, 0, 5, ec).hold(np.zeros(wsb, np.uint8))
    table = operand(ec, np.arange(nz, dtype=np.float64), seed=6)
    dst = Arena(n * 8, GUARD, 8, 7, ec).hold(np.zeros(n * 8, np.uint8))
    dmask = Arena(n, GUARD, 3, 8, ec).hold(np.zeros(n, np.uint8))
    dev = lambda t=ct, p=pa.ptr, m=ma.ptr, z_t=zt, z=za.ptr, nn=n, k=nz, o=out.ptr, w=ws.ptr: L.ec_zonal_table_device(t, p, m, z_t, z, nn, k, o, w, s)
    lk = lambda z_t=zt, z=za.ptr, nn=n, k=nz, t=R.F64, tb=table.ptr, d=dst.ptr, dm=dmask.ptr: L.ec_zonal_lookup(z_t, z, nn, k, t, tb, d, dm, s)
    refused = [dev(k=0), dev(k=2**24 + 1), dev(k=-1), dev(p=None), dev(z=None), dev(o=None), dev(w=None), dev(nn=2**32 + 1), dev(o=out.ptr + 8), dev(w=ws.ptr + 8),
               dev(o=pa.ptr), dev(o=za.ptr + 2 * n - 16), dev(o=ma.ptr), dev(w=pa.ptr), dev(w=za.ptr), dev(w=ma.ptr + n - 8), dev(o=ws.ptr), dev(w=out.ptr - 64),
               lk(k=0), lk(k=2**24 + 1), lk(z=None), lk(tb=None), lk(d=None), lk(d=za.ptr), lk(d=table.ptr), lk(dm=za.ptr), lk(dm=table.ptr), lk(dm=dst.ptr)]
    assert refused == [ARG] * len(refused)
    assert [dev(t=10), dev(z_t=R.U32), dev(z_t=R.F32), lk(t=255), lk(z_t=R.I8)] == [UNSUPPORTED] * 5
    assert lk(nn=0) == OK   # nothing to do
    for arena in (pa, ma, za, out, ws, table, dst, dmask):
        arena.check_unchanged("a refused call")
