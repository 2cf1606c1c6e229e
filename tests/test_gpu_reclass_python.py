"""The Python mirror of ec_reclass on the GPU: classify + zonal_stats is a histogram, classify of one break is the predicate of
ec_compare_scalar, reclassify drops a class through MaskedCellBuffer, and the C++ mirror's program."""
import os
import subprocess

import numpy as np
import pytest

import reclass_ref as Q
from vectors import rand_cells

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def test_classify_and_zonal_stats_are_a_histogram(ec):
    rng = np.random.default_rng(5)
    x = rng.random(20011).astype(np.float32)
    edges = [0.2, 0.4, 0.6, 0.8]
    buf = ec.CellBuffer.from_vec(x)
    classes = buf.classify(edges)
    assert classes.cell_type() == ec.UInt8 and classes.to_numpy().max() <= 4
    counts = [s.count for s in buf.zonal_stats(classes, 5)]
    want, _ = np.histogram(x.astype(np.float64), bins=[-np.inf] + edges + [np.inf])   # numpy's bins are [a, b): right = False
    assert counts == want.tolist() and sum(counts) == x.size
    # masked: the cells that are not valid are in no bin
    mask = rng.random(x.size) < 0.6
    mb = ec.MaskedCellBuffer(buf, ec.Mask.new(mask))
    mc = mb.classify(edges)
    counts = [s.count for s in mb.zonal_stats(mc.buffer(), 5)]
    assert counts == np.histogram(x[mask].astype(np.float64), bins=[-np.inf] + edges + [np.inf])[0].tolist()
    assert np.all(mc.buffer().to_numpy()[~mask] == 255) and np.array_equal(mc.mask().to_numpy().astype(bool), mask)
    # a 16-bit band, integer edges of its own type
    y = rand_cells(Q.U16, 30001, 3)
    e16 = [1000, 20000, 40000, 65535]
    cy = ec.CellBuffer.from_vec(y)
    assert [s.count for s in cy.zonal_stats(cy.classify(e16), 5)] == np.bincount(np.digitize(y, e16), minlength=5).tolist()


def test_one_break_is_the_compare_predicate(ec):
    """a Float32 raster against the Python float 0.3: the break is a Float64 (the union case — 0.3f is not 0.3)"""
    x = np.concatenate([rand_cells(Q.F32, 9001, 2), np.float32([0.3, np.nextafter(np.float32(0.3), np.float32(0)), np.nextafter(np.float32(0.3), np.float32(1))])])
    buf = ec.CellBuffer.from_vec(x)
    assert np.array_equal(buf.classify([0.3]).to_numpy(), buf.ge(0.3).to_numpy().astype(np.uint8))
    assert np.array_equal(buf.classify([0.3], right=True).to_numpy(), buf.gt(0.3).to_numpy().astype(np.uint8))
    assert np.array_equal(buf.classify([0.3]).to_numpy(), Q.classes(Q.F32, x, Q.F64, [0.3], False).astype(np.uint8))


def test_reclassify_with_a_dropped_class(ec):
    x = np.array([0.05, 0.25, 0.45, 0.65, 0.85, np.nan, 0.3] * 700, np.float32)
    mask = np.array([1, 1, 1, 1, 0, 0, 1] * 700, bool)
    mb = ec.MaskedCellBuffer(ec.CellBuffer.from_vec(x), ec.Mask.new(mask))
    out = mb.reclassify([0.2, 0.4, 0.6], np.array([10, 20, -1, 40], np.int16), valid=[1, 1, 0, 1], nodata=-1)
    assert out.cell_type() == ec.Int16
    want, want_ok = Q.reclass(Q.F32, x, mask.astype(np.uint8), Q.F64, [0.2, 0.4, 0.6], False, Q.I16, [10, 20, -1, 40], [1, 1, 0, 1], -1)
    assert np.array_equal(out.buffer().to_numpy(), want) and np.array_equal(out.mask().to_numpy().astype(np.uint8), want_ok)
    assert want[:7].tolist() == [10, 20, -1, 40, -1, -1, 20] and want_ok[:7].tolist() == [1, 1, 0, 1, 0, 0, 1]
    # unmasked with a dropped class: a MaskedCellBuffer comes back; without one, a CellBuffer
    plain = ec.CellBuffer.from_vec(x[:5])
    dropped = plain.reclassify([0.2, 0.4, 0.6], [1, 2, 3, 4], valid=[1, 0, 1, 1])
    assert isinstance(dropped, ec.MaskedCellBuffer) and dropped.mask().to_numpy().astype(int).tolist() == [1, 0, 1, 1, 1] and dropped.buffer().to_numpy().tolist() == [1, 2, 3, 4, 4]
    kept = plain.reclassify([0.2, 0.4, 0.6], [1, 2, 3, 4])
    assert isinstance(kept, ec.CellBuffer) and kept.cell_type() == ec.UInt8 and kept.to_numpy().tolist() == [1, 2, 3, 4, 4]
    # a table built once and used twice
    t = ec.ReclassTable(ec.Float32, [0.2, 0.4, 0.6], [1, 2, 3, 4])
    assert plain.reclassify(t).to_numpy().tolist() == plain.reclassify(t).to_numpy().tolist() == [1, 2, 3, 4, 4]
    assert ec.CellBuffer.from_vec(np.zeros(0, np.float32)).reclassify(t).len() == 0


def test_the_cpp_mirror():
    exe = os.path.join(ROOT, "erased-cells_amd", "host", "test_reclass_mirror")
    assert os.path.exists(exe), "build() makes it"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ok" in r.stdout
