"""The Python surface of the distance transform: Mask.distance and Mask.within against tests/distance_ref.py — result types, the greatest
distance given as int, float and Fraction, the example lines of the README — a stream capture of the caller-workspace form replayed once,
and the C++ mirror's program."""
import ctypes as C
import fractions
import os
import subprocess

import numpy as np
import pytest

import distance_cases as K
import distance_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def same(got, exp, ec):
    """a MaskedCellBuffer against the reference's (cells, mask bytes), bit for bit"""
    cells, valid = exp
    bits = np.uint32 if cells.dtype == np.uint32 else np.uint64
    return (isinstance(got, ec.MaskedCellBuffer) and np.array_equal(got.buffer().to_numpy().view(bits), cells.ravel().view(bits))
            and np.array_equal(got.mask().to_numpy(), valid.ravel()))


def test_distance_and_within_against_the_reference(ec):
    for case in ((K.T + 1, 2 * K.W + 3, "random1"), (2 * K.W + 3, K.T + 1, "diagonal"), (K.T, 3, "none"), (1, K.W + 1, "centre"), (257, 300, "random001")):
        cols, rows, _ = case
        m = K.mask(*case)
        mask = ec.Mask(m.size, ec.buffer._upload(m.ravel()))
        d = mask.distance(cols)
        assert d.cell_type() == ec.Float64 and d.len() == cols * rows and same(d, K.expected(*case), ec)
        sq = mask.distance(cols, squared=True)
        assert sq.cell_type() == ec.UInt32 and same(sq, K.expected(*case, out_type=R.U32), ec)
        # the greatest distance as int, float and Fraction: floor(d^2) is exact, and the limit is inclusive
        for given, max_sq in ((3, 9), (0, 0), (2.5, 6), (2 ** 0.5, 2), (fractions.Fraction(7, 5), 1), (fractions.Fraction(5, 1), 25), (1e9, K.UNLIMITED), (None, K.UNLIMITED)):
            assert same(mask.distance(cols, given), K.expected(*case, max_sq=max_sq), ec), (case, given)
            assert same(mask.distance(cols, max_distance=given, squared=True), K.expected(*case, max_sq=max_sq, out_type=R.U32), ec), (case, given)
            if given is not None:
                near = mask.within(cols, given)
                assert isinstance(near, ec.Mask) and np.array_equal(near.to_numpy(), K.expected(*case, max_sq=max_sq)[1].ravel()), (case, given)
    with pytest.raises(AssertionError):
        ec.Mask.new([True, False, True]).distance(2)   # 3 bytes are no raster of rows of 2
    with pytest.raises(ec.EcError, match="greatest distance"):
        ec.Mask.new([True, False]).within(2, -1)
    empty = ec.Mask.new([])
    assert empty.distance(0).len() == 0 and empty.within(0, 3).len() == 0


def test_the_example_lines_of_the_readme(ec):
    """near = cloud_mask.within(cols, 50); d = water.distance(cols): a disc of radius 50 around a single cloud cell, where seven chained
    dilations give a square"""
    cols, rows = 160, 140
    m = np.zeros((rows, cols), np.uint8)
    m[70, 80] = 1
    cloud_mask = ec.Mask.new(m.ravel())
    near = cloud_mask.within(cols, 50)
    y, x = np.mgrid[0:rows, 0:cols]
    disc = (y - 70) ** 2 + (x - 80) ** 2 <= 2500
    assert np.array_equal(near.to_numpy().reshape(rows, cols), disc.astype(np.uint8))
    assert near.counts()[0] == int(disc.sum()) and not near.to_numpy().reshape(rows, cols)[70 - 36, 80 - 36]   # (36, 36) is inside the square, outside the disc
    water = ec.Mask.new((m.ravel() != 0) | (np.arange(cols * rows) == 0))
    d = water.distance(cols)
    got = d.buffer().to_numpy().reshape(rows, cols)
    assert got[70, 80] == 0.0 and got[0, 0] == 0.0 and got[70, 83] == 3.0 and got[73, 84] == 5.0 and got[71, 81] == np.sqrt(2.0)
    assert d.counts() == (cols * rows, 0)


def test_the_caller_workspace_form_captured_and_replayed(ec):
    """ec_distance with a workspace of the caller's allocates nothing: captured on a prepared stream and replayed once on new mask bytes in
    the same buffer"""
    import torch
    L = ec.lib()
    case_a, case_b = (K.T + 1, 2 * K.W + 3, "random1"), (K.T + 1, 2 * K.W + 3, "diagonal")
    cols, rows, _ = case_a
    n = cols * rows
    side = torch.cuda.Stream()
    ec._ffi.check(L.ec_prepare_stream(side.cuda_stream))
    t_mask = torch.from_numpy(K.mask(*case_a).ravel().copy()).cuda()
    t_out = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    t_valid = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    t_ws = torch.empty(L.ec_distance_workspace_bytes(cols, rows), dtype=torch.uint8, device="cuda")
    assert t_ws.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        h = torch.cuda.current_stream().cuda_stream
        ec._ffi.check(L.ec_distance(t_mask.data_ptr(), cols, rows, 40, R.F64, t_out.data_ptr(), t_valid.data_ptr(), t_ws.data_ptr(), h))
    t_mask.copy_(torch.from_numpy(K.mask(*case_b).ravel().copy()))   # new inputs in the same buffer, the same graph
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    exp, ev = K.expected(*case_b, max_sq=40)
    assert np.array_equal(t_out.cpu().numpy().view(np.uint64), exp.ravel().view(np.uint64))
    assert np.array_equal(t_valid.cpu().numpy(), ev.ravel())


def test_cpp_mirror_distance_program():
    """erased-cells_amd/host/test_distance_mirror.cpp: the C++ mirror's Mask::distance / Mask::within on cells worked out by hand"""
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "erased-cells_amd", "host")
    binary = os.path.join(host, "test_distance_mirror")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", host, "-s", "test_distance_mirror"])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
