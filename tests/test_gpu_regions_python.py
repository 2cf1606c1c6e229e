"""The Python surface of the regions: CellBuffer.regions, MaskedCellBuffer.regions / sieve and Mask.regions / sieve against
tests/regions_ref.py — result types, the numbering by name, the example lines of the README as a chain classify -> focal_majority ->
regions -> zonal_stats — a stream capture of the caller-workspace form replayed once on changed inputs, and the C++ mirror's program."""
import os
import subprocess

import numpy as np
import pytest

import regions_cases as K
import regions_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


def same(got, exp, ec):
    """(MaskedCellBuffer, K) against the reference's (labels, mask bytes, K), bit for bit"""
    (buf, k), (labels, mask, ek) = got, exp
    return (isinstance(buf, ec.MaskedCellBuffer) and buf.cell_type() == ec.Int32 and isinstance(k, int) and k == ek
            and np.array_equal(buf.buffer().to_numpy(), labels.ravel()) and np.array_equal(buf.mask().to_numpy(), mask.ravel()))


def test_regions_and_sieve_against_the_reference(ec):
    for case in ((K.TW + 1, 2 * K.TH + 1, "random59", "random10"), (2 * K.TW + 1, K.TH - 1, "random3", "seam"), (K.TW, 3, "wide4", "none"),
                 (1, K.TH + 1, "checkerboard", "random10"), (257, 300, "spiral", "random10")):
        cols, rows, pattern, mask = case
        cells, valid = K.cells(cols, rows, pattern), K.valid(cols, rows, mask)
        buf = ec.CellBuffer.from_vec(cells.ravel())
        all_valid = (cols, rows, pattern, "none")
        assert same(buf.regions(cols), K.expected(all_valid, 4, K.DENSE, 0), ec), case
        assert same(buf.regions(cols, 8, 5, "root"), K.expected(all_valid, 8, K.ROOT, 5), ec), case
        masked = ec.MaskedCellBuffer(buf, ec.Mask(valid.size, ec.buffer._upload(valid.ravel())) if valid is not None else ec.Mask.fill(buf.len(), True))
        for c, min_cells, numbering in ((4, 0, "dense"), (8, 2, "dense"), (8, 5, "root"), (4, cols * rows + 1, "dense")):
            exp = K.expected(case, c, K.DENSE if numbering == "dense" else K.ROOT, min_cells)
            assert same(masked.regions(cols, connectivity=c, min_cells=min_cells, numbering=numbering), exp, ec), (case, c, min_cells, numbering)
            kept = masked.sieve(cols, min_cells, c)
            assert isinstance(kept, ec.MaskedCellBuffer) and kept.cell_type() == masked.cell_type()
            assert np.array_equal(kept.mask().to_numpy(), exp[1].ravel()) and np.array_equal(kept.buffer().to_numpy().view(np.uint8), cells.ravel().view(np.uint8))
        if pattern in K.BINARY:
            m = K.mask_form(case)
            dev = ec.Mask(m.size, ec.buffer._upload(m.ravel()))
            assert same(dev.regions(cols, 8), K.expected(case, 8, K.DENSE, 0, "mask"), ec), case
            small = dev.sieve(cols, 5)
            assert isinstance(small, ec.Mask) and np.array_equal(small.to_numpy(), K.expected(case, 4, K.ROOT, 5, "mask")[1].ravel()), case
    with pytest.raises(AssertionError):
        ec.Mask.new([True, False, True]).regions(2)   # 3 bytes are no raster of rows of 2
    with pytest.raises(ec.EcError, match="neither 4 nor 8"):
        ec.Mask.new([True, False]).regions(2, connectivity=6)
    with pytest.raises(ec.EcError, match="neither 'root' nor 'dense'"):
        ec.Mask.new([True, False]).regions(2, numbering="sparse")
    empty = ec.Mask.new([])
    labels, k = empty.regions(0)
    assert labels.len() == 0 and k == 0 and empty.sieve(0, 3).len() == 0


def test_the_example_lines_of_the_readme(ec):
    """classes = ndvi.classify(..); cleaned = classes.focal_majority(cols); patches, K = cleaned.regions(cols, connectivity=8, min_cells=20);
    per_patch = ndvi.zonal_stats(patches.buffer(), K + 1): on a raster with at most 255 regions the counts are the reference's sizes"""
    cols, rows = 96, 80
    y, x = np.mgrid[0:rows, 0:cols]
    ndvi_host = (0.5 + 0.45 * np.sin(x / 9.0) * np.cos(y / 7.0)).astype(np.float32)
    ndvi_host.ravel()[(K.hashed(cols * rows, 0x5A17) % np.uint64(50) == 0)] = 0.05     # salt for the majority filter to clean
    ndvi = ec.CellBuffer.from_vec(ndvi_host.ravel())
    classes = ndvi.classify([0.2, 0.4, 0.6])
    cleaned = classes.focal_majority(cols, radius=(1, 1))
    patches, k = cleaned.regions(cols, connectivity=8, min_cells=20)
    cleaned_host = cleaned.to_numpy().reshape(rows, cols)
    labels, mask, ek = R.regions(cleaned_host, None, 8, R.DENSE, 20)
    assert 1 < k == ek <= 255 and same((patches, k), (labels, mask, ek), ec)
    per_patch = ndvi.zonal_stats(patches.buffer(), k + 1)
    root, size = R.fill(cleaned_host, None, 8)
    assert [s.count for s in per_patch] == [int((labels == 0).sum())] + [int(size[labels == z][0]) for z in range(1, k + 1)]
    assert all(s.count >= 20 for s in per_patch[1:])
    for z in (1, k):
        assert per_patch[z].mean == pytest.approx(float(ndvi_host[labels == z].astype(np.float64).mean()), rel=2 * 7680 * 2.0 ** -52)   # two f64 sums of at most 7680 f32 cells
    # clear = cloud_mask.sieve(cols, 10): the specks go, the clouds stay
    cloud = np.zeros((rows, cols), np.uint8)
    cloud[10:30, 20:50] = 1
    cloud[60, 70] = cloud[5, 5] = cloud[5, 6] = 1
    clear = ec.Mask.new(cloud.ravel()).sieve(cols, 10)
    want = np.zeros((rows, cols), np.uint8)
    want[10:30, 20:50] = 1
    assert np.array_equal(clear.to_numpy().reshape(rows, cols), want)


def test_the_caller_workspace_form_captured_and_replayed(ec):
    """ec_regions with a workspace of the caller's allocates nothing: captured on a prepared stream and replayed once on new cells and
    mask bytes in the same buffers"""
    import torch
    L = ec.lib()
    case_a, case_b = (K.TW + 1, 2 * K.TH + 1, "random59", "random10"), (K.TW + 1, 2 * K.TH + 1, "serpentine", "seam")
    cols, rows = case_a[:2]
    n = cols * rows
    side = torch.cuda.Stream()
    ec._ffi.check(L.ec_prepare_stream(side.cuda_stream))
    t_cells = torch.from_numpy(K.cells(*case_a[:3]).ravel().copy()).cuda()
    t_valid = torch.from_numpy(K.valid(cols, rows, case_a[3]).ravel().copy()).cuda()
    t_out = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    t_omask = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    t_k = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    t_ws = torch.empty(L.ec_regions_workspace_bytes(cols, rows), dtype=torch.uint8, device="cuda")
    assert t_ws.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        h = torch.cuda.current_stream().cuda_stream
        ec._ffi.check(L.ec_regions(0, t_cells.data_ptr(), t_valid.data_ptr(), cols, rows, 8, K.DENSE, 5, t_out.data_ptr(), t_omask.data_ptr(), t_k.data_ptr(),
                                   t_ws.data_ptr(), h))
    t_cells.copy_(torch.from_numpy(K.cells(*case_b[:3]).ravel().copy()))   # new inputs in the same buffers, the same graph
    t_valid.copy_(torch.from_numpy(K.valid(cols, rows, case_b[3]).ravel().copy()))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    labels, mask, k = K.expected(case_b, 8, K.DENSE, 5)
    assert np.array_equal(t_out.cpu().numpy(), labels.ravel()) and np.array_equal(t_omask.cpu().numpy(), mask.ravel()) and int(t_k.cpu()[0]) == k


def test_cpp_mirror_regions_program():
    """erased-cells_amd/host/test_regions_mirror.cpp: the C++ mirror's regions / sieve on cells worked out by hand"""
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "erased-cells_amd", "host")
    binary = os.path.join(host, "test_regions_mirror")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", host, "-s", "test_regions_mirror"])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
