"""ec_composite on the GPU against tests/composite_ref.py, bit for bit on the raw bytes: every cell type x every op, stack heights on
both sides of every plausible batch size, lengths that leave a partial last group at every CPL, masks none / all / some entries NULL,
min_count 1, 2 and K, with and without aux, a layer passed twice, both settings of "unaligned_vector", the Python wrapper's return
types.  One test has NaNs planted among the valid cells: there two NaNs of SUM / MEAN are equal by class (which payload an addition
keeps is the processor's choice); FIRST / LAST / MIN / MAX stay strict there too.  tests/test_composite_faults.py shows that these
inputs expose each modelled kernel mistake."""
import ctypes as C

import numpy as np
import pytest

import composite_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    ec.init(0)
    return ec


class Stack:
    """a stack on the device, uploaded once: every layer and mask `off` cells / bytes behind a 256-byte boundary"""

    def __init__(self, ec, ct, layers, masks, off=0):
        self.ec, self.ct, self.k, self.n, self.layers, self.masks = ec, ct, len(layers), layers[0].size, layers, masks
        self._mem = []
        self.lp = (C.c_void_p * self.k)(*[self._up(a, off * a.dtype.itemsize) for a in layers])
        self.mp = None if masks is None else (C.c_void_p * self.k)(*[None if m is None else self._up(m, off) for m in masks])

    def _up(self, a, off_bytes):
        mem = self.ec.DeviceMem(a.nbytes + 512)
        self._mem.append(mem)
        p = mem.ptr - mem.ptr % -256 + off_bytes
        self.ec._ffi.check(self.ec.lib().ec_upload(p, np.ascontiguousarray(a).ctypes.data_as(C.c_void_p), a.nbytes, self.ec.stream()))
        return p

    def run(self, op, min_count, aux=True, off=0, mask_out=None):
        """(cells, mask or None, aux or None) as the device computed them; a mask comes back when a layer has one (or mask_out)"""
        ec, L, n = self.ec, self.ec.lib(), self.n
        rt = R.NP[R.result_type(op, self.ct)]
        masked = (self.masks is not None and any(m is not None for m in self.masks)) if mask_out is None else mask_out
        outs = []
        for want, size in ((True, n * rt.itemsize), (masked, n), (aux, n)):
            mem = ec.DeviceMem(size + 512) if want else None
            outs.append((mem, None if mem is None else mem.ptr - mem.ptr % -256 + off * (rt.itemsize if not outs else 1)))
        ec._ffi.check(L.ec_composite(op, self.ct, self.lp, self.mp, self.k, n, min_count, outs[0][1], outs[1][1], outs[2][1], ec.stream()))
        res = []
        for (mem, p), dt in zip(outs, (rt, np.dtype(np.uint8), np.dtype(np.uint8))):
            if mem is None:
                res.append(None)
                continue
            a = np.empty(n, dt)
            ec._ffi.check(L.ec_download(a.ctypes.data_as(C.c_void_p), p, a.nbytes, ec.stream()))
            res.append(a)
        return res


def check(got, want, where, nan_by_class=False):
    cells, mask, aux = got
    wc, wm, wa = want
    assert R.same_cells(cells, wc, nan_by_class).all(), (where, "cells", int(np.flatnonzero(~R.same_cells(cells, wc, nan_by_class))[0]))
    if mask is not None:
        assert np.array_equal(mask, wm), (where, "mask", int(np.flatnonzero(mask != wm)[0]))
    else:
        assert wm.all(), (where, "no mask came back, yet a cell is invalid")
    if aux is not None:
        assert np.array_equal(aux, wa), (where, "aux", int(np.flatnonzero(aux != wa)[0]))


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_every_op_stack_height_and_min_count(ec, ct, form):
    n = R.main_len(ct)
    for k in R.KS:
        layers, masks = R.stack(ct, k, n, form)
        s = Stack(ec, ct, layers, masks)
        for op in R.OPS:
            for mc in R.min_counts(k):
                check(s.run(op, mc), R.composite(op, ct, layers, masks, mc), (R.NAMES[ct], R.OP_NAMES[op], k, form, mc))


@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_short_lengths_and_lengths_around_a_tile(ec, ct):
    for op in R.OPS:
        for n in R.small_lengths(op, ct):
            for k, form in ((3, "some"), (9, "all")):
                layers, masks = R.stack(ct, k, n, form, seed=1)
                s = Stack(ec, ct, layers, masks)
                for mc in (1, 2):
                    check(s.run(op, mc), R.composite(op, ct, layers, masks, mc), (R.NAMES[ct], R.OP_NAMES[op], n, k, form, mc))


@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_without_aux_and_without_a_result_mask(ec, ct):
    n = R.main_len(ct)
    for k in (2, 5):
        for form in ("none", "all"):
            layers, masks = R.stack(ct, k, n, form, seed=2)
            s = Stack(ec, ct, layers, masks)
            for op in R.OPS:
                want = R.composite(op, ct, layers, masks, 1)
                check(s.run(op, 1, aux=False), want, (R.NAMES[ct], R.OP_NAMES[op], k, form, "no aux"))
                if form == "none":   # a result mask may be asked for all the same: it is always written, all ones here
                    got = s.run(op, k, aux=True, mask_out=True)
                    check(got, R.composite(op, ct, layers, masks, k), (R.NAMES[ct], R.OP_NAMES[op], k, form, "mask asked for"))
                    assert got[1].all()


@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_the_same_layer_twice(ec, ct):
    n = R.main_len(ct)
    layers, masks = R.stack(ct, 3, n, "all", seed=3)
    s = Stack(ec, ct, layers, masks)
    order = (0, 1, 0, 2, 1, 1)
    twice_l, twice_m = [layers[i] for i in order], [masks[i] for i in order]
    s.k, s.lp, s.mp = len(order), (C.c_void_p * len(order))(*[s.lp[i] for i in order]), (C.c_void_p * len(order))(*[s.mp[i] for i in order])
    for op in R.OPS:
        for mc in (1, 4):
            check(s.run(op, mc), R.composite(op, ct, twice_l, twice_m, mc), (R.NAMES[ct], R.OP_NAMES[op], mc))


@pytest.mark.parametrize("vector", (1, 0), ids=("unaligned_vector", "cellwise"))
@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_pointers_at_odd_cell_offsets(ec, ct, vector):
    """inputs and outputs one and three cells behind an aligned address: the vector kernels with under-aligned accesses, and — the knob
    off — the cell-wise kernels"""
    n = R.main_len(ct)
    with ec.tuned(unaligned_vector=vector):
        for k, form, off in ((5, "some", 1), (8, "all", 3)):
            layers, masks = R.stack(ct, k, n, form, seed=4)
            s = Stack(ec, ct, layers, masks, off=off)
            for op in R.OPS:
                check(s.run(op, 2, off=off), R.composite(op, ct, layers, masks, 2), (R.NAMES[ct], R.OP_NAMES[op], k, form, off, vector))


@pytest.mark.parametrize("ct", R.FLOATS, ids=[R.NAMES[t] for t in R.FLOATS])
def test_nans_among_the_valid_cells(ec, ct):
    """NaNs of several payloads and both signs, valid: SUM / MEAN equal by class, the picks bit for bit (a NaN is the greatest cell of
    the total order, a negative NaN the least)"""
    n = R.main_len(ct)
    for k in (3, 8):
        layers, masks = R.stack(ct, k, n, "all", seed=5)
        rng = np.random.default_rng(77 + k)
        for i, a in enumerate(layers):
            at = rng.random(n) < 0.05
            a[at] = np.where(rng.random(int(at.sum())) < 0.5, R.nan_of(ct, 0x100 + i), -R.nan_of(ct, 0x200 + i))
        assert any((np.isnan(a) & (m != 0)).any() for a, m in zip(layers, masks))
        s = Stack(ec, ct, layers, masks)
        for op in R.OPS:
            want = R.composite(op, ct, layers, masks, 1)
            check(s.run(op, 1), want, (R.NAMES[ct], R.OP_NAMES[op], k), nan_by_class=R.sums(op))
            if R.sums(op):
                assert np.isnan(want[0]).any()


def test_the_python_wrappers_return_types(ec):
    n, ct = 1000, R.I16
    layers, masks = R.stack(ct, 3, n, "all", seed=6)
    plain = [ec.CellBuffer.from_vec(a) for a in layers]
    mixed = [plain[0], ec.MaskedCellBuffer(plain[1], ec.Mask.new(masks[1])), plain[2]]
    out = ec.composite(plain, "max")
    assert isinstance(out, ec.CellBuffer) and out.cell_type() == ec.Int16
    assert np.array_equal(out.to_numpy(), R.composite(R.MAX, ct, layers, None, 1)[0])
    out, aux = ec.composite(plain, op="mean", aux=True)
    assert isinstance(out, ec.CellBuffer) and out.cell_type() == ec.Float64 and isinstance(aux, ec.CellBuffer) and aux.cell_type() == ec.UInt8
    assert np.array_equal(out.to_numpy(), R.composite(R.MEAN, ct, layers, None, 1)[0]) and (aux.to_numpy() == 3).all()
    m3 = [None, masks[1], None]
    for op, name in ((R.FIRST, "first"), (R.SUM, "sum")):
        out, aux = ec.composite(mixed, name, min_count=3, aux=True)
        assert isinstance(out, ec.MaskedCellBuffer) and isinstance(aux, ec.CellBuffer)
        wc, wm, wa = R.composite(op, ct, layers, m3, 3)
        assert R.same_cells(out.buffer().to_numpy(), wc).all() and np.array_equal(out.mask().to_numpy(), wm) and np.array_equal(aux.to_numpy(), wa)
    assert isinstance(ec.composite(mixed), ec.MaskedCellBuffer)
    empty = ec.composite([ec.CellBuffer.from_vec(np.zeros(0, np.int16))] * 2, "sum", aux=True)
    assert empty[0].len() == 0 and empty[0].cell_type() == ec.Float64 and empty[1].len() == 0
    for bad, text in (([], "layers"), (plain * 22, "EC_COMPOSITE_MAX_LAYERS"), ([plain[0], ec.CellBuffer.from_vec(layers[0].astype(np.int32))], "cell type"),
                      ([plain[0], ec.CellBuffer.from_vec(layers[0][:5])], "cells"), ([plain[0], masks[0]], "not a CellBuffer")):
        with pytest.raises(ec.EcError, match=text):
            ec.composite(bad)
    for mc in (0, 4, True, 1.0):
        with pytest.raises(ec.EcError, match="min_count"):
            ec.composite(plain, min_count=mc)
    with pytest.raises(ec.EcError, match="operation"):
        ec.composite(plain, "median")


def test_cpp_mirror_composite_program():
    """erased-cells_amd/host/test_composite_mirror.cpp: the C++ mirror's composite, whole-buffer and sharded, on cells worked out by hand"""
    import os
    import subprocess
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "erased-cells_amd", "host")
    binary = os.path.join(host, "test_composite_mirror")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", host, "-s", "test_composite_mirror"])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
