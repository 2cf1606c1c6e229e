"""ec_composite_rank on the GPU against tests/composite_rank_ref.py, bit for bit on the raw bytes — cells, mask and aux: every cell
type x every stack height on both sides of every bucket edge, masks none / all / some entries NULL, both methods, q in (0, 1/4, 1/2,
9/10, 1), min_count 1, the middle and K, lengths of one to three tiles with a partial last group at every cells-per-lane, odd cell
offsets under both settings of "unaligned_vector", NaNs of both signs among the valid cells, a layer passed twice.
tests/test_composite_rank_faults.py shows that these inputs expose each modelled kernel mistake."""
import ctypes as C

import numpy as np
import pytest

import composite_ref as CR
import composite_rank_ref as R

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
        self.od = R.ordered(ct, layers, masks)       # the reference's expensive half, once per stack

    def _up(self, a, off_bytes):
        mem = self.ec.DeviceMem(a.nbytes + 512)
        self._mem.append(mem)
        p = mem.ptr - mem.ptr % -256 + off_bytes
        self.ec._ffi.check(self.ec.lib().ec_upload(p, np.ascontiguousarray(a).ctypes.data_as(C.c_void_p), a.nbytes, self.ec.stream()))
        return p

    def run(self, num, den, method, min_count, aux=True, off=0, mask_out=None):
        """(cells, mask or None, aux or None) as the device computed them; a mask comes back when a layer has one (or mask_out)"""
        ec, L, n = self.ec, self.ec.lib(), self.n
        dt = R.NP[self.ct]
        masked = (self.masks is not None and any(m is not None for m in self.masks)) if mask_out is None else mask_out
        outs = []
        for want, size in ((True, n * dt.itemsize), (masked, n), (aux, n)):
            mem = ec.DeviceMem(size + 512) if want else None
            outs.append((mem, None if mem is None else mem.ptr - mem.ptr % -256 + off * (dt.itemsize if not outs else 1)))
        ec._ffi.check(L.ec_composite_rank(self.ct, self.lp, self.mp, self.k, n, num, den, method, min_count, outs[0][1], outs[1][1], outs[2][1],
                                          ec.stream()))
        res = []
        for (mem, p), t in zip(outs, (dt, np.dtype(np.uint8), np.dtype(np.uint8))):
            if mem is None:
                res.append(None)
                continue
            a = np.empty(n, t)
            ec._ffi.check(L.ec_download(a.ctypes.data_as(C.c_void_p), p, a.nbytes, ec.stream()))
            res.append(a)
        return res

    def want(self, num, den, method, min_count):
        return R.pick(self.ct, self.od, num, den, method, min_count)


def check(got, want, where):
    cells, mask, aux = got
    wc, wm, wa = want
    assert R.same_cells(cells, wc).all(), (where, "cells", int(np.flatnonzero(~R.same_cells(cells, wc))[0]))
    if mask is not None:
        assert np.array_equal(mask, wm), (where, "mask", int(np.flatnonzero(mask != wm)[0]))
    else:
        assert wm.all(), (where, "no mask came back, yet a cell is invalid")
    if aux is not None:
        assert np.array_equal(aux, wa), (where, "aux", int(np.flatnonzero(aux != wa)[0]))


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_every_stack_height_q_method_and_min_count(ec, ct, form):
    n = R.main_len(ct)
    for k in R.KS:
        layers, masks = R.stack(ct, k, n, form)
        s = Stack(ec, ct, layers, masks)
        for num, den in R.QS:
            for method in R.METHODS:
                for mc in R.min_counts(k):
                    check(s.run(num, den, method, mc), s.want(num, den, method, mc), (R.NAMES[ct], k, form, num, den, method, mc))


@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_short_lengths_and_lengths_around_a_tile(ec, ct):
    for k, form in ((3, "some"), (9, "all"), (33, "all")):
        for n in R.small_lengths(ct, k):
            layers, masks = R.stack(ct, k, n, form, seed=1)
            s = Stack(ec, ct, layers, masks)
            for num, den, method, mc in ((1, 2, R.LOWER, 1), (9, 10, R.UPPER, 2)):
                check(s.run(num, den, method, mc), s.want(num, den, method, mc), (R.NAMES[ct], n, k, form, num, den, method, mc))


@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_without_aux_and_without_a_result_mask(ec, ct):
    n = R.main_len(ct)
    for k in (2, 5):
        for form in ("none", "all"):
            layers, masks = R.stack(ct, k, n, form, seed=2)
            s = Stack(ec, ct, layers, masks)
            check(s.run(1, 2, R.UPPER, 1, aux=False), s.want(1, 2, R.UPPER, 1), (R.NAMES[ct], k, form, "no aux"))
            if form == "none":   # a result mask may be asked for all the same: it is always written, all ones here
                got = s.run(1, 2, R.LOWER, k, aux=True, mask_out=True)
                check(got, s.want(1, 2, R.LOWER, k), (R.NAMES[ct], k, form, "mask asked for"))
                assert got[1].all()


@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_the_ends_are_composite_min_and_max_on_the_device(ec, ct):
    """num = 0: the bits and the aux of ec_composite MIN; num = den: the bits of MAX, the aux the greatest k among equal keys"""
    n, L = R.main_len(ct), ec.lib()
    for k, form in ((5, "all"), (17, "some")):
        layers, masks = R.stack(ct, k, n, form, seed=7)
        s = Stack(ec, ct, layers, masks)
        for op, (num, den) in ((CR.MIN, (0, 3)), (CR.MAX, (3, 3))):
            got = s.run(num, den, R.LOWER, 2)
            outs = [ec.DeviceMem(n * R.NP[ct].itemsize), ec.DeviceMem(n), ec.DeviceMem(n)]
            ec._ffi.check(L.ec_composite(op, ct, s.lp, s.mp, k, n, 2, outs[0].ptr, outs[1].ptr, outs[2].ptr, ec.stream()))
            back = []
            for mem, t in zip(outs, (R.NP[ct], np.dtype(np.uint8), np.dtype(np.uint8))):
                a = np.empty(n, t)
                ec._ffi.check(L.ec_download(a.ctypes.data_as(C.c_void_p), mem.ptr, a.nbytes, ec.stream()))
                back.append(a)
            assert R.same_cells(got[0], back[0]).all() and np.array_equal(got[1], back[1])
            if op == CR.MIN:
                assert np.array_equal(got[2], back[2])
            else:
                assert (got[2] >= back[2]).all() and (got[2] > back[2]).any()


@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_the_same_layer_twice(ec, ct):
    n = R.main_len(ct)
    layers, masks = R.stack(ct, 3, n, "all", seed=3)
    s = Stack(ec, ct, layers, masks)
    order = (0, 1, 0, 2, 1, 1)
    twice_l, twice_m = [layers[i] for i in order], [masks[i] for i in order]
    s.k, s.lp, s.mp = len(order), (C.c_void_p * len(order))(*[s.lp[i] for i in order]), (C.c_void_p * len(order))(*[s.mp[i] for i in order])
    for method in R.METHODS:
        for mc in (1, 4):
            check(s.run(1, 2, method, mc), R.composite_rank(ct, twice_l, twice_m, 1, 2, method, mc), (R.NAMES[ct], method, mc))


@pytest.mark.parametrize("vector", (1, 0), ids=("unaligned_vector", "cellwise"))
@pytest.mark.parametrize("ct", range(R.NT), ids=R.NAMES)
def test_pointers_at_odd_cell_offsets(ec, ct, vector):
    """inputs and outputs one and three cells behind an aligned address: the vector kernels with under-aligned accesses, and — the knob
    off — the cell-wise kernels, one of every bucket"""
    n = R.main_len(ct)
    with ec.tuned(unaligned_vector=vector):
        for k, form, off in ((1, "all", 1), (2, "some", 3), (4, "all", 1), (5, "some", 1), (8, "all", 3), (16, "some", 1), (17, "all", 3), (64, "some", 1)):
            layers, masks = R.stack(ct, k, n, form, seed=4)
            s = Stack(ec, ct, layers, masks, off=off)
            for num, den, method in ((1, 2, R.LOWER), (9, 10, R.UPPER)):
                mc = min(2, k)
                check(s.run(num, den, method, mc, off=off), s.want(num, den, method, mc), (R.NAMES[ct], k, form, off, vector, num, den, method))


@pytest.mark.parametrize("ct", R.FLOATS, ids=[R.NAMES[t] for t in R.FLOATS])
def test_nans_among_the_valid_cells(ec, ct):
    """NaNs of several payloads and both signs, valid — the all-ones positive NaN, whose word is the greatest a valid layer can have,
    among them: bit for bit (a NaN is the greatest cell of the total order, a negative NaN the least)"""
    n = R.main_len(ct)
    ones = np.array([-1], np.int32 if ct == R.F32 else np.int64).view(R.NP[ct])[0]
    for k in (3, 8, 64):
        layers, masks = R.stack(ct, k, n, "all", seed=5)
        rng = np.random.default_rng(77 + k)
        for i, a in enumerate(layers):
            at = rng.random(n) < 0.05
            a[at] = np.where(rng.random(int(at.sum())) < 0.5, CR.nan_of(ct, 0x100 + i), -CR.nan_of(ct, 0x200 + i))
            a[rng.random(n) < 0.02] = np.abs(ones)
            a[rng.random(n) < 0.02] = ones
        assert any((np.isnan(a) & (m != 0)).any() for a, m in zip(layers, masks))
        s = Stack(ec, ct, layers, masks)
        for num, den in R.QS:
            for method in R.METHODS:
                want = s.want(num, den, method, 1)
                check(s.run(num, den, method, 1), want, (R.NAMES[ct], k, num, den, method))
        assert np.isnan(s.want(1, 1, R.LOWER, 1)[0]).any() and np.isnan(s.want(0, 1, R.LOWER, 1)[0]).any()


def test_cpp_mirror_composite_rank_program():
    """erased-cells_amd/host/test_composite_rank_mirror.cpp: the C++ mirror's composite_rank, whole-buffer and sharded, on cells worked
    out by hand"""
    import os
    import subprocess
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "erased-cells_amd", "host")
    binary = os.path.join(host, "test_composite_rank_mirror")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", host, "-s", "test_composite_rank_mirror"])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
