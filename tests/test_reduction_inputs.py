"""The inputs of tests/test_gpu_reduction_positions.py are sensitive to WHERE the answer sits — checked here without a GPU.

A reduction returns one or two words, and over `rand_cells` many cells hold each of them: a kernel that dropped the ragged
tail, one element slot of a 16-byte group, lane 0 of every wave, wave 3 of tile 0, the last partial tile, the first or the
last cell, or every even byte would have left the answer of `test_min_max_total_order` (ten types, n in {255, 4096, 100003,
2^21}, seed 61) unchanged in 479 of 484 fault x input combinations when the gap was measured (460 of 482 as
`rand_cells_contrast` below counts them: it drops the whole last tile where the first count dropped less);
`test_rand_cells_contrast` prints today's share.  The cases of reduction_cases.py hold each answer in ONE cell, and every fault model — one position
class left out of the fold, or the mask ignored in the head, the tail or one element slot — must change the reference answer of
at least one case: none may go undetected.  The fold used is reduction_cases.fold_min_max, a numpy restatement of the total
order that is itself checked against the oracle (`eco.f_min_max`) on the same arrays.
"""
import numpy as np
import pytest

import reduction_cases as rc
from oracle import eco
from vectors import rand_cells, rand_mask

NT = eco.NTYPES
# The geometry of the capped-grid windows depends on the CU count: the GPU test reads it from the device, this file assumes the
# MI355X's 256, so both see the same list of cases on a 256-CU part only.  To stay short it also checks the capped grids for two
# types (reduce_bpc = 100 for i64 alone, whose window has the fewest cells) and the generated kernel for f64 and for i64 seen as f64.
CUS = 256


def _oracle_bits(a, m=None):
    mn, mx = eco.f_min_max(a, m)
    return mn.bits(), mx.bits()


@pytest.mark.parametrize("ct", range(NT))
def test_fold_restates_the_oracle(ct):
    """fold_min_max against eco.f_min_max: rand_cells (specials, NaN payloads, signed zeros), every order kind, plain, masked, empty."""
    for n in (0, 1, 255, 4099):
        a, m = rand_cells(ct, n, 21), rand_mask(n, 22)
        assert rc.fold_min_max(a) == _oracle_bits(a)
        assert rc.fold_min_max(a, m) == _oracle_bits(a, m)
        assert rc.fold_min_max(a, np.zeros(n, np.uint8)) == _oracle_bits(a, np.zeros(n, np.uint8))
    for kind in rc.kinds_of(ct):
        a = rc.sole_extreme_cells(ct, 3001, 7, 2998, 4, kind)
        assert rc.fold_min_max(a) == _oracle_bits(a), kind


@pytest.mark.parametrize("ct", range(NT))
def test_every_order_kind_has_a_sole_holder(ct):
    """Every kind of section 'fields and plants' applies to the types it should, the oracle returns the planted pair, and without
    the planted cell it returns something else: the plant is the SOLE holder.  The masked variant hides values beyond the plants."""
    want = rc.KINDS_FLOAT if ct in (eco.F32, eco.F64) else rc.KINDS_INT8 if ct in (eco.U64, eco.I64) else rc.KINDS_INT
    assert rc.kinds_of(ct) == want
    n = 4001
    for kind in want:
        for i_min, i_max in ((0, n - 1), (n - 1, 0), (1234, 1235)):
            a = rc.sole_extreme_cells(ct, n, i_min, i_max, 9, kind)
            mn, mx, _ = rc.plant_bits(ct, kind, rc._band_block(ct, 9, kind))
            got = _oracle_bits(a)
            for side, (plant, at) in enumerate(((mn, i_min), (mx, i_max))):
                if plant is None:
                    continue
                assert got[side] == plant == int(rc.as_bits(a)[at]), (kind, side)
                assert _oracle_bits(np.delete(a, at))[side] != plant, (kind, side, "not the sole holder")
            b = a.copy()
            mask = rc.hide_decoys(ct, b, [i_min, i_max])
            assert _oracle_bits(b, mask) == got, kind
            if (mn, mx) != rc.decoy_bits(ct):   # (i64 / integer extremes: the plants ARE the type's MIN / MAX, nothing lies beyond)
                assert _oracle_bits(b) != got, kind
    if ct in (eco.U64, eco.I64):   # the pairs f64 cannot tell apart really are one f64
        for kind in ("blind63", "blind53"):
            mn, mx, runners = rc.plant_bits(ct, kind, rc._band_block(ct, 9, kind))
            vals = np.array([mx, runners[0]], np.uint64).view(rc.dtype_of(ct))
            assert vals[0] != vals[1] and float(vals[0]) == float(vals[1]), kind
    if ct == eco.U64:              # cells on both sides of 2^63: the top bit the kernel's key flips
        a = rc.field_cells(ct, 4001, 9)
        assert (a < 2**63).any() and (a >= 2**63).any()


def _pools(ct, cases):
    pools = {}
    for kind in sorted({c.kind for c in cases}):
        n = max(c.window.ge.n + c.window.ge.cpl for c in cases if c.kind == kind)
        pools[kind] = rc.HostPool(ct, n, 5, kind)
    return pools


def _premise(ct, pools, cases):
    """The oracle's answer for every case IS the planted pair (what the GPU test asserts before it asks the GPU)."""
    for c in cases:
        pool = pools[c.kind]
        off = pool.offset(c.window.ge)
        cells, mask = pool.arrays(c)
        ce, me, want = rc.case_edits(ct, c, pool.block)
        old_c, old_m = pool.poke(cells, off, ce), (pool.poke(mask, off, me) if c.masked else {})
        got = _oracle_bits(cells[off:off + c.window.ge.n], mask[off:off + c.window.ge.n] if c.masked else None)
        pool.poke(cells, off, old_c)
        if c.masked:
            pool.poke(mask, off, old_m)
        for side in (0, 1):
            assert want[side] is None or got[side] == want[side], (c.label(), side, got, want)


@pytest.mark.parametrize("ct", range(NT))
def test_every_fault_is_detected(ct):
    """Vector kernel, every launch shape, plus the order kinds: the oracle returns the planted pair for every case, and no fault
    model goes undetected."""
    for shape in rc.SHAPES:
        cases = rc.min_max_cases(ct, shape)
        pools = _pools(ct, cases)
        if shape == 0:
            _premise(ct, pools, cases)
        missed, total = rc.undetected(pools["adjacent"], cases)
        assert total > 100 and not missed, (eco.CT_NAMES[ct], shape, missed)
    cases = rc.order_cases(ct)
    pools = _pools(ct, cases)
    _premise(ct, pools, cases)
    assert {c.kind for c in cases} == set(rc.kinds_of(ct))
    for kind, pool in pools.items():
        mn, mx, _ = rc.plant_bits(ct, kind, pool.block)
        ks = [c for c in cases if c.kind == kind]
        hit = set()
        for c in ks:   # leaving out the planted cell changes the answer at every reduced position
            for name, at, plant in ((c.name_min, c.i_min, mn), (c.name_max, c.i_max, mx)):
                if plant is not None and at is not None:
                    drop = np.zeros(c.window.ge.n, bool)
                    drop[at] = True
                    assert rc.detect(pool, c, drop=drop), (kind, c.label())
                    hit.add(name)
        assert set(rc.ORDER_CLASSES) <= hit, (kind, hit)


@pytest.mark.parametrize("ct", [eco.F32, eco.I64])
def test_every_fault_of_the_capped_grids_is_detected(ct):
    """reduce_bpc = 1 (later rounds of the grid-stride loop), the cell-wise kernel (stride 256 x grid), and — on the 8-byte type,
    whose window has the fewest cells — reduce_bpc = 100: the hard cap of 4096 workgroups and the finalize kernel's four load slots."""
    cases = [c for c in rc.capped_cases(ct, CUS) if c.window.name == "rounds" or ct == eco.I64] + rc.cellwise_cases(ct, CUS)
    pools = _pools(ct, cases)
    for c in cases[::7]:
        _premise(ct, pools, [c])
    missed, total = rc.undetected(pools["adjacent"], cases)
    assert not missed, (eco.CT_NAMES[ct], missed)
    names = set()
    for w in {c.window.name: c.window for c in cases}.values():
        names |= set(rc.position_classes(w.ge.n, w.ge.cell_size, w.ge.block, w.ge.u, w.ge.head, w.ge.grid, w.ge.cpg))
    assert {"round1", "round_last"} <= names
    if ct == eco.I64:
        assert {"partial_word1023", "partial_word1024", "partial_word2047", "partial_word2048", "partial_word3072", "wg4095"} <= names


@pytest.mark.parametrize("ct", [eco.F64, eco.I64, eco.U64])
def test_every_fault_of_the_generated_kernel_is_detected(ct):
    """The generated reduce kernel's geometry (pairs, 256 x 4, head cell and odd tail cell, a grid of 8 per CU), on what the kernel
    folds: the oracle's f64 image of the cells (`s0 * 1.0`).  8-byte integers round on the way, so their plants lie 2^13 beyond the
    band (kind "wide"): every plant must still be the only holder of its f64 value."""
    one = eco.Value.of(eco.F64, 1.0)
    image = lambda a: eco.f_binop_scalar(eco.MUL, a, one)   # noqa: E731
    kind = rc.expr_kind(ct)
    for head in (0, 1):
        cases = []
        for w in rc.jit_windows(CUS, head):
            cases += rc.rotate_cases(w, kind) + rc.rotate_cases(w, kind, masked=True)
        pools = _pools(ct, cases)
        pool = pools[kind]
        mn, mx, _ = rc.plant_bits(ct, kind, pool.block)
        want = tuple(int(rc.as_bits(image(np.array([b], rc._UINT[8]).view(rc.dtype_of(ct))))[0]) for b in (mn, mx))
        for c in cases[::3]:   # the premise: the oracle's answer is the plant's f64 image, held by the planted cell alone
            off = pool.offset(c.window.ge)
            cells, mask = pool.arrays(c)
            ce, me, _ = rc.case_edits(ct, c, pool.block)
            old_c, old_m = pool.poke(cells, off, ce), (pool.poke(mask, off, me) if c.masked else {})
            vals = image(cells[off:off + c.window.ge.n])
            m = mask[off:off + c.window.ge.n] if c.masked else None
            got = _oracle_bits(vals, m)
            valid = np.ones(vals.size, bool) if m is None else m.astype(bool)
            holders = [np.flatnonzero((rc.as_bits(vals) == w_) & valid).tolist() for w_ in want]
            pool.poke(cells, off, old_c)
            if c.masked:
                pool.poke(mask, off, old_m)
            assert got == want and holders == [[c.i_min], [c.i_max]], (c.label(), got, want, [h[:3] for h in holders])
        missed, total = rc.undetected(pool, cases, image=image)
        assert not missed, (head, missed)


@pytest.mark.parametrize("size", [1, 2, 4, 8])
def test_difference_and_count_inputs_are_sensitive(size):
    """first_difference / cmp and mask_counts over the same position classes: with the class of the planted cell left out, the
    oracle's `buffer_cmp` says "equal" and its `mask_counts` loses the sole true (or the sole false) cell."""
    ct = {1: eco.U8, 2: eco.I16, 4: eco.F32, 8: eco.U64}[size]
    w = [x for x in rc.min_max_windows(size, 0) if x.name == "main"][0]
    ge = w.ge
    a = rc.field_cells(ct, ge.n, 3)
    pos = rc.window_positions(w)
    fs = rc.faults(ge)
    assert eco.buffer_cmp(a, a.copy()) == 0
    for name, drop in fs.items():
        at = [i for _, i in pos if drop[i]]
        assert at, name
        b = rc.sole_difference(a, at[0])
        assert eco.buffer_cmp(a, b) == -1 and eco.buffer_cmp(a[~drop], b[~drop]) == 0, name
        if size == 1:
            t, f = rc.sole_true_mask(ge.n, at[0]), rc.sole_false_mask(ge.n, at[0])
            assert eco.mask_counts(t) == (1, ge.n - 1) and eco.mask_counts(t[~drop])[0] == 0, name
            assert eco.mask_counts(f) == (ge.n - 1, 1) and eco.mask_counts(f[~drop])[1] == 0, name
    # two differences: the later one is the larger cell, so the ordering tells which was found
    b = rc.sole_difference(a, pos[3][1], later=[i for _, i in pos if i > pos[3][1]][:1])
    assert eco.buffer_cmp(a, b) == -1 and eco.buffer_cmp(a[pos[3][1] + 1:], b[pos[3][1] + 1:]) == 1


def rand_cells_contrast():
    """(undetected, total) over the inputs of test_min_max_total_order for the fault list of the module docstring."""
    undetected = total = 0
    for ct in range(NT):
        size = rc.dtype_of(ct).itemsize
        for n in (255, 4096, 100003, 1 << 21):
            a = rand_cells(ct, n, 61)
            ge = rc.Geometry(n, size, *rc.SHAPES[0])
            body, tile, j, th, k = ge.coords()
            idx = np.arange(n)
            drops = [idx >= ge.ngroups * ge.cpl] + [body & (k == s) for s in range(ge.cpl)]
            drops += [body & (th % rc.WAVE == 0), body & (tile == 0) & (th // rc.WAVE == 3), body & (tile == ge.ntiles - 1),
                      idx == 0, idx == n - 1, (np.arange(n * size) % 2 == 0).reshape(n, size).all(axis=1) if size == 1 else None]
            want = rc.fold_min_max(a)
            for d in drops:
                if d is None or not d.any():
                    continue
                total += 1
                undetected += rc.fold_min_max(a, keep=~d) == want
    return undetected, total


def test_rand_cells_contrast():
    """The recorded contrast: how many faults the rand_cells inputs cannot see (479 of 484 when the gap was measured).  Nothing
    is asserted about the share but that the helper reports it."""
    undetected, total = rand_cells_contrast()
    print(f"rand_cells inputs of test_min_max_total_order: {undetected} of {total} faults leave (min, max) unchanged")
    assert 0 <= undetected <= total and total > 0
