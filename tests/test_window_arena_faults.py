"""The arenas, offsets and shapes of tests/test_gpu_window_bounds.py notice the faults that file is for — checked without a GPU.

As in tests/test_arena_faults.py the kernel is a numpy model that writes the expected result into host arenas the way the window
kernels do, and each fault is one way that structure can go wrong.  Three models, one per store structure:

  * `run_cut` — k_window_copy / k_window_nearest: the value stream in 16-byte slots of CPL = 16 / W cells, whole slots as one store,
    the last partial slot cell by cell, tiles of 1024 slots; the mask stream in 16-byte slots of its own over the same cells;
  * `run_resample` — k_window_resample: the same value slots, the mask bytes of a slot as ONE store of CPL bytes by the lane that
    owns the slot, and the `!whole` arm (the last partial slot, or every slot under `cellwise_stores`) that stores a cell and its
    mask byte together;
  * `run_put` — k_window_put: a slot that lies in one row of the window as one store into the raster, any other cell by cell.

The shapes, the output offsets, the paste placements and the arenas are the GPU file's own (imported, so they cannot drift).  A
fault is a change of the model's STORES; where it has nothing to change (no partial slot when CPL divides n, no second tile below
T cells, ...) the mutated kernel is the correct one.  `APPLIES` says where each fault has an effect; the test asserts that `check`
or `check_unchanged` fails at every such case, passes at the others, and that every fault has an effect somewhere in the lists at
every width it can occur at.  No wrong kernel runs anywhere else, and none runs on a GPU.
"""
import numpy as np
import pytest

import test_gpu_window_bounds as B
from arena import Arena

SLOT = 16          # bytes per slot
TILE_SLOTS = 1024  # value slots per workgroup (kBlock 256 x kWindowU 4)


def _rng(*parts):
    return np.random.default_rng(abs(hash(parts)) & 0xFFFFFFFF)


def _differing(data, there):
    """`data`, except that no byte equals the byte it lands on: a stray store is a store of SOME value, and the one value an arena
    cannot see is the one that is already there"""
    data = data.copy()
    same = data == there
    data[same] ^= 0xFF
    return data


# ---------------------------------------------------------------- cut and resample: the contiguous side
def cut_cases():
    """(W, w, h, value offset in cells, mask offset in bytes): the GPU file's shapes under every pair of its output offsets"""
    return [(W, w, h, vo, mo) for W in B.WIDTHS for w, h in B.shapes(W) for vo, mo in B.offset_pairs(W, True)]


def cellwise_stores(W, vo, mo):
    """what ec_window_resample sets with unaligned_vector = 0: an output pointer that is not 16-byte aligned"""
    return (vo * W) % SLOT != 0 or mo % SLOT != 0


class Cut:
    """The arenas of one cut: the output values and mask as the GPU file places them, and the source window's raster."""

    def __init__(self, W, w, h, vo, mo):
        self.W, self.w, self.h, self.n, self.vo, self.mo = W, w, h, w * h, vo, mo
        rng = _rng(W, w, h)
        self.exp = rng.integers(0, 256, size=self.n * W, dtype=np.uint8)   # the expected cells, as bytes
        self.em = rng.integers(0, 2, size=self.n, dtype=np.uint8)
        self.beyond = rng.integers(0, 256, size=SLOT * W + SLOT, dtype=np.uint8)   # what a lane makes of whatever lies behind the window
        self.out = Arena(self.n * W, offset=vo * W, seed=self.n + vo).expect(self.exp)
        self.om = Arena(self.n, offset=mo, seed=self.n + mo + 1).expect(self.em)
        self.src = Arena(self.n * W, offset=W, seed=self.n + 2).hold(self.exp)   # the window's cells stand for the raster

    def check(self, what):
        self.out.check(self.exp.view(f"u{self.W}"), f"{what}: values")
        self.om.check(self.em, f"{what}: mask")
        self.src.check_unchanged(f"{what}: source")


def _store(arena, at, data, stray=False):
    """`data` at byte `at` of the payload (negative: in front of it; beyond its end: behind it)"""
    lo = arena.lo + at
    data = data[:max(0, arena.mem.size - lo)]   # the image ends with the high guard: what a stray store writes behind it no arena sees
    arena.mem[lo:lo + data.size] = _differing(data, arena.mem[lo:lo + data.size]) if stray else data


def _unstore(arena, first, last):
    """bytes [first, last) of the payload as they were before the call: never stored"""
    arena.mem[arena.lo + first:arena.lo + last] = arena.before[arena.lo + first:arena.lo + last]


def _value_stream(c, fault):
    """the value slots of a cut: whole slots as 16-byte stores, the cells of the last partial slot one by one"""
    W, n, cpl = c.W, c.n, SLOT // c.W
    whole = n // cpl * cpl
    shift = (c.vo * W) % SLOT if fault == "whole_slots_at_dst_rounded_down" else 0
    _store(c.out, -shift, c.exp[:whole * W], stray=shift != 0)
    if fault == "last_slot_stored_whole" and n % cpl:
        _store(c.out, whole * W, np.concatenate([c.exp[whole * W:], c.beyond])[:SLOT], stray=True)
    elif fault != "last_partial_slot_skipped":
        _store(c.out, whole * W, c.exp[whole * W:])


def _skip_a_tile(c):
    """the middle tile of the launch is never run: neither its values nor its mask bytes are stored"""
    cells_per_tile = TILE_SLOTS * SLOT // c.W
    ntiles = -(-c.n // cells_per_tile)
    if ntiles < 2:
        return
    first, last = ntiles // 2 * cells_per_tile, min(c.n, (ntiles // 2 + 1) * cells_per_tile)
    _unstore(c.out, first * c.W, last * c.W)
    _unstore(c.om, first, last)


def run_cut(c, fault=None):
    W, n, cpl = c.W, c.n, SLOT // c.W
    _value_stream(c, fault)
    # the mask stream: 16-byte slots of its own
    mwhole = n // SLOT * SLOT
    if fault == "mask_at_the_value_slot_offset":
        for m0 in range(0, mwhole, SLOT):   # slot m of the mask stored where slot m of the values lies: m * 16 * W bytes in
            _store(c.om, m0 * W, c.em[m0:m0 + SLOT], stray=W > 1 and m0 > 0)
    else:
        _store(c.om, 0, c.em[:mwhole])
    if fault == "mask_slot_whole_when_the_value_slot_is" and n % SLOT and mwhole + cpl <= n:
        _store(c.om, mwhole, np.concatenate([c.em[mwhole:], c.beyond])[:SLOT], stray=True)
    elif fault != "last_partial_slot_skipped":
        _store(c.om, mwhole, c.em[mwhole:])
    if fault == "tile_skipped":
        _skip_a_tile(c)
    if fault == "store_into_the_source":
        _store(c.src, 0, c.exp[:W], stray=True)


def run_resample(c, cellwise, fault=None):
    """the stores of k_window_resample: per whole value slot one 16-byte store and one store of its CPL mask bytes; the `!whole`
    arm — a cell and its mask byte together — for the last partial slot, or for every slot when `cellwise`"""
    W, n, cpl = c.W, c.n, SLOT // c.W
    part = n // cpl * cpl               # the first cell of the last partial slot
    vec = 0 if cellwise else part       # the cells below `vec` go through whole-slot stores
    shift = (c.vo * W) % SLOT if fault == "whole_slots_at_dst_rounded_down" else 0
    _store(c.out, -shift, c.exp[:vec * W], stray=shift != 0)
    _store(c.om, 0, c.em[:vec])
    if fault == "last_slot_stored_whole" and not cellwise and n % cpl:
        _store(c.out, part * W, np.concatenate([c.exp[part * W:], c.beyond])[:SLOT], stray=True)
        _store(c.om, part, np.concatenate([c.em[part:], c.beyond])[:cpl], stray=True)
    else:
        last = part if fault == "last_partial_slot_skipped" else n
        _store(c.out, vec * W, c.exp[vec * W:last * W])
        if fault != "cellwise_arm_stores_no_mask_byte":
            _store(c.om, vec, c.em[vec:last])
    if fault == "tile_skipped":
        _skip_a_tile(c)
    if fault == "store_into_the_source":
        _store(c.src, 0, c.exp[:W], stray=True)


def _tiles(W, n):
    return -(-n // (TILE_SLOTS * SLOT // W))


CUT_FAULTS = {
    # fault: (the model it is planted in, where it changes what the model stores)
    "last_slot_stored_whole": ("cut", lambda W, n, vo, mo: n % (SLOT // W) != 0),
    "mask_slot_whole_when_the_value_slot_is": ("cut", lambda W, n, vo, mo: n % SLOT != 0 and n % SLOT >= SLOT // W),
    "tile_skipped": ("cut", lambda W, n, vo, mo: _tiles(W, n) >= 2),
    "last_partial_slot_skipped": ("cut", lambda W, n, vo, mo: n % SLOT != 0),   # the mask's partial slot, and the values' where CPL does not divide n
    "mask_at_the_value_slot_offset": ("cut", lambda W, n, vo, mo: W > 1 and n >= 2 * SLOT),
    "cellwise_arm_stores_no_mask_byte": ("resample", lambda W, n, vo, mo: cellwise_stores(W, vo, mo) or n % (SLOT // W) != 0),
    "store_into_the_source": ("cut", lambda W, n, vo, mo: True),
    "whole_slots_at_dst_rounded_down": ("cut", lambda W, n, vo, mo: (vo * W) % SLOT != 0 and n >= SLOT // W),
}
# the widths at which a fault can occur at all: a mask slot is a value slot at 1-byte cells
CUT_FAULT_WIDTHS = {"mask_slot_whole_when_the_value_slot_is": (2, 4, 8), "mask_at_the_value_slot_offset": (2, 4, 8)}
# the faults that k_window_resample's stores share with the copies', and where they change what ITS model stores (cw: cellwise_stores)
RESAMPLE_APPLIES = {
    "last_slot_stored_whole": lambda W, n, vo, cw: not cw and n % (SLOT // W) != 0,
    "tile_skipped": lambda W, n, vo, cw: _tiles(W, n) >= 2,
    "last_partial_slot_skipped": lambda W, n, vo, cw: n % (SLOT // W) != 0,
    "store_into_the_source": lambda W, n, vo, cw: True,
    "whole_slots_at_dst_rounded_down": lambda W, n, vo, cw: not cw and (vo * W) % SLOT != 0 and n >= SLOT // W,
}


def _expect(applies, check, what):
    if applies:
        with pytest.raises(AssertionError):
            check(what)
    else:
        check(what)   # nothing for the fault to change here: the model is the correct kernel


def test_the_fault_free_model_passes():
    for case in cut_cases():
        W, w, h, vo, mo = case
        c = Cut(*case)
        run_cut(c)
        c.check(("cut", case))
        for cellwise in (False, True):
            c = Cut(*case)
            run_resample(c, cellwise)
            c.check(("resample", cellwise, case))
    for case in put_cases():
        p = Put(*case)
        run_put(p)
        p.check(("put", case))


@pytest.mark.parametrize("fault", sorted(CUT_FAULTS))
def test_every_fault_of_the_contiguous_side_is_caught(fault):
    model, applies = CUT_FAULTS[fault]
    effect = {W: 0 for W in B.WIDTHS}
    for case in cut_cases():
        W, w, h, vo, mo = case
        c = Cut(*case)
        if model == "cut":
            run_cut(c, fault)
        else:
            run_resample(c, cellwise_stores(W, vo, mo), fault)
        hit = applies(W, w * h, vo, mo)
        effect[W] += hit
        _expect(hit, c.check, (fault, case))
    for W in CUT_FAULT_WIDTHS.get(fault, B.WIDTHS):
        assert effect[W] >= 1, (fault, W)
    assert all(effect[W] == 0 for W in B.WIDTHS if W not in CUT_FAULT_WIDTHS.get(fault, B.WIDTHS))


@pytest.mark.parametrize("fault", sorted(RESAMPLE_APPLIES))
def test_the_resampling_stores_with_the_same_faults(fault):
    """the faults that k_window_resample's value stream shares with the copies, under both knob arms of the GPU file: whole-slot
    stores wherever the output sits, and `cellwise_stores` wherever it is misaligned"""
    effect = {W: 0 for W in B.WIDTHS}
    for case in cut_cases():
        W, w, h, vo, mo = case
        for knob_off in (False, True):
            cw = knob_off and cellwise_stores(W, vo, mo)
            c = Cut(*case)
            run_resample(c, cw, fault)
            hit = RESAMPLE_APPLIES[fault](W, w * h, vo, cw)
            effect[W] += hit
            _expect(hit, c.check, (fault, case, knob_off))
    assert all(effect[W] >= 1 for W in B.WIDTHS), (fault, effect)


# ---------------------------------------------------------------- paste: the raster side
def put_cases():
    """(W, w, h, x0, tile offset in cells, tile mask offset in bytes): the GPU file's shapes at each of its placements"""
    return [(W, w, h, x0, to, tmo) for W in B.WIDTHS for w, h in B.shapes(W) for x0 in B.put_x0s(W) for to, tmo in ((0, 0), (1, 1))]


class Put:
    """The arenas of one paste, as the GPU file builds them: the destination raster and its mask with the window pre-filled
    with the complement of the tile, the tile and its mask as operands."""

    def __init__(self, W, w, h, x0, to, tmo):
        self.W, self.w, self.h, self.n, self.x0 = W, w, h, w * h, x0
        self.cols, self.rows = B.put_cols(x0, w), h + 2
        rng = _rng(W, w, h, x0)
        self.t = rng.integers(0, 256, size=(h, w, W), dtype=np.uint8)
        self.tm = rng.integers(0, 2, size=(h, w), dtype=np.uint8)
        base = rng.integers(0, 256, size=(self.rows, self.cols, W), dtype=np.uint8)
        bm = rng.integers(2, 256, size=(self.rows, self.cols), dtype=np.uint8)
        base[1:1 + h, x0:x0 + w], bm[1:1 + h, x0:x0 + w] = ~self.t, self.tm ^ 1
        self.exp, self.expm = base.copy(), bm.copy()
        self.exp[1:1 + h, x0:x0 + w], self.expm[1:1 + h, x0:x0 + w] = self.t, self.tm
        self.dst = Arena(base.size, seed=self.n + x0).hold(base)
        self.dm = Arena(bm.size, seed=self.n + x0 + 1).hold(bm)
        self.tile = Arena(self.t.size, offset=to * W, seed=self.n + 2).hold(self.t)
        self.tmask = Arena(self.tm.size, offset=tmo, seed=self.n + 3).hold(self.tm)

    def check(self, what):
        self.dst.check(self.exp, f"{what}: values")
        self.dm.check(self.expm, f"{what}: mask")
        self.tile.check_unchanged(f"{what}: tile")
        self.tmask.check_unchanged(f"{what}: tile mask")


def straddling_slots(w, n, cpl):
    """first cells of the whole slots that run over a row end of the window"""
    c0 = np.arange(0, n // cpl * cpl, cpl)
    return c0[c0 % w + cpl > w]


def _put_stream(arena, cells, p, cpl, fault):
    """cells: (n, bytes per cell).  Cell c of the tile goes to cell origin + row * pitch + col of the raster."""
    n, width = cells.shape
    c = np.arange(n)
    step = p.w if fault == "row_step_w_instead_of_the_pitch" else p.cols
    at = p.cols + p.x0 + c // p.w * step + c % p.w
    if fault == "slot_stored_across_a_row_end":
        for c0 in straddling_slots(p.w, n, cpl):   # one 16-byte store where the slot begins: on over the row end
            at[c0:c0 + cpl] = at[c0] + np.arange(cpl)
    image = arena.mem[arena.lo:arena.lo + arena.nbytes].reshape(-1, width)
    image[at] = cells


def run_put(p, fault=None):
    _put_stream(p.dst, p.t.reshape(p.n, p.W), p, SLOT // p.W, fault)
    _put_stream(p.dm, p.tm.reshape(p.n, 1), p, SLOT, fault)


PUT_FAULTS = {
    "slot_stored_across_a_row_end": lambda W, w, h: straddling_slots(w, w * h, SLOT // W).size > 0 or straddling_slots(w, w * h, SLOT).size > 0,
    "row_step_w_instead_of_the_pitch": lambda W, w, h: h > 1,
}


@pytest.mark.parametrize("fault", sorted(PUT_FAULTS))
def test_every_fault_of_a_paste_is_caught(fault):
    effect = {W: 0 for W in B.WIDTHS}
    for case in put_cases():
        W, w, h, x0, to, tmo = case
        p = Put(*case)
        run_put(p, fault)
        hit = PUT_FAULTS[fault](W, w, h)
        effect[W] += hit
        _expect(hit, p.check, (fault, case))
    assert all(effect[W] >= len(B.put_x0s(W)) for W in B.WIDTHS), (fault, effect)


def test_check_names_the_cell_and_the_side():
    """what a failing case of the GPU file would print"""
    W = 8
    c = Cut(W, B.tile(W) - 1, 1, 1, 3)      # n % 16 = 15: the last value slot but one is whole, the mask slot is not
    run_cut(c, "mask_slot_whole_when_the_value_slot_is")
    with pytest.raises(AssertionError, match=r"mask: .* first at byte n \+ 0: 0 bytes behind the payload's n = \d+ bytes \(guard overwritten\)"):
        c.check("probe")
    c = Cut(W, 2 * B.tile(W) + B.cpl(W) + 3, 1, 1, 3)   # three tiles: the second is left out
    run_cut(c, "tile_skipped")
    with pytest.raises(AssertionError, match=r"values: .* first at cell 2048 .*never written"):
        c.check("probe")
