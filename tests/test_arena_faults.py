"""The arenas of tests/arena.py notice what they are for — checked here without a GPU.

tests/test_gpu_output_bounds.py trusts `Arena.check` to see a kernel that stores outside its `n` cells or skips one of them.  Here
the kernel is a numpy model that writes the expected result into a host arena the way the streaming frame does (the pair grid of
`stream_tile` / `binop_direct_body`: `head` peeled cells, pairs of f64 cells in tiles of 512 pairs, the odd tail cell; and the
mask phase: 16-byte groups, then the remainder by cell), and each fault model is one way that frame can go wrong.  No wrong
kernel runs anywhere else, and none runs on a GPU.

A fault is a change of the model's STORES.  At some (n, head) a fault has nothing to change — no head cell when head = 0, no
tail cell when n - head is even, no guarded tile when the pairs fill their tiles, no remainder when 16 divides n, no second
tile below 1025 cells — and the mutated kernel is then the correct one: `APPLIES` says where each fault has an effect, the
test asserts that `check` fails at every such (n, head), that it passes at the others, and that every fault has an effect at
most of the list.  n = 0 launches nothing, so only the fault-free model has a case there.
"""
import re

import numpy as np
import pytest

from arena import Arena, GUARD

T = 1024                 # cells per tile of the pair grid (kBlock 256 x U 2 pairs)
PAIRS = T // 2
BASE = [0, 1, 2, 3, 4, 15, 16, 17, 31, 33, 255, 256, 257]
SIZES = sorted(set(BASE + [T - 1, T, T + 1, T + 2, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 7] + [T + 3, 2 * T + 2, 3 * T + 8]))
CASES = [(n, head) for n in SIZES for head in (0, 1) if head == 0 or n >= 2]   # peel_head peels nothing below two cells


def expected_cells(n, seed=1):
    """n distinct f64 results (random bit patterns: no two cells, and no cell and its neighbour's half, coincide)."""
    return np.random.default_rng(seed).integers(1, 1 << 62, size=n, dtype=np.int64).view(np.float64)


def geometry(n, head):
    npairs = (n - head) >> 1
    ntiles = max(1, (npairs + PAIRS - 1) // PAIRS)   # grid_for: at least one workgroup
    return npairs, ntiles


# ---------------------------------------------------------------- the model: the value stream
def run_values(arena, exp, n, head, fault=None):
    """Writes `exp` into the host arena as the pair-grid frame does, with one fault.  Cell i of the output is bytes
    [lo + 8 i, lo + 8 i + 8) of the image; the model may address cells in front of and behind the payload, as a kernel can."""
    mem, lo = arena.mem, arena.lo
    npairs, ntiles = geometry(n, head)
    beyond = expected_cells(2 * T + 4, seed=99)   # what a lane computes from whatever lies behind the operands

    def value(i):
        return exp[i] if 0 <= i < n else beyond[i - n]

    def store(i, v):
        mem[lo + 8 * i:lo + 8 * i + 8] = np.array([v]).view(np.uint8)

    def store_pair(pr, at=None):
        i = head + 2 * pr
        at = i if at is None else at
        store(at, value(i))
        store(at + 1, value(i + 1))

    for tile in range(ntiles):
        full = tile * PAIRS + PAIRS <= npairs
        if fault == "middle_tile_skipped" and ntiles >= 3 and tile == ntiles // 2:
            continue
        for pr in range(tile * PAIRS, tile * PAIRS + PAIRS):
            guard = pr < npairs
            if fault == "last_tile_unguarded" and tile == ntiles - 1:
                guard = True
            if fault == "pr_le_npairs":
                guard = pr <= npairs
            if not (full or guard):
                continue
            if fault == "front_tiles_swapped" and ntiles >= 2 and tile in (0, ntiles - 1):
                # the two fronts (workgroups 0 and 1 of two_front_tile) store each other's values: the pair computed for the
                # first tile lands in the last one and the reverse, under the destination's guard
                other = pr + (ntiles - 1) * PAIRS if tile == 0 else pr - (ntiles - 1) * PAIRS
                if other < npairs:
                    store_pair(pr, at=head + 2 * other)
                continue
            store_pair(pr)
    if head:
        if fault == "head_at_minus_1":
            store(-1, exp[0])
        elif fault != "head_never_stored":
            store(0, exp[0])
    if (n - head) & 1:
        if fault == "tail_at_n":
            store(n, exp[n - 1])
        elif fault != "tail_never_stored":
            store(n - 1, exp[n - 1])
    if fault == "group_twice_shifted_8" and npairs >= 1:
        # the last pair's 16 bytes once more, 8 bytes on; modelled as the last store to land
        i = head + 2 * (npairs - 1)
        store(i + 1, exp[i])
        store(i + 2, exp[i + 1])
    if fault == "legitimate_value_into_guard" and n >= 1:
        store(n, exp[n - 1])      # a stray store of a value the result really holds, one cell behind ...
        store(-1, exp[0])         # ... and one cell in front


VALUE_FAULTS = {
    # fault: where it changes what the model stores
    "last_tile_unguarded": lambda n, head: geometry(n, head)[0] % PAIRS != 0 or geometry(n, head)[0] == 0,
    "pr_le_npairs": lambda n, head: geometry(n, head)[0] % PAIRS != 0 or geometry(n, head)[0] == 0,
    "tail_at_n": lambda n, head: (n - head) & 1 == 1,
    "head_at_minus_1": lambda n, head: head == 1,
    "head_never_stored": lambda n, head: head == 1,
    "tail_never_stored": lambda n, head: (n - head) & 1 == 1,
    "middle_tile_skipped": lambda n, head: geometry(n, head)[1] >= 3,
    "front_tiles_swapped": lambda n, head: geometry(n, head)[1] >= 2,
    "group_twice_shifted_8": lambda n, head: geometry(n, head)[0] >= 1,
    "legitimate_value_into_guard": lambda n, head: True,
}
# the fewest (n, head) of the list at which a fault must have an effect (counted from the predicates above; the tile faults need
# two or three tiles, which the sizes around 2 T and 3 T give)
MIN_EFFECT = {"middle_tile_skipped": 5, "front_tiles_swapped": 15}


def _value_arena(n, head, seed):
    exp = expected_cells(n)
    a = Arena(8 * n, GUARD, offset=8 * head, seed=seed).expect(exp)   # a peeled head puts the pair stores at 8 mod 16
    return a, exp


def test_the_fault_free_model_passes():
    for k, (n, head) in enumerate(CASES):
        a, exp = _value_arena(n, head, k)
        if n:
            run_values(a, exp, n, head)
        a.check(exp, (n, head))
    for n in SIZES:
        m = Arena(n, GUARD, offset=n % 16, seed=n)
        want = expected_mask(n)
        m.expect(want)
        if n:
            run_mask(m, want, n)
        m.check(want, n)


@pytest.mark.parametrize("fault", sorted(VALUE_FAULTS))
def test_every_value_fault_is_caught(fault):
    effect = 0
    for k, (n, head) in enumerate(CASES):
        if n == 0:
            continue
        a, exp = _value_arena(n, head, k)
        run_values(a, exp, n, head, fault)
        if VALUE_FAULTS[fault](n, head):
            effect += 1
            with pytest.raises(AssertionError):
                a.check(exp, (fault, n, head))
        else:
            a.check(exp, (fault, n, head))   # nothing for the fault to change here: the model is the correct kernel
    assert effect >= MIN_EFFECT.get(fault, len(CASES) // 2 - 2), (fault, effect, len(CASES))


# ---------------------------------------------------------------- the model: the mask stream
def expected_mask(n, seed=2):
    return np.random.default_rng(seed).integers(0, 2, size=n, dtype=np.uint8)


def run_mask(arena, exp, n, fault=None):
    mem, lo = arena.mem, arena.lo
    ngroups = n // 16
    mem[lo:lo + 16 * ngroups] = exp[:16 * ngroups]
    if fault != "mask_remainder_not_stored":
        mem[lo + 16 * ngroups:lo + n] = exp[16 * ngroups:]


def test_the_unwritten_mask_remainder_is_caught():
    """[n / 16 * 16, n) left as it was: caught whatever the mask holds, because the payload started as its complement."""
    effect = 0
    for n in SIZES[1:]:
        for want in (expected_mask(n), np.zeros(n, np.uint8), np.ones(n, np.uint8)):
            m = Arena(n, GUARD, offset=3, seed=n).expect(want)
            run_mask(m, want, n, "mask_remainder_not_stored")
            if n % 16:
                effect += 1
                with pytest.raises(AssertionError):
                    m.check(want, n)
            else:
                m.check(want, n)
    assert effect >= 3 * (len(SIZES) - 6)


# ---------------------------------------------------------------- what check reports
def _message(fault, n, head):
    a, exp = _value_arena(n, head, 5)
    run_values(a, exp, n, head, fault)
    with pytest.raises(AssertionError) as e:
        a.check(exp, "probe")
    return str(e.value)


def test_check_reports_the_position_relative_to_the_payload():
    # (a stored byte equals the guard's random byte once in 256: the first difference lies within the stray cell's 8 bytes)
    assert re.search(r"first at byte -[1-8]: ", _message("head_at_minus_1", 2 * T + 1, 1))
    assert re.search(r"first at byte n \+ [0-7]: ", _message("last_tile_unguarded", 3 * T + 8, 0))
    assert re.search(r"first at byte -[1-8]: ", _message("legitimate_value_into_guard", 17, 0))
    msg = _message("head_never_stored", T + 2, 1)
    assert "first at cell 0 " in msg and "never written" in msg
    assert f"first at cell {T} " in _message("tail_never_stored", T + 1, 0)
    assert f"first at cell {2 * T} " in _message("middle_tile_skipped", 3 * T + 7, 0)   # four tiles: the third is left out
    # a tail cell stored one cell on leaves cell n - 1 unwritten as well: the first difference is that cell, the last lies behind n
    msg = _message("tail_at_n", T + 1, 0)
    assert f"first at cell {T} " in msg and int(re.search(r"last at byte (\d+)", msg).group(1)) >= 8 * (T + 1)


def test_a_result_of_another_length_is_refused():
    a = Arena(80, GUARD).expect(expected_cells(10))
    run_values(a, expected_cells(10), 10, 0)
    with pytest.raises(AssertionError):
        a.check(expected_cells(9))
    with pytest.raises(AssertionError):
        a.check(expected_cells(11))
    a.check(expected_cells(10))


def test_an_operand_arena_sees_one_changed_byte():
    cells = expected_cells(100)
    for at in (0, GUARD - 1, GUARD + 8, GUARD + 8 + 799, GUARD + 8 + 800, 2 * GUARD + 8 + 799):
        a = Arena(800, GUARD, offset=8, seed=3).hold(cells)
        a.check_unchanged()
        a.mem[at] ^= 0x10
        with pytest.raises(AssertionError):
            a.check_unchanged()


def test_guards_are_seeded_noise_and_the_payload_sits_where_it_was_asked_to():
    a, b = Arena(64, GUARD, offset=5, seed=1), Arena(64, GUARD, offset=5, seed=1)
    assert np.array_equal(a.before, b.before) and not np.array_equal(a.before, Arena(64, GUARD, offset=5, seed=2).before)
    assert len(set(a.before[:GUARD].tolist())) > 200          # not a constant
    for off in (0, 1, 3, 8, 15, 24):
        a = Arena(64, GUARD, offset=off, seed=off)
        assert a.ptr % 256 == off and a.lo >= GUARD and a.total - a.lo - a.nbytes == GUARD
        assert a.mem.ctypes.data + a.lo == a.ptr
