"""Guarded arenas: where a kernel's output lands, and what it must leave alone.

The header promises that an element-wise entry point writes exactly `n` cells at the caller's output pointer and nothing
else, wherever that pointer sits, and that it never writes an operand.  An `Arena` holds one such block so that a test can see
every way of breaking that promise:

    low guard | payload | high guard

  * the guards (32 KiB each by default: more than the largest tile any of these kernels stores — k_map's 256 lanes x map_u 4
    x 16 B = 16 KiB, k_expr's 1536 cells x 8 B = 12 KiB) hold seeded random bytes, so a stray store of any value, a plausible
    result among them, differs from what was there;
  * the payload of an OUTPUT is pre-filled with the bitwise complement of the expected result (`expect`): every byte the
    kernel fails to write differs from the oracle's, whatever the cell type and whatever the oracle's value — no poison value
    that a result might happen to equal;
  * the payload of an OPERAND holds the operand (`hold`), and `check_unchanged` compares the whole arena byte for byte;
  * the payload starts `offset` bytes behind a 256-byte-aligned address, so the test chooses its residue mod 16.

`check(expected)` reads the whole arena back once and names the first differing byte by its position relative to the payload:
`-k` (k bytes in front of it), `n + k` (k bytes behind its n bytes), or the cell it belongs to.

The memory is the device's (`ec` given: a block of the library's pool, uploaded and downloaded through the C ABI) or the host's
(a numpy array: the host-to-host entry points, and tests/test_arena_faults.py, which models kernels in numpy).  Plain numpy plus
that thin glue; imports nothing from the library itself.
"""
import ctypes as C

import numpy as np

GUARD = 32768
ALIGN = 256
_NOISE = np.random.default_rng(0xA7E7A5EED).integers(0, 256, size=(1 << 20) + 4099, dtype=np.uint8)


def noise(nbytes: int, seed: int) -> np.ndarray:
    """`nbytes` seeded random bytes (a fresh copy)."""
    if nbytes <= _NOISE.size // 2:
        at = (seed * 7919 + 13) % (_NOISE.size - nbytes)
        return _NOISE[at:at + nbytes].copy()
    return np.random.default_rng(seed).integers(0, 256, size=nbytes, dtype=np.uint8)


def as_bytes(a) -> np.ndarray:
    """The bytes of an array (or of a ctypes structure), as a flat uint8 array."""
    if isinstance(a, np.ndarray):
        return np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return np.frombuffer(bytes(a), dtype=np.uint8)


class Arena:
    def __init__(self, nbytes_payload: int, guard: int = GUARD, offset: int = 0, seed: int = 0, ec=None):
        """`offset`: bytes between a 256-byte-aligned address and the payload's first byte.  `ec`: the erased_cells_hip module
        for device memory, None for host memory."""
        assert nbytes_payload >= 0 and guard >= 0 and offset >= 0
        self.nbytes, self.guard, self.offset, self.ec = nbytes_payload, guard, offset, ec
        self.lo = guard - guard % -ALIGN + offset            # the payload's first byte within the image
        self.total = self.lo + nbytes_payload + guard
        self.before = noise(self.total, seed)                # what the arena holds when the kernel starts
        if ec is None:
            self._store = np.empty(self.total + ALIGN, dtype=np.uint8)
            self.base = self._store.ctypes.data - self._store.ctypes.data % -ALIGN
            skip = self.base - self._store.ctypes.data
            self.mem = self._store[skip:skip + self.total]   # the image itself: a numpy model of a kernel writes here
            self.mem[:] = self.before
        else:
            self._store = ec.DeviceMem(self.total + ALIGN)
            self.base = self._store.ptr - self._store.ptr % -ALIGN
            self.mem = None
        assert self.base % ALIGN == 0
        self.ptr = self.base + self.lo                       # what the entry point is given
        self._synced = ec is None

    # ---- what the arena holds before the call
    def hold(self, payload) -> "Arena":
        """The payload as given (an operand, or the left side of an in-place form)."""
        b = as_bytes(payload)
        assert b.size == self.nbytes, f"payload of {b.size} bytes for an arena of {self.nbytes}"
        self.before[self.lo:self.lo + self.nbytes] = b
        self._write()
        return self

    def expect(self, expected) -> "Arena":
        """The payload as the bitwise complement of `expected`: an unwritten byte can never pass."""
        return self.hold(~as_bytes(expected))

    def _write(self):
        if self.ec is None:
            self.mem[:] = self.before
        else:
            self.ec._ffi.check(self.ec.lib().ec_upload(self.base, self.before.ctypes.data_as(C.c_void_p), self.total, self.ec.stream()))
        self._synced = True

    # ---- what it holds afterwards
    def image(self) -> np.ndarray:
        """The whole arena as it is now (one download for device memory, which also waits for the stream)."""
        assert self._synced, "hold() or expect() first: the arena's memory was never written"
        if self.ec is None:
            return self.mem.copy()
        out = np.empty(self.total, dtype=np.uint8)
        self.ec._ffi.check(self.ec.lib().ec_download(out.ctypes.data_as(C.c_void_p), self.base, self.total, self.ec.stream()))
        return out

    def payload(self, dtype) -> np.ndarray:
        return self.image()[self.lo:self.lo + self.nbytes].view(dtype)

    def _compare(self, want: np.ndarray, itemsize: int, what):
        got = self.image()
        bad = np.flatnonzero(got != want)
        if bad.size == 0:
            return
        at = int(bad[0]) - self.lo
        last = int(bad[-1]) - self.lo
        if at < 0:
            where = f"byte {at}: {-at} bytes in front of the payload (guard overwritten)"
        elif at >= self.nbytes:
            where = f"byte n + {at - self.nbytes}: {at - self.nbytes} bytes behind the payload's n = {self.nbytes} bytes (guard overwritten)"
        else:
            where = f"cell {at // itemsize} (byte {at} of the payload's {self.nbytes})"
            if got[bad[0]] == self.before[bad[0]]:
                where += ", still as it was before the call (never written)"
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {where}, last at byte {last}; "
                             f"got {int(got[bad[0]]):#04x}, expected {int(want[bad[0]]):#04x} (payload offset {self.offset} bytes mod {ALIGN})")

    def check(self, expected, what="arena") -> None:
        """Both guards byte-identical to their before-image, the payload bit-identical to `expected` and exactly as long."""
        exp = as_bytes(expected)
        assert exp.size == self.nbytes, f"{what}: expected result of {exp.size} bytes, payload of {self.nbytes}"
        want = self.before.copy()
        want[self.lo:self.lo + self.nbytes] = exp
        self._compare(want, expected.dtype.itemsize if isinstance(expected, np.ndarray) else 1, what)

    def check_unchanged(self, what="operand") -> None:
        """Every byte — guards and payload — as it was before the call."""
        self._compare(self.before, 1, what)


def output(ec, expected: np.ndarray, offset_cells: int = 0, seed: int = 0, guard: int = GUARD) -> Arena:
    """An arena for a result the oracle says is `expected`, its first cell `offset_cells` cells behind a 256-byte boundary,
    pre-filled with the complement."""
    exp = np.ascontiguousarray(expected)
    return Arena(exp.nbytes, guard, offset_cells * exp.dtype.itemsize, seed, ec).expect(exp)


def operand(ec, cells: np.ndarray, offset_cells: int = 0, seed: int = 0, guard: int = GUARD) -> Arena:
    """An operand uploaded at a cell offset inside its own guarded arena; `check_unchanged()` after the sweep."""
    a = np.ascontiguousarray(cells)
    return Arena(a.nbytes, guard, offset_cells * a.dtype.itemsize, seed, ec).hold(a)
