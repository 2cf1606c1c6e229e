"""The inputs and shapes that the GPU tests of ec_focal / ec_focal_convolve run (tests/test_gpu_focal.py, test_gpu_focal_bounds.py), shared
with tests/test_focal_faults.py, which shows without a GPU that these very inputs expose each modelled mistake of a tiled kernel.

Plain numpy; imports nothing from the library.  TW x TH is the output tile of the kernels (csrc/ec_focal_kernels.hpp;
tests/test_focal_args.py checks that the two files agree).
"""
import numpy as np

TW, TH = 64, 16
RADII = [(0, 0), (1, 1), (2, 1), (1, 3), (7, 7), (7, 0), (0, 7)]   # (rx, ry)
NP_DTYPES = [np.dtype(d) for d in (np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64)]
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
MASK_KINDS = ("all-zero", "all-one", "single-zero", "single-one", "hashed")


def axis_values(r, t):
    """the sizes of one axis at which the tiling can go wrong: below, at and above the radius, the footprint and the tile"""
    return sorted({1, 2, r, r + 1, 2 * r + 1, t - 1, t, t + 1, 2 * t + 1} - {0})


def shapes(rx, ry):
    """(cols, rows): a pairing that covers every value of each axis, not the full product — about a dozen shapes per radius"""
    xs, ys = axis_values(rx, TW), axis_values(ry, TH)
    n = max(len(xs), len(ys))
    out = [(xs[i % len(xs)], ys[(i + 4) % len(ys)]) for i in range(n)]
    out += [(1, 1), (TW, TH), (2 * TW + 1, 2 * TH + 1), (TW + 1, 1), (1, TH + 1)]
    out = sorted(set(out))
    assert {c for c, _ in out} == set(xs) and {r for _, r in out} == set(ys)
    return out


def hashed_u64(n, seed):
    """n 64-bit words of splitmix64(seed + index)"""
    with np.errstate(over="ignore"):
        x = (np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def hashed_bytes(n, seed):
    return hashed_u64((n + 7) // 8, seed).view(np.uint8)[:n].copy()


def raster_cells(ct, cols, rows, seed, raw=False):
    """rows x cols cells of type number ct whose BYTES are a hash of their position.  Floats keep their hashed sign and mantissa and get
    an exponent of -32 .. 31 from their hashed one (finite, and so are all sums of them) unless `raw`; there is a -0.0 among them,
    and every fourth row that is wide enough starts with 1e16, 1.0, -1e16, 1.0: a sum that depends on the order of its additions.
    `raw`: the hashed bits as they are, with NaNs and infinities of both signs planted."""
    dt = NP_DTYPES[ct]
    a = hashed_bytes(cols * rows * dt.itemsize, seed).view(dt).copy()
    if dt.kind == "f":
        if not raw:
            u = a.view(UINT[dt.itemsize])
            mant, ebits = (23, 8) if dt.itemsize == 4 else (52, 11)
            e = (u >> mant) & ((1 << ebits) - 1)
            folded = (e % 64) + ((1 << (ebits - 1)) - 1 - 32)
            keep = ((1 << (8 * dt.itemsize)) - 1) ^ (((1 << ebits) - 1) << mant)
            u[...] = (u & u.dtype.type(keep)) | (folded << mant).astype(u.dtype)
            assert np.isfinite(a).all()
        else:
            a[5::37], a[6::41], a[9::43] = np.nan, np.inf, -np.inf
        a = a.reshape(rows, cols)
        if cols >= 4 and not raw:
            a[::4, :4] = np.array([1e16, 1.0, -1e16, 1.0], dtype=dt)
        if a.size > 3:
            a.reshape(-1)[a.size // 2] = dt.type(-0.0)
    return a.reshape(rows, cols)


def mask_bytes(kind, cols, rows, seed):
    n = cols * rows
    if kind == "all-zero":
        m = np.zeros(n, np.uint8)
    elif kind == "all-one":
        m = np.ones(n, np.uint8)
    elif kind == "single-zero":
        m = np.ones(n, np.uint8)
        m[(seed * 7 + n // 3) % n] = 0
    elif kind == "single-one":
        m = np.zeros(n, np.uint8)
        m[(seed * 5 + n // 2) % n] = 1
    else:
        assert kind == "hashed", kind
        m = (hashed_bytes(n, seed ^ 0x3A5C) & 1).astype(np.uint8)
    return m.reshape(rows, cols)


def weights(rx, ry, seed=0):
    """(2 ry + 1) x (2 rx + 1) doubles of both signs and several magnitudes, none a power of two; their sum is not 0"""
    n = (2 * rx + 1) * (2 * ry + 1)
    h = hashed_u64(n, 0xC0 + seed + 16 * rx + ry)
    w = ((h % np.uint64(2001)).astype(np.float64) - 1000.0) / 317.0 * np.where((h >> np.uint64(40)) & np.uint64(1), 0.125, 3.0)
    w[w == 0.0] = 0.7
    assert w.sum() != 0.0
    return w.reshape(2 * ry + 1, 2 * rx + 1)


SOBEL_X = np.array([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]])   # its weights sum to 0.0: NORMALIZE leaves no valid whole footprint


def order_edge_raster(dt):
    """one row of floats on which the total order, the raw bit patterns and `<` disagree: both zeros side by side, NaNs of both signs,
    negative values, an infinity"""
    return np.array([[0.0, -0.0, 0.0, -1.5, -2.5, np.nan, 1.0, -np.nan, -0.0, 0.0, 3.0, -np.inf]], dtype=dt)


def impulse_positions(cols, rows):
    """the 2 x 2 block of cells around every tile corner and the four raster corners, inside a cols x rows raster"""
    at = {(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)}
    for y in range(0, rows + TH, TH):
        for x in range(0, cols + TW, TW):
            for dy in (-1, 0):
                for dx in (-1, 0):
                    if 0 <= y + dy < rows and 0 <= x + dx < cols:
                        at.add((y + dy, x + dx))
    return sorted(at)
