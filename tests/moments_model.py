"""A numpy fp64 restatement of the moment matrices of the stored states (wafer_k_moment_sums, wafer_amd/csrc/wafer_moments.hip.h),
for tests/test_moments_host.py (CPU: held to the oracle's observables) and the GPU tests.

Per work cell c with 0-based work indices (ix, iy, iz) of a grid nx x ny x nz, w = l_j[c], l = l_i[c]:
    dx = ix - (nx + 1.) / 2.    dy, dz likewise    r2c = dx * dx + dy * dy + dz * dz        p = l * w
    S += p    X += p * dx    Y += p * dy    Z += p * dz    R2 += p * r2c
one numpy elementwise operation per operation of the kernel, then np.sum (another order than the device's: sums of rounded terms
are compared to a tolerance scaled by sum |term|, which matrices() returns too; sums of integers are exact in any order).  The
origin (n + 1) / 2 is compute_observables' own, one cell above the geometric centre (n - 1) / 2.  Nothing here imports the engine."""
import numpy as np

NAMES = ("s", "x", "y", "z", "r2")


def _work(p, e):
    return p[e:-e, e:-e, e:-e]


def centres(shape):
    """the kernel's origin, per axis: ((double)n + 1.) / 2."""
    return tuple((float(n) + 1.) / 2. for n in shape)


def offsets(shape, origin=None):
    """dx, dy, dz broadcast over the work shape [x][y][z], and r2c = dx * dx + dy * dy + dz * dz in that association"""
    cx, cy, cz = centres(shape) if origin is None else origin
    dx = (np.arange(shape[0], dtype=np.float64) - cx)[:, None, None] + np.zeros(shape)
    dy = (np.arange(shape[1], dtype=np.float64) - cy)[None, :, None] + np.zeros(shape)
    dz = (np.arange(shape[2], dtype=np.float64) - cz)[None, None, :] + np.zeros(shape)
    r2c = dx * dx + dy * dy + dz * dz
    return dx, dy, dz, r2c


def terms(shape, ext, lj, li, origin=None):
    """the five per-cell terms of entry (j, i): arrays of the work shape, in NAMES' order"""
    dx, dy, dz, r2c = offsets(shape, origin)
    w, l = _work(lj, ext), _work(li, ext)
    p = l * w
    return p, p * dx, p * dy, p * dz, p * r2c


def matrices(shape, ext, states, scales=False, origin=None):
    """{"s", "x", "y", "z", "r2"}: (k, k) each, [j, i] = the sum over the work cells of terms(l_j, l_i) -- computed for i <= j and
    mirrored, as the engine does.  scales=True: (matrices, sums of |terms|) -- what a tolerance on a sum of rounded terms is
    relative to.  origin: other centres than the kernel's (to tell conventions apart)."""
    k = len(states)
    m = {n: np.zeros((k, k)) for n in NAMES}
    a = {n: np.zeros((k, k)) for n in NAMES}
    for j in range(k):
        for i in range(j + 1):
            for n, t in zip(NAMES, terms(shape, ext, states[j], states[i], origin)):
                m[n][j, i] = m[n][i, j] = np.sum(t)
                a[n][j, i] = a[n][i, j] = np.sum(np.abs(t))
    return (m, a) if scales else m


def integer_states(shape, ext, k, seed, storage=np.float64):
    """k padded arrays of integers in -3 .. 3, frame included: every product and every sum of the five matrices is exact in fp64"""
    rng = np.random.default_rng(seed)
    padded = tuple(n + 2 * ext for n in shape)
    return [np.ascontiguousarray(rng.integers(-3, 4, padded).astype(storage).astype(np.float64)) for _ in range(k)]
