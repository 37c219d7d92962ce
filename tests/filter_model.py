"""A numpy restatement of the Chebyshev filter on the stored states, for tests/test_filter_host.py (CPU: the coefficients bit for bit,
the solver against a dense eigh of H) and tests/test_gpu_filter.py (GPU: the cells of wafer_k_batch_store_filter and
wafer_k_filter_step bit for bit, the spectral bound, the device's solve_filtered).  Nothing here loads the engine's library; only solve_filtered
reaches for the package, for filtered_solve_loop, which is plain Python.

The coefficients, in this order, every operation a float64 operation of its own:
    e = (b - a) / 2    cc = (b + a) / 2    sigma = e / (a0 - cc)    gamma = 2 / sigma
    step 1:      al = sigma / e,  be = 0
    step i >= 2: s2 = 1 / (gamma - sigma)    al = (2 s2) / e    be = sigma s2    sigma = s2
One step per work cell c of the padded array cur, with S = the bracketed sum of cur at c (stencil_sum of tests/fp32_reference.py,
frame cells read as they are stored), one numpy elementwise operation per operation of the kernel:
    w = cur[c]    q = S / den    hw = V[c] * w - q    t = hw - cc * w    y = al * t    not first: y = y - be * prev[c]
rounded once to the storage type.  Step 1 writes into an array of zeros; step i >= 2 writes the work cells of the iterate before
last, whose other cells stay: an even degree keeps the start's frame, an odd one ends on a zero frame."""
import numpy as np

from tests import residual_model as res
from tests import ritz_model as rm
from tests.fp32_reference import denominator, stencil_sum

ABS_WEIGHT = {1: 12.0, 2: 192.0, 3: 3264.0}   # the sum of the absolute weights of stencil_sum, centre included
K, GUARD, DEGREE, TOLERANCE, MAX_BLOCKS = 5, 1, 30, 1e-10, 40
SEED = 20
WAFER_OK, WAFER_ERR_STATE = 0, -4   # include/wafer_hip.h


class Cfg:
    """what the models read"""

    def __init__(self, ext, dn, mass=1.0):
        self.ext, self.dn, self.mass = ext, dn, mass


def coefficients(degree, a, b, a0):
    """(al[degree], be[degree], cc)"""
    a, b, a0 = np.float64(a), np.float64(b), np.float64(a0)
    e = (b - a) / np.float64(2.0)
    cc = (b + a) / np.float64(2.0)
    sigma = e / (a0 - cc)
    gamma = np.float64(2.0) / sigma
    al, be = [sigma / e], [np.float64(0.0)]
    for _ in range(1, degree):
        s2 = np.float64(1.0) / (gamma - sigma)
        al.append((np.float64(2.0) * s2) / e)
        be.append(sigma * s2)
        sigma = s2
    return np.array(al), np.array(be), float(cc)


def _work(p, e):
    return p[e:-e, e:-e, e:-e]


def step(cfg, v, cur, prev, al, be, cc, first, storage=np.float64):
    """the array one step writes: the padded float64 array whose work cells hold y rounded to `storage` and whose other cells are
    zeros (first) or prev's"""
    e = cfg.ext
    w = _work(cur, e)
    q = stencil_sum(cur, e) / denominator(cfg)
    hw = _work(v, e) * w - q
    t = hw - cc * w
    y = al * t
    out = np.zeros_like(cur) if first else prev.copy()
    if not first:
        y = y - be * _work(prev, e)
    with np.errstate(over="ignore"):
        _work(out, e)[...] = y.astype(storage).astype(np.float64)
    return out


def filter(cfg, v, state, degree, a, b, a0, storage=np.float64):
    """the state after `degree` steps, rounded to `storage` between the steps"""
    al, be, cc = coefficients(degree, a, b, a0)
    prev, cur = None, state
    for i in range(degree):
        prev, cur = cur, step(cfg, v, cur, prev, al[i], be[i], cc, i == 0, storage)
    return cur


def bound(cfg, v):
    """Gershgorin: no eigenvalue of H lies above it"""
    return ABS_WEIGHT[cfg.ext] / denominator(cfg) + float(np.max(_work(v, cfg.ext)))


def apply_h(cfg, v, l):
    """H l over the work area"""
    e = cfg.ext
    return _work(v, e) * _work(l, e) - stencil_sum(l, e) / denominator(cfg)


def dense_h(cfg, v, shape):
    """H assembled cell by cell: column c is H applied to the unit vector of work cell c inside a zero frame"""
    e, n = cfg.ext, int(np.prod(shape))
    H = np.zeros((n, n))
    l = np.zeros(tuple(s + 2 * e for s in shape))
    work = _work(l, e)
    for c, idx in enumerate(np.ndindex(*shape)):
        work[idx] = 1.0
        H[:, c] = apply_h(cfg, v, l).ravel()
        work[idx] = 0.0
    return H


def harmonic_v(shape, ext, dn, strength=200.0):
    """the padded V = strength r^2 with r = dn * (distance from the box's centre in cells), zero on the frame"""
    ax = [(np.arange(n) - (n - 1) / 2.0) * dn for n in shape]
    r2 = ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2
    v = np.zeros(tuple(n + 2 * ext for n in shape))
    _work(v, ext)[...] = strength * r2
    return v


def start_states(shape, ext, k=K, seed=SEED):
    """k padded N(0, 1) arrays on the work cells inside a zero frame"""
    return rm.random_states(shape, ext, k, seed, frame=False)


class Member:
    """one problem of the numpy backend: the padded V and the k padded states"""

    def __init__(self, cfg, v, states):
        self.cfg = cfg
        self.v = np.ascontiguousarray(v, dtype=np.float64)
        self.states = [np.ascontiguousarray(s, dtype=np.float64).copy() for s in states]

    def filter(self, degree, a, b, a0):
        self.states = [filter(self.cfg, self.v, s, degree, a, b, a0) for s in self.states]

    def ritz(self):
        """-> (status, evals); on WAFER_OK the states are rotated"""
        h, s = rm.matrices(self.cfg, self.v, self.states)
        A, B = 0.5 * (h + h.T), 0.5 * (s + s.T)
        if not (np.all(np.isfinite(A)) and np.all(np.isfinite(B))):
            return WAFER_ERR_STATE, None
        try:
            L = np.linalg.cholesky(B)
        except np.linalg.LinAlgError:
            return WAFER_ERR_STATE, None
        Li = np.linalg.inv(L)
        At = Li @ A @ Li.T
        evals, Q = np.linalg.eigh(0.5 * (At + At.T))
        coef = Li.T @ Q   # coef[j, a]: the component of input state j in output state a
        if not np.all(np.isfinite(coef)):
            return WAFER_ERR_STATE, None
        self.states = rm.rotate(self.states, coef)
        return WAFER_OK, evals

    def rho(self, theta):
        out = []
        for l, t in zip(self.states, theta):
            r2, _, s = res.sums(self.cfg, self.v, l, float(t))
            out.append(np.sqrt(r2 / s))
        return np.array(out)


def solve_filtered(members, k=K, tolerance=TOLERANCE, degree=DEGREE, max_blocks=MAX_BLOCKS, guard=GUARD):
    """filtered_solve_loop over the numpy members: per member the loop's dict"""
    from wafer_amd.engine import filtered_solve_loop

    def filt(going, n, iv):
        for m in going:
            members[m].filter(n, *iv[m])

    return filtered_solve_loop(lambda going: {m: bound(members[m].cfg, members[m].v) for m in going}, filt,
                               lambda going: {m: members[m].ritz() for m in going},
                               lambda going, theta: {m: members[m].rho(theta[m]) for m in going},
                               [k] * len(members), tolerance, degree, max_blocks, guard)
