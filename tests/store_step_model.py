"""A numpy backend for wafer_amd.engine.block_solve_loop, for tests/test_store_step_host.py (CPU) and tests/test_gpu_store_step.py
(GPU: the device's solve_block is held to it).  Per member: the oracle's plain step on every state of the block, tests/ritz_model.py
for the Ritz step (sums and rotation; the generalised eigenproblem by numpy's Cholesky and eigh) and tests/residual_model.py for rho.
Nothing here loads the engine's library: block_solve_loop is plain Python.

The cases of the issue, on 9^3 with dt = 0.9 dn^2 / 3, ThreePoint, k = 4, N(0, 1) starts inside a zero frame:
  (a) NoPotential: the levels are (1 / (2 m dn^2)) sum_d (2 - 2 cos(pi n_d / 10)) for (1,1,1) and three times (2,1,1);
  (b) V = 200 r^2, r measured from the box's centre in units of dn."""
import numpy as np

from tests import residual_model as res
from tests import ritz_model as rm
from wafer_amd.engine import WAFER_ERR_STATE, WAFER_OK, block_solve_loop

SHAPE, K, STEPS_PER_BLOCK, TOLERANCE, MAX_BLOCKS = (9, 9, 9), 4, 50, 1e-10, 40
SEED = 20


def dt_of(dn):
    return 0.9 * dn * dn / 3.0


def box_levels(dn, mass=1.0, shape=SHAPE):
    """the four lowest levels of the discrete ThreePoint H with V = 0 in a zero frame: (1,1,1), then (2,1,1) three times"""
    def level(p):
        return sum(2.0 - 2.0 * np.cos(np.pi * pa / (n + 1.0)) for pa, n in zip(p, shape)) / (2.0 * mass * dn * dn)
    return np.array([level((1, 1, 1)), level((2, 1, 1)), level((1, 2, 1)), level((1, 1, 2))])


def harmonic_v(shape, ext, dn, strength=200.0):
    """the padded V = strength r^2 with r = dn * (distance from the box's centre in cells), zero on the frame"""
    ax = [(np.arange(n) - (n - 1) / 2.0) * dn for n in shape]
    r2 = ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2
    v = np.zeros(tuple(n + 2 * ext for n in shape))
    v[ext:-ext, ext:-ext, ext:-ext] = strength * r2
    return v


def start_states(shape=SHAPE, ext=1, k=K, seed=SEED):
    """k padded N(0, 1) arrays on the work cells inside a zero frame"""
    return rm.random_states(shape, ext, k, seed, frame=False)


class Member:
    """one problem of the numpy backend: the oracle's Config, the padded V with its a, b, and the k padded states"""

    def __init__(self, oracle, shape, dn, v, states, ext=1, mass=1.0):
        self.wo = oracle
        self.cfg = oracle.Config(shape[0], shape[1], shape[2], ext=ext, potential="NoPotential", dn=dn, dt=dt_of(dn), mass=mass)
        self.v = np.ascontiguousarray(v, dtype=np.float64)
        self.a, self.b = oracle.ab(self.cfg, self.v)
        self.states = [np.ascontiguousarray(s, dtype=np.float64).copy() for s in states]

    def step(self, n):
        for s in self.states:
            self.wo.evolve(self.cfg, 0, self.a, self.b, s, [], int(n))

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


def solve_block(members, k=K, tolerance=TOLERANCE, steps_per_block=STEPS_PER_BLOCK, max_blocks=MAX_BLOCKS):
    """block_solve_loop over the numpy members: per member the loop's dict"""
    def step(going, n):
        for m in going:
            members[m].step(n)

    def ritz(going):
        return {m: members[m].ritz() for m in going}

    def residuals(going, theta):
        return {m: members[m].rho(theta[m]) for m in going}

    return block_solve_loop(step, ritz, residuals, [k] * len(members), tolerance, steps_per_block, max_blocks)
