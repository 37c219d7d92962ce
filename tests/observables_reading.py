"""A second reading of compute_observables (grid.rs:303-445) in numpy, for tests/test_observables_reading.py (CPU: held to the
oracle's per-cell terms bit for bit) and tests/test_gpu_observables_exact.py (GPU: the sums on integer-valued data, with ==).

cells() writes the four per-cell terms, one numpy elementwise operation per operation of the Rust source and in the source's
association; numpy's float64 elementwise operations are the IEEE operations (no extended precision, no contraction).  The
bracketed sum S is stencil_sum of tests/fp32_reference.py, which tests/test_fp32_reference.py already holds to the oracle's
step bit for bit.  Nothing here imports the oracle or the engine.

integer_case() builds inputs on which every term is a multiple of 1/4 and every partial sum of every quantity stays below 2^53
quarters, so that any summation order gives the exact sum and == replaces a tolerance at any shape."""
import math

import numpy as np

from tests.fp32_reference import denominator, stencil_sum

QUANTITIES = ("energy", "norm2", "v_infinity", "r2")


def _work(p, e):
    return p[e:-e, e:-e, e:-e]


def r2_of(shape):
    """potential::calculate_r2 (potential.rs:366-371) of every WORK-area index (grid.rs:428-437 passes the index into the work
    view, not the padded one): d = idx - (n + 1) / 2, then dx*dx + dy*dy + dz*dz from left to right"""
    d = [np.arange(n, dtype=np.float64) - (np.float64(n) + 1.) / 2. for n in shape]
    dx, dy, dz = d[0][:, None, None], d[1][None, :, None], d[2][None, None, :]
    return dx * dx + dy * dy + dz * dz


def cells(cfg, v, phi, potsub=(0, 0.0, None)):
    """the four per-cell terms over the work area.  cfg: anything with ext, dn, mass (the oracle's Config, a Case); v, phi:
    padded float64 arrays; potsub: (kind, scalar, array of the work shape) -- 0 none, 1 scalar, 2 array.  v_infinity is the
    float 0.0 without a pot_sub (grid.rs:425), not an array."""
    e = cfg.ext
    assert v.dtype == np.float64 and phi.dtype == np.float64 and v.shape == phi.shape
    kind, scalar, arr = potsub
    w, vv = _work(phi, e), _work(v, e)
    S = stencil_sum(phi, e)                    # grid.rs:326-331 / 350-362 / 382-399
    den = denominator(cfg)                     # grid.rs:314 / 337 / 367: lead * dn * dn * mass, from left to right
    energy = (vv * w) * w - (w * S) / den      # grid.rs:325-332 / 349-362 / 381-399: v*w*w - w*S/denominator
    norm2 = w * w                              # grid.rs:407
    if kind == 2:
        v_infinity = (w * w) * arr             # grid.rs:410-418: w*w*pot_sub[i], the unpadded array
    elif kind == 1:
        v_infinity = (w * w) * np.float64(scalar)   # grid.rs:419-424
    else:
        assert kind == 0
        v_infinity = 0.0                       # grid.rs:425
    r2 = (w * w) * r2_of(w.shape)              # grid.rs:428-437
    return dict(energy=energy, norm2=norm2, v_infinity=v_infinity, r2=r2)


def exact_sums(c):
    """the correctly rounded sum of every quantity's terms (math.fsum): on integer_case's data, the exact sum"""
    return {k: math.fsum(np.ravel(c[k]).tolist()) if isinstance(c[k], np.ndarray) else float(c[k]) for k in QUANTITIES}


class Case:
    """the inputs of integer_case: shape, ext, dn, mass (cfg-like: cells() and denominator() take it), padded phi and v,
    the work-shaped pot_sub array and the scalar pot_sub"""

    def __init__(self, shape, ext, dn, mass, phi, v, potsub, potsub_scalar):
        self.shape, self.ext, self.dn, self.mass = tuple(shape), ext, dn, mass
        self.nx, self.ny, self.nz = self.shape
        self.phi, self.v, self.potsub, self.potsub_scalar = phi, v, potsub, potsub_scalar

    def potsub_form(self, form):
        """(kind, scalar, array) as set_potential_host and the oracle take them; form: "none" / "scalar" / "array" """
        return {"none": (0, 0.0, None), "scalar": (1, self.potsub_scalar, None), "array": (2, 0.0, self.potsub)}[form]

    def cells(self, form):
        return cells(self, self.v, self.phi, self.potsub_form(form))

    def sums(self, form):
        return exact_sums(self.cells(form))


POTSUB_FORMS = ("none", "scalar", "array")


def integer_case(shape, ext, seed, storage="f64"):
    """Inputs on which all four sums are exact in fp64 in any order.  dn = 0.5 and mass = 2 / 0.5 / 0.5 make the denominator
    1 / 3 / 45 for ThreePoint / FivePoint / SevenPoint; phi = q k with q = 1 / 3 / 45 = den and integer k in [-8, 8], so that
    w S is an integer multiple of q^2 and (w S) / den an integer; V is an integer in [-4, 4] (frame included), the pot_sub array
    an integer in [-5, 5], the scalar pot_sub 0.75; dx, dy, dz are half-integers, so r2 is a multiple of 1/4.  storage: "f64" or
    "f32" -- the values are the same and a float holds each of them exactly (asserted), so an engine of either storage type
    sees these numbers.  Asserts its own preconditions: den, terms in quarters, sum |term| < 2^51 per quantity."""
    assert storage in ("f64", "f32"), storage
    q = {1: 1.0, 2: 3.0, 3: 45.0}[ext]
    dn, mass = 0.5, {1: 2.0, 2: 0.5, 3: 0.5}[ext]
    rng = np.random.default_rng(seed)
    padded = tuple(n + 2 * ext for n in shape)
    phi = np.zeros(padded)
    _work(phi, ext)[...] = q * rng.integers(-8, 9, size=shape)
    v = rng.integers(-4, 5, size=padded).astype(np.float64)
    potsub = rng.integers(-5, 6, size=shape).astype(np.float64)
    case = Case(shape, ext, dn, mass, phi, v, potsub, 0.75)
    for a in (phi, v, potsub):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    assert np.float32(case.potsub_scalar) == case.potsub_scalar
    assert denominator(case) == q
    for form in POTSUB_FORMS:
        for k, t in case.cells(form).items():
            t = np.asarray(t, dtype=np.float64)
            assert np.array_equal(np.floor(t * 4.0), t * 4.0), (k, form)          # a multiple of 1/4 (t * 4 is exact)
            # then every partial sum, in any order and grouping, is a multiple of 1/4 below 2^51: a double holds it exactly
            assert math.fsum(np.abs(t).ravel().tolist()) < 2.0 ** 51, (k, form)
    return case
