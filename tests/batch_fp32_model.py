"""What tests/test_batch_fp32_host.py (CPU) and tests/test_gpu_batch_fp32.py (GPU) share: the member table of the float-storage
batches, their inputs, and a chain model of one excited-state step on a storage type.  Nothing here imports the engine.

The chain of one step with `lowers` stored states (grid.rs:674-681, wafer_gs_batch.hip.h), every operation in fp64 on values of
the storage type:

    phi  <- fp32_reference.step(phi)                   rounded to storage      (the fp64-arithmetic step: both float dtypes)
    n2   =  sum phi^2
    phi  <- phi / sqrt(n2)                             rounded to storage
    s_l  =  sum lower_l * phi;  phi <- phi - lower_l * s_l     rounded to storage, l = 0, 1, ... in storage order

With storage = float64 this is the oracle's excited-state evolve (pinned to it by the CPU file to 1e-13 per cell).  Every scalar
(n2, s_l) passes through `scalar(value)`: the identity for the model proper, a relative perturbation of +-1e-12 (the project's bar
for sums) for the run that measures how far a differently partitioned sum can move a float result."""
import numpy as np

from tests import fp32_reference as ref

SIG = 0.3
# three members with distinct dn, dt, mass (dt <= dn^2 / 3) and the bit-comparable potentials of fp32_reference.POTENTIALS
MEMBERS = [
    dict(dn=0.2, dt=0.004, mass=1.3, potential=ref.POTENTIALS[0]),
    dict(dn=0.25, dt=0.006, mass=1.0, potential=ref.POTENTIALS[1]),
    dict(dn=0.15, dt=0.002, mass=0.8, potential=ref.POTENTIALS[2]),
]
SHAPES = [(65, 33, 20), (17, 17, 17), (3, 2, 5), (1, 1, 1)]        # of fp32_reference.SHAPES
assert all(s in ref.SHAPES for s in SHAPES)
STEP_COUNTS = ref.STEP_COUNTS                                       # cumulative: [1, 2, 3, 7, 8, 12]
VARIANT_SHAPES = [(65, 33, 20), (50, 50, 50)]                       # one step per launch against fused passes
VARIANT_STEPS = (1, 2, 3, 5, 8)
EXCITED_SHAPES = [(33, 20, 11), (65, 33, 20)]
REL_SUM = 1e-12                                                     # every global sum


def member_inputs(wo, k, shape, ext, seed=0):
    """(cfg, stored V, start) of member k on `shape`: the oracle's V and a N(0, 1) work area inside a zero frame, both rounded
    to float (fp32_reference.case_inputs with the member's own dn, dt, mass and potential)"""
    m = MEMBERS[k]
    pot = "Coulomb" if m["potential"] == "Cube" and min(shape) < 4 else m["potential"]   # (fp32_reference.potential_of)
    cfg = wo.Config(*shape, ext=ext, potential=pot, dn=m["dn"], dt=m["dt"], mass=m["mass"], sig=SIG)
    phi = np.zeros(cfg.padded_shape)
    rng = np.random.default_rng([seed, k, ext, *shape])
    phi[ext:-ext, ext:-ext, ext:-ext] = rng.standard_normal(cfg.work_shape)
    return cfg, ref.r32(wo.potential_generate(cfg)), ref.r32(phi)


def stored_states(cfg, k, wnum, storage=np.float32):
    """wnum normalised random states of the storage type (not orthogonal to each other: the chain must not rely on it)"""
    e, out = cfg.ext, []
    for i in range(wnum):
        rng = np.random.default_rng([77, k, i, e, cfg.nx, cfg.ny, cfg.nz])
        l = np.zeros(cfg.padded_shape)
        l[e:-e, e:-e, e:-e] = rng.standard_normal(cfg.work_shape)
        out.append(np.ascontiguousarray((l / np.sqrt(np.sum(l * l))).astype(storage).astype(np.float64)))
    return out


def exact(x):
    return x


class Perturbed:
    """scalar -> scalar * (1 +- 1e-12), the signs from a fixed sequence"""

    def __init__(self, seed=0, rel=REL_SUM):
        self.rng, self.rel = np.random.default_rng(seed), rel

    def __call__(self, x):
        return x * (1.0 + (self.rel if self.rng.integers(2) else -self.rel))


def _store(x, storage):
    return np.ascontiguousarray(x.astype(storage).astype(np.float64))


def orthogonalise(phi, lowers, storage, scalar=exact):
    """modified Gram-Schmidt in storage order (grid.rs:477-492), phi rounded to storage after each projection"""
    for l in lowers:
        s = scalar(float(np.sum(l * phi)))
        phi = _store(phi - l * s, storage)
    return phi


def excited_steps(cfg, v_stored, phi, lowers, steps, storage, scalar=exact, ab="registers"):
    """`steps` steps of the chain above from `phi`; a new array.  ab: fp32_reference.ab_of's source ("stored": the arrays the
    direct kernel, variant 0, streams)"""
    a, b = ref.ab_of(v_stored, cfg.dt, np.float64, ab)
    den = ref.denominator(cfg)
    for _ in range(steps):
        phi = ref.step(phi, a, b, cfg.dt, den, cfg.ext, np.float64, storage)
        n2 = scalar(float(np.sum(phi * phi)))
        phi = _store(phi / np.sqrt(n2), storage)
        phi = orthogonalise(phi, lowers, storage, scalar)
    return phi


def spacing_u(phi):
    """u: the spacing of floats at max |phi|"""
    return float(np.spacing(np.float32(np.max(np.abs(phi)))))


def work(cfg, x):
    e = cfg.ext
    return x[e:-e, e:-e, e:-e]
