"""A numpy model of the one-pass form of the batched excited step (wafer_batch_set_gs_variant(b, 1); wafer_gs_batch.hip.h) on a
storage type, shared by tests/test_batch_onepass_host.py (CPU) and tests/test_gpu_batch_onepass.py (GPU).  Nothing here imports
the engine.  Every operation is fp64 on values of the storage type:

    phi'  <- fp32_reference.step(phi)                          rounded to storage      (the stencil step's own store)
    n2    =  sum phi'^2,   t_j = sum l_j phi'                  on the un-normalised phi'
    G_ji  =  sum l_j l_i   (i < j)                             once per store
    norm  =  sqrt(n2),     s_j = t_j / norm - sum_{i<j} s_i G_ji
    phi   <- phi' / norm - l_0 s_0 - l_1 s_1 - ...             in storage order, unfused, rounded to storage ONCE

Every scalar (n2, t_j, G_ji) passes through `scalar(value)`: batch_fp32_model's `exact` for the model proper, its `Perturbed` for
the run that measures how far a differently partitioned sum can move a float result.  Orthogonalise alone is the same without the
division (norm = 1)."""
import functools

import numpy as np

from tests import fp32_reference as ref
from tests.batch_fp32_model import Perturbed, exact, member_inputs, stored_states

FLOAT_SHAPES = [(33, 20, 11), (65, 33, 20)]
FLOAT_STEPS = (1, 4)


def _store(x, storage):
    return np.ascontiguousarray(x.astype(storage).astype(np.float64))


def gram(lowers, scalar=exact):
    """G[j][i] = sum l_j l_i for i < j"""
    return [[scalar(float(np.sum(lowers[j] * lowers[i]))) for i in range(j)] for j in range(len(lowers))]


def coefficients(t, norm, G):
    """s_j = t_j / norm - sum_{i<j} s_i G_ji, the subtractions in the order of i (norm None: no division)"""
    s = []
    for j, tj in enumerate(t):
        v = tj if norm is None else tj / norm
        for i in range(j):
            v = v - s[i] * G[j][i]
        s.append(v)
    return s


def apply(phi, lowers, norm, s, storage):
    x = phi if norm is None else phi / norm
    for l, sj in zip(lowers, s):
        x = x - l * sj
    return _store(x, storage)


def orthogonalise(phi, lowers, storage, scalar=exact, G=None):
    G = gram(lowers, scalar) if G is None else G
    t = [scalar(float(np.sum(l * phi))) for l in lowers]
    return apply(phi, lowers, None, coefficients(t, None, G), storage)


def excited_steps(cfg, v_stored, phi, lowers, steps, storage, scalar=exact):
    """`steps` one-pass steps from `phi`; a new array"""
    a, b = ref.ab_of(v_stored, cfg.dt, np.float64, "registers")
    den = ref.denominator(cfg)
    G = gram(lowers, scalar)
    for _ in range(steps):
        phi = ref.step(phi, a, b, cfg.dt, den, cfg.ext, np.float64, storage)
        n2 = scalar(float(np.sum(phi * phi)))
        t = [scalar(float(np.sum(l * phi))) for l in lowers]
        norm = float(np.sqrt(n2))
        phi = apply(phi, lowers, norm, coefficients(t, norm, G), storage)
    return phi


@functools.lru_cache(maxsize=None)
def float_models(wo, k, shape, ext, wnum):
    """member k of batch_fp32_model.MEMBERS on float storage -> (cfg, stored states, {operation: (exact, perturbed)}): per
    operation ("orthogonalise", 1, 4: steps from the member's start) the model with exact scalars and with every scalar moved by
    +-1e-12 relative.  Computed once and shared; the arrays are not to be written."""
    cfg, v, phi = member_inputs(wo, k, shape, ext)
    lowers = stored_states(cfg, k, wnum)
    out = {"orthogonalise": (orthogonalise(phi, lowers, np.float32), orthogonalise(phi, lowers, np.float32, Perturbed(k)))}
    for steps in FLOAT_STEPS:
        out[steps] = (excited_steps(cfg, v, phi, lowers, steps, np.float32),
                      excited_steps(cfg, v, phi, lowers, steps, np.float32, Perturbed(k)))
    return cfg, lowers, out
