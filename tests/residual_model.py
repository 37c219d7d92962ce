"""A numpy fp64 restatement of the residual r = H l - theta l of a stored state, for tests/test_residual_host.py (CPU: box states
with known levels, the oracle's observables) and tests/test_gpu_residual.py (GPU: the cells of wafer_k_residual_write, the sums of
wafer_k_residual_sums).

Per work cell c of the padded array l, with S = the bracketed sum of l at c (stencil_sum of tests/fp32_reference.py, frame cells
read as they are stored) and vv = V[c], one numpy elementwise operation per operation of the kernel:
    w = l[c]    q = S / den    hw = vv * w - q    r = hw - theta * w
    r2 = sum r * r        wh = sum w * hw        s = sum w * w
The sums go through np.sum (another order than the device's): they are compared to a tolerance scaled by sum |term|, which
sums(scales=True) returns for wh.  Nothing here imports the engine."""
import numpy as np

from tests.fp32_reference import denominator, stencil_sum


def _work(p, e):
    return p[e:-e, e:-e, e:-e]


def _hw(cfg, v, l):
    e = cfg.ext
    w = _work(l, e)
    q = stencil_sum(l, e) / denominator(cfg)
    hw = _work(v, e) * w - q
    return w, hw


def cells(cfg, v, l, theta, storage=np.float64):
    """r over the work area of the padded float64 array l under the padded potential v, rounded once to `storage`; float64 out"""
    w, hw = _hw(cfg, v, l)
    r = hw - theta * w
    return np.ascontiguousarray(r.astype(storage).astype(np.float64))


def sums(cfg, v, l, theta, scales=False):
    """(r2, wh, s); scales=True: (r2, wh, s, sum |w * hw|) -- what a tolerance on wh, a sum of rounded terms of both signs, is
    relative to (the terms of r2 and s are not negative: they are their own scales)"""
    w, hw = _hw(cfg, v, l)
    r = hw - theta * w
    r2, wh, s = float(np.sum(r * r)), float(np.sum(w * hw)), float(np.sum(w * w))
    return (r2, wh, s, float(np.sum(np.abs(w * hw)))) if scales else (r2, wh, s)


def rayleigh(cfg, v, l):
    """(theta, r2, s) of Rayleigh mode: theta = wh / s of a pass with theta = 0, then the sums with that theta"""
    _, wh, s = sums(cfg, v, l, 0.0)
    theta = wh / s
    r2, _, s = sums(cfg, v, l, theta)
    return theta, r2, s
