"""A numpy fp64 restatement of Rayleigh-Ritz on the stored states, for tests/test_ritz_host.py (CPU: held to the oracle's
observables) and tests/test_gpu_ritz.py (GPU: the sums of wafer_k_ritz_sums, the rotation of wafer_k_rotate_states).

The sums, per work cell c, with w = l_j[c], S = the bracketed sum of l_j at c (stencil_sum of tests/fp32_reference.py, frame
cells read as they are stored) and vv = V[c]:
    h[j, i] = sum_c  (vv * l_i[c]) * w - (l_i[c] * S) / den          s[j, i] = sum_c  l_i[c] * w
one numpy elementwise operation per operation of the kernel, then np.sum (another order than the device's: sums are compared
to a tolerance scaled by sum |term|, which matrices() returns too).  For i == j the h term is the energy integrand of
compute_observables (grid.rs:325-332).  Nothing here imports the engine."""
import numpy as np

from tests.fp32_reference import denominator, stencil_sum


def _work(p, e):
    return p[e:-e, e:-e, e:-e]


def matrices(cfg, v, states, scales=False):
    """(h, s) of the padded float64 arrays `states` under the padded potential v; cfg: anything with ext, dn, mass.
    scales=True: (h, s, sum |h terms|, sum |s terms|) -- what a tolerance on a sum of rounded terms is relative to"""
    e, k = cfg.ext, len(states)
    den = denominator(cfg)
    vv = _work(v, e)
    h, s, ah, as_ = (np.zeros((k, k)) for _ in range(4))
    for j in range(k):
        w = _work(states[j], e)
        S = stencil_sum(states[j], e)
        for i in range(k):
            li = _work(states[i], e)
            th = (vv * li) * w - (li * S) / den
            ts = li * w
            h[j, i], s[j, i] = np.sum(th), np.sum(ts)
            ah[j, i], as_[j, i] = np.sum(np.abs(th)), np.sum(np.abs(ts))
    return (h, s, ah, as_) if scales else (h, s)


def rotate(states, coef, storage=np.float64):
    """l'_a = sum_j coef[j, a] l_j over the whole padded arrays, in the kernel's order -- acc = coef[0, a] * l_0, then
    acc = acc + coef[j, a] * l_j for j = 1 .. k-1 -- rounded once to `storage`; float64 arrays out"""
    k = len(states)
    coef = np.asarray(coef, dtype=np.float64)
    assert coef.shape == (k, k)
    out = []
    for a in range(k):
        acc = coef[0, a] * states[0]
        for j in range(1, k):
            acc = acc + coef[j, a] * states[j]
        out.append(np.ascontiguousarray(acc.astype(storage).astype(np.float64)))
    return out


def random_states(shape, ext, k, seed, frame=True, storage=np.float64):
    """k padded N(0, 1) arrays, random on the frame too unless frame=False (a zero frame), rounded to `storage`"""
    rng = np.random.default_rng(seed)
    padded = tuple(n + 2 * ext for n in shape)
    out = []
    for _ in range(k):
        p = rng.standard_normal(padded)
        if not frame:
            q = np.zeros(padded)
            _work(q, ext)[...] = _work(p, ext)
            p = q
        out.append(np.ascontiguousarray(p.astype(storage).astype(np.float64)))
    return out


# ---- the particle in a box on the ThreePoint stencil: S sin = sum_axes (2 cos(p pi / (n + 1)) - 2) sin ------------------------
def sine_state(shape, ext, p):
    """the normalised product of sin(p_a pi (i_a + 1) / (n_a + 1)) over the work area, inside a zero frame"""
    ax = [np.sin(pa * np.pi * (np.arange(n) + 1.0) / (n + 1.0)) for pa, n in zip(p, shape)]
    w = ax[0][:, None, None] * ax[1][None, :, None] * ax[2][None, None, :]
    w = w / np.sqrt(np.sum(w * w))
    out = np.zeros(tuple(n + 2 * ext for n in shape))
    _work(out, ext)[...] = w
    return out


def sine_level(shape, p, dn, mass):
    """<sin| -S / (2 dn^2 m) |sin> = sum_axes (1 - cos(p pi / (n + 1))) / (dn^2 m)"""
    return sum(1.0 - np.cos(pa * np.pi / (n + 1.0)) for pa, n in zip(p, shape)) / (dn * dn * mass)
