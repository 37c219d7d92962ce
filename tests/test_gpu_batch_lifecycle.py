"""A batch's lazily made buffer groups, one life each: create a batch, use ONE group (or none), close it -- and last one batch that
uses all of them in sequence, held bit for bit to a second, fresh batch running the same sequence in the same process.

The groups are what wafer_engine_batch.hip and wafer_engine_batch_stores.hip make on first use: the sequential Gram-Schmidt buffers (norm2), the one-pass buffers grown
from them (set_gs_variant(1) and an excited step), the resample scratch and its growth, the Rayleigh-Ritz tables, the residual tables
(on phi, with no ritz call before), the shadows, store_k and the copy table of evolve_states with an odd step count, and the store's
slots shrinking and regrowing (clear_states after three pushes, then one push).  A batch that closes after any one of them must free
what that group made and nothing twice; the last batch shows that the order of first uses changes no bit.

Shapes: those of tests/test_gpu_store_step.py, as one mixed batch with state stores, and (12, 10, 9) three times as a uniform batch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = 0.004
SHAPES = [(12, 10, 9), (65, 6, 5), (5, 4, 20)]
BATCHES = {"mixed": SHAPES, "uniform": [SHAPES[0]] * 3}
POTS = ["Harmonic", "Cube", "Periodic"]


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def make(wa, kind, ext, dtype):
    shapes = BATCHES[kind]
    members = [wa.Params(*s, dn=0.2 + 0.03 * m, dt=DT, mass=1.3 - 0.1 * m, central_difference=ext, dtype=dtype, max_states=4)
               for m, s in enumerate(shapes)]
    mixed = len(set(shapes)) > 1
    return wa.Batch(members, mixed_shapes=mixed, state_stores=mixed)


def start(b, seed):
    b.set_potentials(POTS)
    b.set_initial_conditions(["Gaussian"] * 3, [seed, seed + 1, seed + 2])


def source(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


# ---- one function per lazily made group; each returns what it read back ---------------------------------------------------------
def g_nothing(b):
    return []


def g_norm2(b):
    start(b, 3)
    return [np.array(b.norm2())]


def g_onepass(b):
    start(b, 5)
    b.normalise(b.norm2())
    b.push_state()
    b.set_initial_conditions(["Gaussian"] * 3, [11, 12, 13])
    b.set_gs_variant(1)
    before = b.gs_steps()
    b.evolve(1, wnum=1)
    assert b.gs_steps() == (before[0] + 1, before[1])   # the step took the one-pass form
    return [np.array(b.norm2())]


def g_scratch(b):
    b.resample_phi(source((3, 4, 2), 1))
    b.resample_phi(source((7, 5, 6), 2))   # the scratch grows
    return [b.download_phi(m) for m in range(3)]


def g_ritz(b):
    start(b, 7)
    b.seed_states(2, 21)
    r = b.ritz(k=2)
    return [np.array([x["status"] for x in r])] + [x[key] for x in r if x["status"] == 0 for key in ("evals", "coef", "h", "s")]


def g_residuals_phi(b):
    start(b, 9)
    r = b.residuals(source="phi")
    return [x[key] for x in r if x["status"] == 0 for key in ("theta", "r2", "norm2")]


def g_evolve_states(b):
    start(b, 13)
    b.seed_states(2, 31)
    b.evolve_states(3, k=2)   # odd: the copy back, with its table
    return [b.download_state(m, l) for m in range(3) for l in range(2)]


def g_clear(b):
    start(b, 15)
    for _ in range(3):
        b.push_state()
    b.clear_states()
    assert b.num_states() == [0, 0, 0]
    b.push_state()
    assert b.num_states() == [1, 1, 1]
    return [b.download_state(m, 0) for m in range(3)]


GROUPS = [g_nothing, g_norm2, g_onepass, g_scratch, g_ritz, g_residuals_phi, g_evolve_states, g_clear]


def everything(b):
    """every group in sequence on one batch (the stores are cleared where a group pushes afresh), then phi, the stored states
    and the Ritz values"""
    out = []
    for g in GROUPS:
        if g in (g_onepass, g_ritz, g_evolve_states, g_clear):
            b.clear_states()
        out += g(b)
    b.set_gs_variant(-1)
    r = b.ritz()
    out += [x["evals"] for x in r if x["status"] == 0]
    out += [b.download_phi(m) for m in range(3)]
    out += [b.download_state(m, l) for m, n in enumerate(b.num_states()) for l in range(n)]
    return out


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ext", [1, 3])
@pytest.mark.parametrize("kind", ["mixed", "uniform"])
def test_every_group_alone_then_all_of_them(wa, kind, ext, dtype):
    for g in GROUPS:
        b = make(wa, kind, ext, dtype)
        try:
            got = g(b)
            assert all(np.all(np.isfinite(x)) for x in got), g.__name__
            if g is g_residuals_phi:
                assert b.ritz_counts() == (0, 0)   # no Rayleigh-Ritz call made its tables first
        finally:
            b.close()
    first, second = make(wa, kind, ext, dtype), make(wa, kind, ext, dtype)
    try:
        a = everything(first)
        first.close()
        c = everything(second)
    finally:
        first.close()
        second.close()
    assert len(a) == len(c) and len(a) > 20
    for i, (x, y) in enumerate(zip(a, c)):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), "output %d differs between two batches running the same sequence" % i
