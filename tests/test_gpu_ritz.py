"""Rayleigh-Ritz on the stored states, on the device: wafer_k_ritz_sums and wafer_k_rotate_states through Context.ritz_matrices /
rotate_states / ritz, against the context's own observables (==), the numpy model of tests/ritz_model.py, closed-form levels of
the particle in a box, a fresh context after a rotation, and the wafer-hip driver's `gpu.ritz` step.

Shapes: smaller than a tile, odd sizes, and one whose observables launch has several tiles in x and y and several z-chunks
(the tile is 128 x 16 cells on doubles, 256 x 16 on floats, 8 rows high for SevenPoint).  The stored states are N(0, 1) on the
work cells AND on the frame unless a test says otherwise.

G1 holds on a random frame because wafer_observables' kernel (wafer_k_step_lds, NLOW = -2) reads every frame cell as it is
stored, the halo columns left and right of the work area included (the step kernels take those as the zeros the engine's own
states hold there; the observables mode did too before the sums kernel existed, and then missed the model's energy on a loaded
frame: f64 (12, 10, 9) ThreePoint gave 66858.55838404773 where the model and h[0][0] have 66747.354260761)."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import ritz_model as rm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DN, DT, MASS = 0.2, 0.004, 1.3
KS = [1, 2, 4, 5, 8]
DTYPES = ["f64", "f32", "f32fast"]
SMALL = [(12, 10, 9), (17, 17, 17), (3, 2, 5)]


def shapes_of(dtype):
    return SMALL + [(130, 20, 40) if dtype == "f64" else (258, 20, 40)]


CASES = [(dtype, shape, ext) for dtype in DTYPES for shape in shapes_of(dtype) for ext in (1, 2, 3)]


def storage_of(dtype):
    return np.float64 if dtype == "f64" else np.float32


class Cfg:
    """what the model reads"""

    def __init__(self, ext, dn=DN, mass=MASS):
        self.ext, self.dn, self.mass = ext, dn, mass


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


def params_of(wa, shape, ext, dtype, max_states=8, **kw):
    return wa.Params(*shape, dn=DN, dt=DT, mass=MASS, central_difference=ext, dtype=dtype, max_states=max_states, **kw)


def seed_of(dtype, shape, ext):
    return 1000 * DTYPES.index(dtype) + 10 * sum(shape) + ext


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def measured(dtype, shape, ext, frame):
    """one context per case: eight random stored states, ritz_matrices for every k of KS, observables of every state, and the
    model's matrices of the downloaded states under the downloaded V -- computed once, shared by the tests below"""
    import wafer_amd as wa
    states = rm.random_states(shape, ext, 8, seed_of(dtype, shape, ext), frame=frame, storage=storage_of(dtype))
    with wa.Context(params_of(wa, shape, ext, dtype)) as ctx:
        ctx.set_potential("Harmonic")
        for j, l in enumerate(states):
            ctx.load_state(j, l)
        down = [ctx.download_state(j) for j in range(8)]
        v = ctx.download_array("v")
        mats = {k: ctx.ritz_matrices(k) for k in KS}
        obs = []
        for j in range(8):
            ctx.clone_state_to_phi(j)
            obs.append(ctx.observables())
    for a, b in zip(states, down):
        assert np.array_equal(a, b)              # the store holds what was loaded, frame included
    return dict(mats=mats, obs=obs, model=rm.matrices(Cfg(ext), v, down, scales=True))


# ---- G1: the diagonal is wafer_observables on that state, bit for bit ------------------------------------------------------------
def check_diagonal(m):
    for k in KS:
        h, s = m["mats"][k]
        for j in range(k):
            print(k, j, repr(h[j, j]), repr(m["obs"][j]["energy"]), repr(s[j, j]), repr(m["obs"][j]["norm2"]))
    for k in KS:
        h, s = m["mats"][k]
        for j in range(k):
            assert s[j, j] == m["obs"][j]["norm2"], (k, j)
            assert h[j, j] == m["obs"][j]["energy"], (k, j, h[j, j], m["obs"][j]["energy"], m["model"][0][j, j])


@pytest.mark.parametrize("dtype,shape,ext", CASES)
def test_diagonal_is_observables(dtype, shape, ext):
    check_diagonal(measured(dtype, shape, ext, True))


@pytest.mark.parametrize("dtype,shape,ext", CASES)
def test_diagonal_is_observables_zero_frame(dtype, shape, ext):
    check_diagonal(measured(dtype, shape, ext, False))


# ---- G2: all of h and s against the model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", [True, False], ids=["random_frame", "zero_frame"])
@pytest.mark.parametrize("dtype,shape,ext", CASES)
def test_matrices_against_the_model(dtype, shape, ext, frame):
    m = measured(dtype, shape, ext, frame)
    mh, ms, ah, as_ = m["model"]
    for k in KS:
        h, s = m["mats"][k]
        assert h.shape == (k, k) and s.shape == (k, k)
        assert np.all(np.abs(h - mh[:k, :k]) <= 1e-12 * ah[:k, :k]), (k, np.max(np.abs(h - mh[:k, :k]) / ah[:k, :k]))
        assert np.all(np.abs(s - ms[:k, :k]) <= 1e-12 * as_[:k, :k]), (k, np.max(np.abs(s - ms[:k, :k]) / as_[:k, :k]))
        assert np.array_equal(bits(s), bits(s.T)), k
        if k > 1:
            assert np.count_nonzero(h - np.diag(np.diag(h))) == k * (k - 1)


# ---- G3: the rotation, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dtype,shape,ext", CASES)
def test_rotation_against_the_model(wa, dtype, shape, ext, k):
    n = min(8, k + 2)                            # two states beyond k, which must keep every bit
    states = rm.random_states(shape, ext, n + 1, seed_of(dtype, shape, ext) + k, storage=storage_of(dtype))
    coef = np.random.default_rng(k).standard_normal((k, k))
    with wa.Context(params_of(wa, shape, ext, dtype)) as ctx:
        for j in range(n):
            ctx.load_state(j, states[j])
        ctx.upload_phi(states[n])
        ctx.rotate_states(coef)
        got = [ctx.download_state(j) for j in range(n)]
        phi = ctx.download_phi()
    want = rm.rotate(states[:k], coef, storage_of(dtype)) + states[k:n]
    for j in range(n):
        assert np.array_equal(bits(got[j]), bits(want[j])), (j, int(np.count_nonzero(bits(got[j]) != bits(want[j]))))
    assert np.array_equal(bits(phi), bits(states[n]))


def test_rotation_keeps_the_zeros_outside_the_frame(wa):
    """the kernel runs over pad and guard cells too: a step that reads them must see what it saw before.  ThreePoint steps of a
    state after rotate_states(identity permutation) equal the steps of the same state in a fresh context"""
    shape, ext = (17, 17, 17), 1
    states = rm.random_states(shape, ext, 3, 5, frame=False)
    perm = np.eye(2)[:, ::-1].copy()
    out = []
    for rotate in (True, False):
        with wa.Context(params_of(wa, shape, ext, "f64")) as ctx:
            ctx.set_potential("Harmonic")
            order = (1, 0) if rotate else (0, 1)
            for j in range(2):
                ctx.load_state(j, states[order[j]])
            if rotate:
                ctx.rotate_states(perm)
            ctx.upload_phi(states[2])
            ctx.evolve(2, 5)
            out.append(ctx.download_phi())
    assert np.array_equal(bits(out[0]), bits(out[1]))


# ---- G4: the particle in a box ------------------------------------------------------------------------------------------------------
# fp64 storage only: the check is rel 1e-12 against closed forms, and float storage rounds the states themselves at 6e-8.
MIX = np.array([[1.0, 0.3, 0.2, 0.1], [0.2, 1.0, 0.3, 0.1], [0.1, 0.2, 1.0, 0.3], [0.3, 0.1, 0.2, 1.0]])   # cond ~ 3
LEVELS = [(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2)]


def box_ritz(wa, shape):
    sines = [rm.sine_state(shape, 1, p) for p in LEVELS]
    mixed = [sum(MIX[a, b] * sines[b] for b in range(4)) for a in range(4)]
    with wa.Context(wa.Params(*shape, dn=DN, dt=DT, mass=MASS, central_difference=1, max_states=4)) as ctx:
        ctx.set_potential("NoPotential")
        for j, l in enumerate(mixed):
            ctx.load_state(j, l)
        res = ctx.ritz(4)
        down = [ctx.download_state(j) for j in range(4)]
        v = ctx.download_array("v")
    return sines, res, down, v


def test_box_levels_and_states():
    import wafer_amd as wa
    shape = (12, 10, 9)
    sines, res, down, _ = box_ritz(wa, shape)
    exact = np.array([rm.sine_level(shape, p, DN, MASS) for p in LEVELS])
    order = np.argsort(exact)
    assert np.all(np.diff(exact[order]) > 1e-3 * exact[order][0])          # four distinct levels: not a cube
    assert np.all(np.abs(res["evals"] - exact[order]) <= 1e-12 * exact[order]), (res["evals"], exact[order])
    for a in range(4):
        want = sines[order[a]]
        err = min(np.max(np.abs(down[a] - want)), np.max(np.abs(down[a] + want)))
        assert err <= 1e-12, (a, err)


def test_box_threefold_level_on_a_cube():
    """(2, 1, 1), (1, 2, 1), (1, 1, 2) share a level on a cube: any orthonormal basis of the shell is right, so the states are
    held to the invariants S' = 1 and H' = diag(evals), both from the model on the downloaded states.  Bounds: the solver's
    own 1e-12 (tests/test_ritz_host.py) plus the rounding of the rotated states, 2^-53 per cell, far below it."""
    import wafer_amd as wa
    shape = (10, 10, 10)
    _, res, down, v = box_ritz(wa, shape)
    exact = np.sort([rm.sine_level(shape, p, DN, MASS) for p in LEVELS])
    assert exact[1] == exact[2] == exact[3] or np.ptp(exact[1:]) <= 4 * np.spacing(exact[1])
    assert np.all(np.abs(res["evals"] - exact) <= 1e-12 * exact), (res["evals"], exact)
    h, s = rm.matrices(Cfg(1), v, down)
    assert np.max(np.abs(s - np.eye(4))) <= 1e-12
    assert np.max(np.abs(h - np.diag(res["evals"]))) <= 1e-12 * np.max(np.abs(exact))


# ---- G5: everything derived from the store is forgotten ------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [None, 0, 1, 2, 3])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_evolve_after_ritz_equals_a_fresh_context(wa, dtype, variant):
    shape, ext = (12, 10, 9), 1
    start = rm.random_states(shape, ext, 3, 77, frame=False, storage=storage_of(dtype))

    def prepared(ctx):
        ctx.set_potential("Harmonic")
        if variant is not None:
            ctx.set_stencil_variant(variant)

    with wa.Context(params_of(wa, shape, ext, dtype)) as ctx:
        prepared(ctx)
        for j in range(2):
            ctx.load_state(j, start[j])
        ctx.upload_phi(start[2])
        ctx.evolve(2, 8)
        if variant != 0:
            assert ctx.x2_passes() > 0          # the two-step pass is armed: images M_j and their matrix are in use
        ctx.ritz(2)
        rotated = [ctx.download_state(j) for j in range(2)]
        phi = ctx.download_phi()
        ctx.evolve(2, 6)
        got = ctx.download_phi()
    assert not np.array_equal(rotated[0], start[0])
    with wa.Context(params_of(wa, shape, ext, dtype)) as ctx:
        prepared(ctx)
        for j in range(2):
            ctx.load_state(j, rotated[j])
        ctx.upload_phi(phi)
        ctx.evolve(2, 6)
        want = ctx.download_phi()
    assert np.array_equal(bits(got), bits(want)), int(np.count_nonzero(bits(got) != bits(want)))


# ---- G6: refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(wa):
    from wafer_amd.engine import WAFER_ERR_INVALID, WAFER_ERR_STATE
    shape, ext = (12, 10, 9), 1
    states = rm.random_states(shape, ext, 3, 9)

    def refused(call, code, match=None):
        with pytest.raises(wa.WaferError, match=match) as e:
            call()
        assert e.value.code == code, (e.value.code, code)

    with wa.Context(params_of(wa, shape, ext, "f64", max_states=10)) as ctx:
        for j in range(2):
            ctx.load_state(j, states[j])
        ctx.upload_phi(states[2])
        refused(lambda: ctx.ritz_matrices(2), WAFER_ERR_STATE)                 # no potential yet
        refused(lambda: ctx.ritz(2), WAFER_ERR_STATE)
        ctx.set_potential("Harmonic")
        for call in (ctx.ritz_matrices, ctx.ritz):
            refused(lambda: call(0), WAFER_ERR_INVALID)
            refused(lambda: call(9), WAFER_ERR_INVALID)
            refused(lambda: call(3), WAFER_ERR_STATE)                          # two states stored
        refused(lambda: ctx.rotate_states(np.eye(3)), WAFER_ERR_STATE)
        refused(lambda: ctx.rotate_states(np.eye(9)), WAFER_ERR_INVALID)
        refused(lambda: ctx.rotate_states(np.zeros((0, 0))), WAFER_ERR_INVALID)
        ctx.load_state(2, states[0])                                           # states 0 and 2 are equal: S is singular
        refused(lambda: ctx.ritz(3), WAFER_ERR_STATE)
        for j, want in enumerate([states[0], states[1], states[0]]):
            assert np.array_equal(bits(ctx.download_state(j)), bits(want)), j
        assert np.array_equal(bits(ctx.download_phi()), bits(states[2]))
        refused(lambda: ctx.ritz(), WAFER_ERR_STATE)                           # k = None: all three


def test_a_slab_context_is_refused(wa):
    from wafer_amd.engine import WAFER_ERR_INVALID
    shape, ext = (12, 10, 9), 1
    states = rm.random_states(shape, ext, 2, 4, frame=False)
    with wa.Context(params_of(wa, shape, ext, "f64", z_begin=0, z_count=shape[2])) as ctx:
        ctx.set_potential("Harmonic")
        for j in range(2):
            ctx.load_state(j, states[j])
        for call in (lambda: ctx.ritz_matrices(2), lambda: ctx.ritz(2), lambda: ctx.rotate_states(np.eye(2))):
            with pytest.raises(wa.WaferError, match="z-slab") as e:
                call()
            assert e.value.code == WAFER_ERR_INVALID
        for j in range(2):
            assert np.array_equal(bits(ctx.download_state(j)), bits(states[j]))


# ---- G7: wafer-hip -----------------------------------------------------------------------------------------------------------------------
YAML = """project_name: ritz_cli
grid:
    size:
        x: 20
        y: 20
        z: 20
    dn: 0.5
    dt: 0.04
tolerance: 1e-7
central_difference: ThreePoint
max_steps: 200000
wavenum: 0
wavemax: 2
potential: Harmonic
mass: 1.0
init_condition: Boolean
sig: 1.0
init_symmetry: NotConstrained
output:
    screen_update: 100
    file_type: Csv
    save_wavefns: true
    save_potential: false
"""


def run_cli(tmp_path, name, extra):
    from wafer_amd import build
    d = tmp_path / name
    d.mkdir()
    (d / "wafer.yaml").write_text(YAML + extra)
    r = subprocess.run([build.CLI, "-c", str(d / "wafer.yaml"), "--output-dir", str(d / "out"), "--input-dir", str(d / "in")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    (od,) = os.listdir(d / "out")
    return r, d / "out" / od


def table_of(stdout):
    """stdout without its last two lines (the elapsed time and the output directory's time stamp)"""
    lines = stdout.splitlines()
    assert lines[-2].startswith("Simulation complete.") and lines[-1].startswith("Output directory:")
    return lines[:-2]


def solve_like_the_driver(wa):
    """wafer_cli.cpp's loop (grid.rs:31-47, 50-246) for YAML on a Context; -> the context, three states stored"""
    from wafer_amd.run import rust_lower_exp
    ctx = wa.Context(wa.Params(20, 20, 20, dn=0.5, dt=0.04, mass=1.0, sig=1.0, central_difference=1, max_states=3))
    ctx.set_potential("Harmonic")
    for wnum in range(3):
        if wnum == 0:
            ctx.set_initial_condition("Boolean")
            ctx.symmetrise("NotConstrained")
        else:
            ctx.clone_state_to_phi(wnum - 1)
        cloned, step, last = wnum > 0, 0, sys.float_info.max
        while True:
            obs = ctx.observables()
            energy = obs["energy"] / obs["norm2"]
            ctx.normalise(obs["norm2"])
            if wnum > 0:
                ctx.orthogonalise(wnum)
            if cloned and step == 0:
                n2 = ctx.norm2()
                if not (n2 > 0.0) or not np.isfinite(n2):
                    ctx.set_initial_condition("Gaussian", seed=0x5EED + wnum)
                    cloned, last = False, sys.float_info.max
                    continue
            if abs(energy - last) < 1e-7:
                break
            last = energy
            assert step <= 200000
            ctx.evolve(wnum, 100)
            step += 100
        ctx.push_state()
    return ctx, rust_lower_exp


def test_driver_ritz_step(wa, tmp_path):
    plain, plain_dir = run_cli(tmp_path, "plain", "")
    off, _ = run_cli(tmp_path, "off", "gpu:\n    ritz: false\n")
    on, on_dir = run_cli(tmp_path, "on", "gpu:\n    ritz: true\n")
    assert table_of(plain.stdout) == table_of(off.stdout)
    assert "Ritz" not in plain.stdout
    lines = table_of(on.stdout)
    at = lines.index("Ritz")
    assert lines[:at] == table_of(plain.stdout)                    # the solve itself is untouched
    rows = [l.split() for l in lines[at + 1:at + 4]]
    ctx, fmt = solve_like_the_driver(wa)
    with ctx:
        res = ctx.ritz()
        energies = []
        for a in range(3):
            ctx.clone_state_to_phi(a)
            o = ctx.observables()
            energies.append(o["energy"] / o["norm2"])
    assert res["evals"].shape == (3,)
    for a in range(3):
        assert rows[a] == [str(a), fmt(res["h"][a, a] / res["s"][a, a], 10), fmt(res["evals"][a], 10)], (a, rows[a])
        before = open(plain_dir / f"observables_{a}.csv").read().splitlines()[1].split(",")
        after = open(on_dir / f"observables_{a}.csv").read().splitlines()[1].split(",")
        assert after[0] == str(a) and float(after[1]) == energies[a]                     # rewritten from the rotated state
        assert abs(float(after[1]) - res["evals"][a]) <= 1e-9 * abs(res["evals"][a])
        assert before[0] == after[0]
    assert any(open(plain_dir / f"observables_{a}.csv").read() != open(on_dir / f"observables_{a}.csv").read() for a in range(3))
    # save_wavefns: the files hold the rotated states -- as many lines as before, other values where the rotation mixed
    assert sorted(os.listdir(on_dir)) == sorted(os.listdir(plain_dir))
    texts = [(open(plain_dir / f"wavefunction_{a}.csv").read(), open(on_dir / f"wavefunction_{a}.csv").read()) for a in range(3)]
    assert all(len(p.splitlines()) == len(o.splitlines()) for p, o in texts) and any(p != o for p, o in texts)


def test_sweep_and_run_refuse_the_key(tmp_path):
    d = tmp_path / "k"
    d.mkdir()
    (d / "wafer.yaml").write_text(YAML + "gpu:\n    ritz: true\n")
    for module, extra in (("wafer_amd.sweep", ["--plan"]), ("wafer_amd.run", [])):
        r = subprocess.run([sys.executable, "-m", module, "-c", str(d / "wafer.yaml"), *extra], capture_output=True, text=True, cwd=ROOT, timeout=120)
        assert r.returncode != 0 and "gpu.ritz" in r.stderr and len(r.stderr.strip().splitlines()) == 1, (module, r.stderr)
    (d / "wafer.yaml").write_text(YAML)
    r = subprocess.run([sys.executable, "-m", "wafer_amd.sweep", "-c", str(d / "wafer.yaml"), "--plan"], capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
