"""Residuals r = H l - theta l on the device: wafer_k_residual_sums and wafer_k_residual_write through Context.residuals /
residual_to_phi, against the numpy model of tests/residual_model.py (cells bit for bit, sums to 1e-12 of sum |terms|), the
context's own observables and Ritz sums (==), closed-form levels of the particle in a box, and the wafer-hip driver's
`gpu.residual` block.

Cases follow tests/test_gpu_ritz.py: shapes smaller than a tile, odd sizes, and one whose launch has several tiles in x and y and
several z-chunks; eight N(0, 1) stored states, on a random frame and on a zero frame; Harmonic V.

The C ABI returns theta, r2 and s, not wh: wh is seen through Rayleigh mode's theta = wh / s.  So "wh against the model" is
|theta * s - wh_model| <= 1e-12 sum |w hw| (the quotient's and the product's roundings are 2^-52 |wh| together, far below), and
"theta equals wh / s of a theta = 0 call" is held as: Rayleigh mode's theta has the same bits for every k, its r2 and s are those
of the call given that theta, and theta * s meets the model's wh."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import residual_model as res  # noqa: E402
from tests import ritz_model as rm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DN, DT, MASS = 0.2, 0.004, 1.3
KS = [1, 2, 4, 5, 8]
DTYPES = ["f64", "f32", "f32fast"]
SMALL = [(12, 10, 9), (17, 17, 17), (3, 2, 5)]
CELL_STATES = (0, 7)
FIXED = -3.5


def shapes_of(dtype):
    return SMALL + [(130, 20, 40) if dtype == "f64" else (258, 20, 40)]


CASES = [(dtype, shape, ext) for dtype in DTYPES for shape in shapes_of(dtype) for ext in (1, 2, 3)]
FRAMES = pytest.mark.parametrize("frame", [True, False], ids=["random_frame", "zero_frame"])


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
    return 2000 * (1 + DTYPES.index(dtype)) + 10 * sum(shape) + ext


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def work(p, e):
    return p[e:-e, e:-e, e:-e]


@functools.lru_cache(maxsize=None)
def measured(dtype, shape, ext, frame):
    """one context per case, computed once and shared by the tests below: eight random stored states; Rayleigh mode and the call
    given that theta for every k of KS; theta = 0 and theta = -3.5 on all eight; the Ritz overlap diagonal and observables' norm2;
    the phi source on every state; residual_to_phi of two states with three thetas each over a phi that held a random frame"""
    import wafer_amd as wa
    states = rm.random_states(shape, ext, 9, seed_of(dtype, shape, ext), frame=frame, storage=storage_of(dtype))
    cfg = Cfg(ext)
    with wa.Context(params_of(wa, shape, ext, dtype)) as ctx:
        ctx.set_potential("Harmonic")
        for j in range(8):
            ctx.load_state(j, states[j])
        v = ctx.download_array("v")
        quot = [res.rayleigh(cfg, v, states[j])[0] for j in range(8)]
        ray = {k: ctx.residuals(k) for k in KS}
        given = {k: ctx.residuals(k, theta=ray[8]["theta"][:k]) for k in KS}
        zero = ctx.residuals(8, theta=np.zeros(8))
        fixed = ctx.residuals(8, theta=np.full(8, FIXED))
        sdiag = np.diag(ctx.ritz_matrices(8)[1]).copy()
        norm2, phi_ray, phi_given = [], [], []
        for j in range(8):
            ctx.clone_state_to_phi(j)
            norm2.append(ctx.observables()["norm2"])
            phi_ray.append(ctx.residuals(source="phi"))
            phi_given.append(ctx.residuals(1, theta=[FIXED], source="phi"))
        cells = {}
        for j in CELL_STATES:
            for theta in (0.0, quot[j], FIXED):
                ctx.upload_phi(states[8])             # (a random frame unless frame is False: the writer must zero it)
                ctx.residual_to_phi(j, theta)
                cells[j, theta] = ctx.download_phi()
        down = [ctx.download_state(j) for j in range(8)]
    for a, b in zip(states, down):
        assert np.array_equal(bits(a), bits(b))      # the store holds what was loaded, before and after
    return dict(states=states, v=v, quot=quot, ray=ray, given=given, zero=zero, fixed=fixed, sdiag=sdiag, norm2=norm2, phi_ray=phi_ray,
                phi_given=phi_given, cells=cells)


# ---- R1: cells ----------------------------------------------------------------------------------------------------------------------------
@FRAMES
@pytest.mark.parametrize("dtype,shape,ext", CASES)
def test_cells_against_the_model(dtype, shape, ext, frame):
    m = measured(dtype, shape, ext, frame)
    cfg = Cfg(ext)
    for (j, theta), got in m["cells"].items():
        want = res.cells(cfg, m["v"], m["states"][j], theta, storage_of(dtype))
        gw = work(got, ext)
        assert np.array_equal(bits(gw), bits(want)), (j, theta, int(np.count_nonzero(bits(gw) != bits(want))))
        outside = got.copy()
        work(outside, ext)[...] = 0.0
        assert not np.any(outside), (j, theta)
        assert np.any(gw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_the_residual_is_a_wavefunction_for_the_step_kernels(wa, dtype, ext):
    """pad and guard cells are zeros: steps on the written phi equal the same steps in a fresh context that uploaded it"""
    shape = (17, 17, 17)
    states = rm.random_states(shape, ext, 2, 31 + ext, frame=False, storage=storage_of(dtype))
    with wa.Context(params_of(wa, shape, ext, dtype)) as ctx:
        ctx.set_potential("Harmonic")
        ctx.load_state(0, states[0])
        ctx.upload_phi(states[1])
        ctx.evolve(0, 3)                              # both ping-pong buffers have been written
        ctx.residual_to_phi(0, 1.25)
        r = ctx.download_phi()
        ctx.evolve(0, 5)
        got = ctx.download_phi()
    with wa.Context(params_of(wa, shape, ext, dtype)) as ctx:
        ctx.set_potential("Harmonic")
        ctx.upload_phi(r)
        ctx.evolve(0, 5)
        want = ctx.download_phi()
    assert np.any(r) and np.array_equal(bits(got), bits(want)), int(np.count_nonzero(bits(got) != bits(want)))


# ---- R2: sums -----------------------------------------------------------------------------------------------------------------------------
@FRAMES
@pytest.mark.parametrize("dtype,shape,ext", CASES)
def test_sums_against_the_model(dtype, shape, ext, frame):
    m = measured(dtype, shape, ext, frame)
    cfg = Cfg(ext)
    for j in range(8):
        l = m["states"][j]
        theta = m["ray"][8]["theta"][j]
        for label, out, th in (("rayleigh", m["ray"][8], theta), ("zero", m["zero"], 0.0), ("fixed", m["fixed"], FIXED)):
            r2, wh, s, awh = res.sums(cfg, m["v"], l, th, scales=True)
            print(label, j, repr(out["r2"][j]), repr(r2), repr(out["norm2"][j]), repr(s))
            assert out["theta"][j] == th
            assert abs(out["r2"][j] - r2) <= 1e-12 * r2, (label, j, out["r2"][j], r2)          # (terms r * r: their own scale)
            assert abs(out["norm2"][j] - s) <= 1e-12 * s, (label, j)
            assert out["rho"][j] == np.sqrt(out["r2"][j] / out["norm2"][j])
        _, wh, s, awh = res.sums(cfg, m["v"], l, 0.0, scales=True)
        print("wh", j, repr(theta * m["ray"][8]["norm2"][j]), repr(wh), awh)
        assert abs(theta * m["ray"][8]["norm2"][j] - wh) <= 1e-12 * awh, (j, theta, wh, awh)


@FRAMES
@pytest.mark.parametrize("dtype,shape,ext", CASES)
def test_norm2_is_the_ritz_overlap_and_observables(dtype, shape, ext, frame):
    m = measured(dtype, shape, ext, frame)
    for out in (m["ray"][8], m["given"][8], m["zero"], m["fixed"]):
        for j in range(8):
            assert out["norm2"][j] == m["sdiag"][j] == m["norm2"][j], (j, out["norm2"][j], m["sdiag"][j], m["norm2"][j])


@FRAMES
@pytest.mark.parametrize("dtype,shape,ext", CASES)
def test_a_state_has_the_same_bits_for_every_k(dtype, shape, ext, frame):
    m = measured(dtype, shape, ext, frame)
    for k in KS:
        for name in ("theta", "r2", "norm2"):
            assert m["ray"][k][name].shape == (k,)
            assert np.array_equal(bits(m["ray"][k][name]), bits(m["ray"][8][name][:k])), (k, name)


# ---- R3: Rayleigh mode ---------------------------------------------------------------------------------------------------------------------
@FRAMES
@pytest.mark.parametrize("dtype,shape,ext", CASES)
def test_rayleigh_mode_is_the_call_given_its_theta(dtype, shape, ext, frame):
    m = measured(dtype, shape, ext, frame)
    for k in KS:
        for name in ("theta", "r2", "norm2", "rho"):
            assert np.array_equal(bits(m["ray"][k][name]), bits(m["given"][k][name])), (k, name)
    # and the quotient is a minimum of r2 over theta: no more than at 0 or at -3.5
    assert np.all(m["ray"][8]["r2"] <= m["zero"]["r2"]) and np.all(m["ray"][8]["r2"] <= m["fixed"]["r2"])


# ---- R5: the phi source -----------------------------------------------------------------------------------------------------------------------
@FRAMES
@pytest.mark.parametrize("dtype,shape,ext", CASES)
def test_phi_source_is_the_states_source(dtype, shape, ext, frame):
    m = measured(dtype, shape, ext, frame)
    for j in range(8):
        for name in ("theta", "r2", "norm2"):
            assert m["phi_ray"][j][name].shape == (1,)
            assert bits(m["phi_ray"][j][name])[0] == bits(m["ray"][8][name])[j], (j, name)
            assert bits(m["phi_given"][j][name])[0] == bits(m["fixed"][name])[j], (j, name)


# ---- R4: the particle in a box (f64: the bounds are rel 1e-12 and below) ------------------------------------------------------------------------
BOX = (12, 10, 9)
LEVELS = [(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2)]
MIX = np.array([[1.0, 0.3, 0.2, 0.1], [0.2, 1.0, 0.3, 0.1], [0.1, 0.2, 1.0, 0.3], [0.3, 0.1, 0.2, 1.0]])


def box_context(wa, states):
    ctx = wa.Context(wa.Params(*BOX, dn=DN, dt=DT, mass=MASS, central_difference=1, max_states=len(states)))
    ctx.set_potential("NoPotential")
    for j, l in enumerate(states):
        ctx.load_state(j, l)
    return ctx


def test_box_states_on_the_device(wa):
    sines = [rm.sine_state(BOX, 1, p) for p in LEVELS]
    E = np.array([rm.sine_level(BOX, p, DN, MASS) for p in LEVELS])
    c = np.array([1.0, 0.3, 0.2, 0.1])
    eps = 1e-3
    with box_context(wa, sines + [sum(ci * si for ci, si in zip(c, sines)), sines[0] + eps * sines[1]]) as ctx:
        pure = ctx.residuals(4, theta=E)
        ray = ctx.residuals(6)
        zero = ctx.residuals(6, theta=np.zeros(6))
    print(pure["rho"] / E)
    assert np.all(pure["rho"] <= 1e-13 * E), pure["rho"] / E
    want_theta = np.sum(c * c * E) / np.sum(c * c)
    want_r2 = np.sum(c * c * (E - want_theta) ** 2)
    want_zero = np.sum(c * c * E * E)
    print(abs(ray["theta"][4] - want_theta) / want_theta, abs(ray["r2"][4] - want_r2) / want_r2, abs(zero["r2"][4] - want_zero) / want_zero)
    assert abs(ray["theta"][4] - want_theta) <= 1e-12 * want_theta
    assert abs(ray["r2"][4] - want_r2) <= 1e-12 * want_r2
    assert abs(zero["r2"][4] - want_zero) <= 1e-12 * want_zero
    theta = ray["theta"][5]
    want = eps * eps * (E[1] - theta) ** 2 + (E[0] - theta) ** 2
    print(abs(ray["r2"][5] - want) / want)
    assert abs(ray["r2"][5] - want) <= 1e-10 * want, (ray["r2"][5], want)


def test_ritz_values_of_the_box_are_converged(wa):
    sines = [rm.sine_state(BOX, 1, p) for p in LEVELS]
    E = np.array([rm.sine_level(BOX, p, DN, MASS) for p in LEVELS])
    with box_context(wa, [sum(MIX[a, b] * sines[b] for b in range(4)) for a in range(4)]) as ctx:
        before = ctx.residuals(4)
        evals = ctx.ritz(4)["evals"]
        after = ctx.residuals(4, theta=evals)
    print(before["rho"], after["rho"] / np.max(E))
    assert np.all(before["rho"] > 1e-3 * np.max(E))                 # the mixed states are far from eigenstates
    assert np.all(after["rho"] <= 1e-12 * np.max(E)), after["rho"]


# ---- R6: read-only ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_residuals_change_nothing(wa, dtype):
    shape, ext = (12, 10, 9), 1
    start = rm.random_states(shape, ext, 3, 77, frame=False, storage=storage_of(dtype))
    out = []
    for call in (True, False):
        with wa.Context(params_of(wa, shape, ext, dtype)) as ctx:
            ctx.set_potential("Harmonic")
            for j in range(2):
                ctx.load_state(j, start[j])
            ctx.upload_phi(start[2])
            ctx.evolve(2, 8)
            assert ctx.x2_passes() > 0          # the two-step pass is armed: images M_j and their matrix are in use
            phi = ctx.download_phi()
            if call:
                ctx.residuals(2)
                ctx.residuals(2, theta=[1.0, -2.0])
                ctx.residuals(source="phi")
                for j in range(2):
                    assert np.array_equal(bits(ctx.download_state(j)), bits(start[j])), j
                assert np.array_equal(bits(ctx.download_phi()), bits(phi))
            ctx.evolve(2, 6)
            out.append(ctx.download_phi())
    assert np.array_equal(bits(out[0]), bits(out[1])), int(np.count_nonzero(bits(out[0]) != bits(out[1])))


# ---- R7: refusals -----------------------------------------------------------------------------------------------------------------------------
def raw(wa, ctx, source, k, theta_in):
    """wafer_residuals on sentinel-filled outputs -> (rc, outputs)"""
    import ctypes as C
    dp = C.POINTER(C.c_double)
    out = np.full((3, 8), -77.0)
    tin = None if theta_in is None else np.ascontiguousarray(theta_in, dtype=np.float64)
    rc = ctx._L.wafer_residuals(ctx._h, source, k, None if tin is None else tin.ctypes.data_as(dp), out[0].ctypes.data_as(dp),
                                out[1].ctypes.data_as(dp), out[2].ctypes.data_as(dp))
    return rc, out


def test_refusals_change_nothing(wa):
    from wafer_amd.engine import WAFER_ERR_INVALID, WAFER_ERR_STATE, WAFER_OK
    shape, ext = (12, 10, 9), 1
    states = rm.random_states(shape, ext, 3, 9)

    def refused(source, k, theta_in, code):
        rc, out = raw(wa, ctx, source, k, theta_in)
        assert rc == code, (source, k, rc, code)
        assert np.all(out == -77.0)

    with wa.Context(params_of(wa, shape, ext, "f64", max_states=10)) as ctx:
        for j in range(2):
            ctx.load_state(j, states[j])
        refused(0, 2, None, WAFER_ERR_STATE)                                    # no potential yet
        assert ctx._L.wafer_residual_to_phi(ctx._h, 0, 1.0) == WAFER_ERR_STATE
        ctx.set_potential("Harmonic")
        refused(1, 1, None, WAFER_ERR_STATE)                                    # phi not set
        ctx.upload_phi(states[2])
        refused(0, 0, None, WAFER_ERR_INVALID)
        refused(0, 9, None, WAFER_ERR_INVALID)
        refused(1, 2, None, WAFER_ERR_INVALID)                                  # the phi source is one array
        refused(2, 1, None, WAFER_ERR_INVALID)                                  # unknown source
        refused(-1, 1, None, WAFER_ERR_INVALID)
        refused(0, 2, [1.0, np.nan], WAFER_ERR_INVALID)
        refused(0, 2, [np.inf, 1.0], WAFER_ERR_INVALID)
        refused(0, 3, None, WAFER_ERR_STATE)                                    # two states stored
        refused(0, 3, [1.0, 2.0, 3.0], WAFER_ERR_STATE)
        assert ctx._L.wafer_residual_to_phi(ctx._h, 2, 1.0) == WAFER_ERR_STATE
        assert ctx._L.wafer_residual_to_phi(ctx._h, 0, float("nan")) == WAFER_ERR_INVALID
        ctx.load_state(2, np.zeros_like(states[0]))                             # a zero state has no Rayleigh quotient
        refused(0, 3, None, WAFER_ERR_STATE)
        assert "state 2" in ctx._L.wafer_last_error().decode()
        rc, out = raw(wa, ctx, 0, 3, [1.0, 2.0, 3.0])                           # ... but a residual with theta given: zero
        assert rc == WAFER_OK and out[1][2] == 0.0 and out[2][2] == 0.0 and out[0][2] == 3.0
        for j, want in enumerate([states[0], states[1], np.zeros_like(states[0])]):
            assert np.array_equal(bits(ctx.download_state(j)), bits(want)), j
        assert np.array_equal(bits(ctx.download_phi()), bits(states[2]))
        with pytest.raises(wa.WaferError) as e:
            ctx.residuals()                                                     # k = None: all three, Rayleigh mode
        assert e.value.code == WAFER_ERR_STATE


def test_a_slab_context_is_refused(wa):
    from wafer_amd.engine import WAFER_ERR_INVALID
    shape, ext = (12, 10, 9), 1
    states = rm.random_states(shape, ext, 2, 4, frame=False)
    with wa.Context(params_of(wa, shape, ext, "f64", z_begin=0, z_count=shape[2])) as ctx:
        ctx.set_potential("Harmonic")
        for j in range(2):
            ctx.load_state(j, states[j])
        for call in (lambda: ctx.residuals(2), lambda: ctx.residuals(2, theta=[1.0, 2.0]), lambda: ctx.residuals(source="phi"),
                     lambda: ctx.residual_to_phi(0, 1.0)):
            with pytest.raises(wa.WaferError, match="z-slab") as e:
                call()
            assert e.value.code == WAFER_ERR_INVALID
        for j in range(2):
            assert np.array_equal(bits(ctx.download_state(j)), bits(states[j]))


# ---- R8: wafer-hip ------------------------------------------------------------------------------------------------------------------------------
def test_driver_residual_block(wa, tmp_path):
    from tests.test_gpu_ritz import run_cli, solve_like_the_driver, table_of
    plain, _ = run_cli(tmp_path, "plain", "")
    off, _ = run_cli(tmp_path, "off", "gpu:\n    residual: false\n")
    on, _ = run_cli(tmp_path, "on", "gpu:\n    residual: true\n")
    both, _ = run_cli(tmp_path, "both", "gpu:\n    ritz: true\n    residual: true\n")
    ritz, _ = run_cli(tmp_path, "ritz", "gpu:\n    ritz: true\n")
    assert table_of(plain.stdout) == table_of(off.stdout) and "Residual" not in plain.stdout
    lines = table_of(on.stdout)
    at = lines.index("Residual")
    assert lines[:at] == table_of(plain.stdout)                    # everything before the block is the plain run's
    ctx, fmt = solve_like_the_driver(wa)
    with ctx:
        res0 = ctx.residuals()
        ctx.ritz()
        res1 = ctx.residuals()
    assert res0["theta"].shape == (3,) and len(lines) == at + 5 and lines[at + 4] == ""
    for a in range(3):
        assert lines[at + 1 + a] == "%3d %19s %19s" % (a, fmt(res0["theta"][a], 10), fmt(res0["rho"][a], 10)), (a, lines[at + 1 + a])
    lines = table_of(both.stdout)
    at = lines.index("Residual")
    assert lines[:at] == table_of(ritz.stdout) and "Ritz" in lines[:at]   # the Ritz block is unchanged, the residuals come after it
    for a in range(3):
        assert lines[at + 1 + a] == "%3d %19s %19s" % (a, fmt(res1["theta"][a], 10), fmt(res1["rho"][a], 10)), (a, lines[at + 1 + a])
