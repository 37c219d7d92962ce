"""Residuals r = H l - theta l, the parts that need no GPU: the numpy model of tests/residual_model.py on box states with known
levels and against the oracle's observables, why the API takes two passes, the four entry points' ABI, the argument checks of
Context and Batch before any library call, and the driver's and the sweep's handling of `gpu.residual` / --residuals.

Box states: the particle in a box on the ThreePoint stencil with V = 0, shape (12, 10, 9): sin_p is an exact eigenvector of the
discrete H with level E_p = sine_level(p), the sines are orthonormal, so for l = sum c_p sin_p
    theta_Rayleigh = sum c^2 E / sum c^2        r2(theta) = sum c^2 (E - theta)^2."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import residual_model as res
from tests import ritz_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "golden", "cli_case.yaml")
CALLS = {"wafer_residuals": 7, "wafer_residual_to_phi": 3, "wafer_batch_residuals": 9, "wafer_batch_diag_residual_counts": 3}
SHAPE, DN, MASS = (12, 10, 9), 0.2, 1.3
LEVELS = [(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2)]


class Cfg:
    """what the model reads"""

    def __init__(self, ext=1, dn=DN, mass=MASS):
        self.ext, self.dn, self.mass = ext, dn, mass


def box():
    sines = [rm.sine_state(SHAPE, 1, p) for p in LEVELS]
    E = np.array([rm.sine_level(SHAPE, p, DN, MASS) for p in LEVELS])
    return sines, E, np.zeros_like(sines[0])


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    from wafer_amd import build
    if not os.path.exists(build.LIB):
        build.build()
    wafer_amd.load_library()
    return wafer_amd


# ---- box states ------------------------------------------------------------------------------------------------------------------------
def test_a_pure_level_has_no_residual():
    sines, E, v = box()
    for l, e in zip(sines, E):
        r2, wh, s = res.sums(Cfg(), v, l, e)
        rho = np.sqrt(r2 / s)
        print(e, rho / e)
        assert rho <= 1e-13 * e, (e, rho)
        assert abs(wh / s - e) <= 1e-13 * e


def test_a_mixture_against_the_closed_forms():
    sines, E, v = box()
    c = np.array([1.0, 0.3, 0.2, 0.1])
    l = sum(ci * si for ci, si in zip(c, sines))
    theta, r2, s = res.rayleigh(Cfg(), v, l)
    want_theta = np.sum(c * c * E) / np.sum(c * c)
    want_r2 = np.sum(c * c * (E - want_theta) ** 2)
    r2_zero = res.sums(Cfg(), v, l, 0.0)[0]
    want_zero = np.sum(c * c * E * E)
    print(abs(theta - want_theta) / want_theta, abs(r2 - want_r2) / want_r2, abs(r2_zero - want_zero) / want_zero)
    assert abs(theta - want_theta) <= 1e-12 * want_theta
    assert abs(r2 - want_r2) <= 1e-12 * want_r2
    assert abs(r2_zero - want_zero) <= 1e-12 * want_zero
    assert abs(s - np.sum(c * c)) <= 1e-12 * np.sum(c * c)


def nearly_converged(eps):
    sines, E, v = box()
    l = sines[0] + eps * sines[1]
    theta = (E[0] + eps * eps * E[1]) / (1.0 + eps * eps)
    return l, v, theta, eps * eps * (E[1] - theta) ** 2 + (E[0] - theta) ** 2


def test_a_nearly_converged_state_in_rayleigh_mode():
    """the bound the GPU file relies on: per-cell rounding of hw, about 4 ulp E |w|, against |r| ~ eps dE |w| at eps = 1e-3, with
    margin for another summation order: rel 1e-10"""
    l, v, _, want = nearly_converged(1e-3)
    _, r2, _ = res.rayleigh(Cfg(), v, l)
    print(abs(r2 - want) / want)
    assert abs(r2 - want) <= 1e-10 * want, (r2, want)


def test_one_pass_cannot_give_the_residual_of_a_nearly_converged_state():
    """why the API takes two passes: at eps = 1e-9 the expansion sum (Hl)^2 - 2 theta sum l Hl + theta^2 sum l^2 is lost to
    cancellation, while forming r per cell with theta known is not"""
    l, v, _, want = nearly_converged(1e-9)
    cfg = Cfg()
    w, hw = res._hw(cfg, v, l)
    hh, wh, s = np.sum(hw * hw), np.sum(w * hw), np.sum(w * w)
    theta = wh / s
    one_pass = hh - 2.0 * theta * wh + theta * theta * s
    _, two_pass, _ = res.rayleigh(cfg, v, l)
    print(one_pass, two_pass, want)
    assert not (0.5 * want <= one_pass <= 2.0 * want), (one_pass, want)
    assert abs(two_pass - want) <= 1e-5 * want, (two_pass, want)


# ---- the model against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_model_rayleigh_quotient_is_the_oracles_energy(oracle, ext):
    cfg = oracle.Config(17, 17, 17, ext=ext, potential="Harmonic", dn=0.2, dt=0.004, mass=1.3)
    v = oracle.potential_generate(cfg)
    (l,) = rm.random_states(cfg.work_shape, ext, 1, seed=40 + ext, frame=False)
    _, wh, s = res.sums(cfg, v, l, 0.0)
    want = oracle.observables(cfg, v, l)
    assert abs(s - want["norm2"]) <= 1e-12 * want["norm2"]
    assert abs(wh / s - want["energy"] / want["norm2"]) <= 1e-12 * abs(want["energy"] / want["norm2"]), (ext, wh / s)
    # cells() is sums() before the sum, and the storage rounding is one rounding
    r = res.cells(cfg, v, l, wh / s)
    assert r.shape == cfg.work_shape and abs(np.sum(r * r) - res.sums(cfg, v, l, wh / s)[0]) == 0.0
    r32 = res.cells(cfg, v, l, wh / s, np.float32)
    assert np.array_equal(r32, r.astype(np.float32).astype(np.float64)) and not np.array_equal(r32, r)


# ---- ABI and bindings ------------------------------------------------------------------------------------------------------------------------
def test_the_four_calls_are_declared_exported_bound_and_mirrored(wa):
    import wafer_amd.engine as eng
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wafer_hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    L = wa.load_library()
    assert re.search(r"#define\s+WAFER_ABI_VERSION\s+1\b", header) and L.wafer_abi_version() == 1
    assert re.search(r"#define\s+WAFER_RESIDUAL_STATES\s+0\b", header) and re.search(r"#define\s+WAFER_RESIDUAL_PHI\s+1\b", header)
    assert eng.RESIDUAL_SOURCES == {"states": 0, "phi": 1}
    for name, arity in CALLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m and m.group(1).count(",") + 1 == arity, name
        assert name in eng.EXPORTS and hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == arity, name
        r = re.search(r"pub fn %s\s*\((.*?)\)\s*->\s*c_int" % name, rust, flags=re.S)
        assert r and len([a for a in r.group(1).split(",") if a.strip()]) == arity, name


def test_null_handles_are_refused(wa):
    from wafer_amd.engine import WAFER_ERR_INVALID
    L = wa.load_library()
    d = np.zeros(8)
    dp = d.ctypes.data_as(C.POINTER(C.c_double))
    k = (C.c_uint32 * 1)(1)
    st = (C.c_int * 1)(0)
    n = C.c_uint64(0)
    assert L.wafer_residuals(None, 0, 1, None, dp, dp, dp) == WAFER_ERR_INVALID
    assert "null" in L.wafer_last_error().decode()
    assert L.wafer_residual_to_phi(None, 0, 0.0) == WAFER_ERR_INVALID
    assert L.wafer_batch_residuals(None, 0, None, k, None, dp, dp, dp, st) == WAFER_ERR_INVALID
    assert L.wafer_batch_diag_residual_counts(None, C.byref(n), C.byref(n)) == WAFER_ERR_INVALID
    assert "null" in L.wafer_last_error().decode()
    assert np.all(d == 0.0)


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError("argument check missing: %s reached the library" % name)


def test_context_arguments_are_checked_before_the_library(wa):
    c = object.__new__(wa.Context)
    c._L, c._h = _NoDevice(), None
    for k in (0, 9, -1):
        with pytest.raises(ValueError, match="RITZ_MAX"):
            c.residuals(k)
    with pytest.raises(ValueError, match="source"):
        c.residuals(1, source="store")
    with pytest.raises(ValueError, match="k = 1"):
        c.residuals(2, source="phi")
    with pytest.raises(ValueError, match="k = 2 values"):
        c.residuals(2, theta=[1.0])
    with pytest.raises(ValueError, match="finite"):
        c.residuals(2, theta=[1.0, np.nan])
    with pytest.raises(ValueError, match="finite"):
        c.residual_to_phi(0, np.inf)
    with pytest.raises(AssertionError, match="reached the library"):
        c.residuals(2, theta=[1.0, 2.0])
    with pytest.raises(AssertionError, match="reached the library"):
        c.residual_to_phi(0, 1.5)


def test_batch_arguments_are_checked_before_the_library(wa):
    import inspect
    b = object.__new__(wa.Batch)
    b.members = [wa.Params(16, 16, 16, dn=0.2, dt=0.004, max_states=2), wa.Params(16, 16, 16, dn=0.2, dt=0.002, max_states=3)]
    b._L, b._h = _NoDevice(), None
    p = inspect.signature(wa.Batch.residuals).parameters
    assert list(p) == ["self", "k", "theta", "active", "source"] and p["source"].default == "states"
    assert callable(wa.Batch.residual_counts)
    with pytest.raises(ValueError, match="one entry per member"):
        b.residuals(2, active=[1, 0, 1])
    for k in (0, 9, -1, [2, 0], [9, 2]):
        with pytest.raises(ValueError, match="RITZ_MAX"):
            b.residuals(k)
    with pytest.raises(ValueError, match="max_states"):
        b.residuals(3)
    with pytest.raises(ValueError, match="one entry per member"):
        b.residuals([2, 2, 2])
    with pytest.raises(ValueError, match="one entry per member"):
        b.residuals(2, theta=[[1.0, 2.0]])
    with pytest.raises(ValueError, match="no theta"):
        b.residuals(2, theta=[[1.0, 2.0], None])
    with pytest.raises(ValueError, match="k = 2 values"):
        b.residuals(2, theta=[[1.0, 2.0], [1.0]])
    with pytest.raises(ValueError, match="finite"):
        b.residuals(2, theta=[[1.0, 2.0], [1.0, np.inf]])
    with pytest.raises(ValueError, match="source"):
        b.residuals(2, source="store")
    with pytest.raises(ValueError, match="k = 1"):
        b.residuals(2, source="phi")
    with pytest.raises(ValueError, match="one entry per member"):
        b.residuals([1], source="phi")
    # members that are not listed are not checked, and the phi source does not look at max_states
    with pytest.raises(AssertionError, match="reached the library"):
        b.residuals([9, 3], theta=[None, [1.0, 2.0, 3.0]], active=[0, 1])
    with pytest.raises(AssertionError, match="reached the library"):
        b.residuals(source="phi")


# ---- driver and sweep -------------------------------------------------------------------------------------------------------------------------
def with_key(tmp_path, value):
    text = open(CASE).read()
    assert "gpu:" not in text
    p = tmp_path / f"residual_{value}.yaml"
    p.write_text(text + f"gpu:\n    residual: {value}\n")
    return str(p)


def test_check_config_echoes_the_key(wa, tmp_path):
    from wafer_amd import build
    for path, want in ((CASE, False), (with_key(tmp_path, "true"), True), (with_key(tmp_path, "false"), False)):
        r = subprocess.run([build.CLI, "-c", path, "--check-config"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        assert json.loads(r.stdout)["residual"] is want
    r = subprocess.run([build.CLI, "-c", with_key(tmp_path, "maybe"), "--check-config"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "gpu.residual" in r.stderr


def test_residuals_flag_leaves_the_plan_alone():
    out = []
    for extra in ([], ["--residuals"]):
        r = subprocess.run([sys.executable, "-m", "wafer_amd.sweep", "--plan", *extra, "-c", CASE, "-c", CASE], capture_output=True, text=True,
                           cwd=ROOT, timeout=120)
        assert r.returncode == 0, r.stderr
        out.append(r.stdout)
    assert out[0] == out[1] and "batches" in json.loads(out[0])


def test_sweep_and_run_refuse_the_key(tmp_path):
    path = with_key(tmp_path, "true")
    for module, extra in (("wafer_amd.sweep", ["--plan"]), ("wafer_amd.run", [])):
        r = subprocess.run([sys.executable, "-m", module, "-c", path, *extra], capture_output=True, text=True, cwd=ROOT, timeout=120)
        assert r.returncode != 0 and "gpu.residual" in r.stderr and len(r.stderr.strip().splitlines()) == 1, (module, r.stderr)
    r = subprocess.run([sys.executable, "-m", "wafer_amd.sweep", "-c", with_key(tmp_path, "false"), "--plan"], capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
