"""Moment matrices of the stored states, the parts that need no GPU: the numpy model of tests/moments_model.py against the oracle's
observables (per cell, ==, and exact integer sums), that the model tells the two origin conventions apart, the three entry points'
ABI, the argument checks of Context and Batch before any library call, and the driver's and the sweep's handling of `gpu.moments`
/ --moments."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import moments_model as mm
from tests import ritz_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "golden", "cli_case.yaml")
CALLS = {"wafer_moment_matrices": 3, "wafer_batch_moment_matrices": 4, "wafer_batch_diag_moment_counts": 3}
CONSTANTS = {"WAFER_MOMENT_S": 0, "WAFER_MOMENT_X": 1, "WAFER_MOMENT_Y": 2, "WAFER_MOMENT_Z": 3, "WAFER_MOMENT_R2": 4, "WAFER_MOMENT_COUNT": 5}
SHAPES = [(12, 10, 9), (17, 17, 17), (3, 2, 5)]


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    from wafer_amd import build
    if not os.path.exists(build.LIB):
        build.build()
    wafer_amd.load_library()
    return wafer_amd


def config_of(oracle, shape, ext):
    return oracle.Config(*shape, ext=ext, potential="Harmonic", dn=0.2, dt=0.004, mass=1.3)


# ---- the model against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_diagonal_terms_are_the_oracles_cells(oracle, shape, ext):
    """per cell, before any sum: the R2 and S terms of entry (j, j) are compute_observables' r2 and norm2 terms, bit for bit"""
    cfg = config_of(oracle, shape, ext)
    v = oracle.potential_generate(cfg)
    for l in rm.random_states(shape, ext, 2, seed=70 + ext + sum(shape)):
        want = oracle.observables_cells(cfg, v, l)
        s, _, _, _, r2 = mm.terms(shape, ext, l, l)
        assert s.shape == shape
        assert np.array_equal(s, want["norm2"])
        assert np.array_equal(r2, want["r2"])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_integer_states_sum_exactly_to_the_oracles_observables(oracle, shape, ext):
    """entries in -3 .. 3: every product and every sum is exact, so no order of summation can differ"""
    cfg = config_of(oracle, shape, ext)
    v = oracle.potential_generate(cfg)
    states = mm.integer_states(shape, ext, 3, seed=5 + ext)
    m = mm.matrices(shape, ext, states)
    for j, l in enumerate(states):
        want = oracle.observables(cfg, v, l)
        assert m["r2"][j, j] == want["r2"], (j, m["r2"][j, j], want["r2"])
        assert m["s"][j, j] == want["norm2"], j
    for name in mm.NAMES:
        assert np.array_equal(m[name], m[name].T)
        assert np.all(m[name] * 4.0 == np.round(m[name] * 4.0))       # quarters at the finest: nothing was rounded


def test_the_model_tells_the_two_origins_apart(oracle):
    """the origin is (n + 1) / 2, one cell above the geometric centre (n - 1) / 2: on the same input the geometric centre gives
    another r2 and other dipole entries, and only the former is the oracle's"""
    shape, ext = (12, 10, 9), 1
    cfg = config_of(oracle, shape, ext)
    states = mm.integer_states(shape, ext, 2, seed=11)
    ours = mm.matrices(shape, ext, states)
    centred = mm.matrices(shape, ext, states, origin=tuple((n - 1.) / 2. for n in shape))
    want = oracle.observables(cfg, oracle.potential_generate(cfg), states[0])["r2"]
    assert ours["r2"][0, 0] == want and centred["r2"][0, 0] != want
    assert mm.centres(shape) == (6.5, 5.5, 5.0)
    assert np.array_equal(ours["s"], centred["s"])
    for name, axis in (("x", 0), ("y", 1), ("z", 2)):
        # moving the origin by one cell moves the dipole matrix by S (exact on integers): <i|x - c|j> = X_ij - c S_ij
        assert np.array_equal(centred[name], ours[name] + ours["s"]), name
        assert not np.array_equal(centred[name], ours[name])
    # each axis has its own offset: a state that is one cell gives that cell's dx, dy, dz
    one = np.zeros(tuple(n + 2 * ext for n in shape))
    one[ext + 2, ext + 7, ext + 4] = 1.0
    m = mm.matrices(shape, ext, [one])
    assert (m["x"][0, 0], m["y"][0, 0], m["z"][0, 0]) == (2 - 6.5, 7 - 5.5, 4 - 5.0)
    assert m["r2"][0, 0] == 4.5 * 4.5 + 1.5 * 1.5 + 1.0


def test_scales_bound_the_entries():
    shape, ext = (3, 2, 5), 2
    m, a = mm.matrices(shape, ext, rm.random_states(shape, ext, 3, seed=2), scales=True)
    for name in mm.NAMES:
        assert m[name].shape == (3, 3) and np.all(np.abs(m[name]) <= a[name]) and np.all(a[name] > 0.0)


# ---- ABI and bindings ------------------------------------------------------------------------------------------------------------------------
def test_the_three_calls_are_declared_exported_bound_and_mirrored(wa):
    import wafer_amd.engine as eng
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wafer_hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    L = wa.load_library()
    for name, value in CONSTANTS.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
        assert re.search(r"pub const %s: usize = %d;" % (name, value), rust), name
    assert eng.MOMENT_NAMES == ("s", "x", "y", "z", "r2") and eng.MOMENT_COUNT == 5
    assert eng.moment_origin(12, 10, 9) == mm.centres((12, 10, 9))
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
    d = np.zeros(5 * 64)
    dp = d.ctypes.data_as(C.POINTER(C.c_double))
    k = (C.c_uint32 * 1)(1)
    n = C.c_uint64(0)
    assert L.wafer_moment_matrices(None, 1, dp) == WAFER_ERR_INVALID
    assert "null" in L.wafer_last_error().decode()
    assert L.wafer_batch_moment_matrices(None, None, k, dp) == WAFER_ERR_INVALID
    assert L.wafer_batch_diag_moment_counts(None, C.byref(n), C.byref(n)) == WAFER_ERR_INVALID
    assert "null" in L.wafer_last_error().decode()
    assert np.all(d == 0.0)


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError("argument check missing: %s reached the library" % name)


def test_batch_arguments_are_checked_before_the_library(wa):
    import inspect
    b = object.__new__(wa.Batch)
    b.members = [wa.Params(16, 16, 16, dn=0.2, dt=0.004, max_states=2), wa.Params(16, 16, 16, dn=0.2, dt=0.002, max_states=3)]
    b._L, b._h = _NoDevice(), None
    assert list(inspect.signature(wa.Batch.moments).parameters) == ["self", "k", "active"]
    assert list(inspect.signature(wa.Context.moments).parameters) == ["self", "k"]
    assert callable(wa.Batch.moment_counts)
    with pytest.raises(ValueError, match="one entry per member"):
        b.moments(2, active=[1, 0, 1])
    for k in (0, 9, -1, [2, 0], [9, 2]):
        with pytest.raises(ValueError, match="RITZ_MAX"):
            b.moments(k)
    with pytest.raises(ValueError, match="max_states"):
        b.moments(3)
    with pytest.raises(AssertionError, match="reached the library"):
        b.moments([9, 3], active=[0, 1])                       # members that are not listed are not checked


# ---- driver and sweep -------------------------------------------------------------------------------------------------------------------------
def with_key(tmp_path, value):
    text = open(CASE).read()
    assert "gpu:" not in text
    p = tmp_path / f"moments_{value}.yaml"
    p.write_text(text + f"gpu:\n    moments: {value}\n")
    return str(p)


def test_check_config_echoes_the_key(wa, tmp_path):
    from wafer_amd import build
    for path, want in ((CASE, False), (with_key(tmp_path, "true"), True), (with_key(tmp_path, "false"), False)):
        r = subprocess.run([build.CLI, "-c", path, "--check-config"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        assert json.loads(r.stdout)["moments"] is want
    r = subprocess.run([build.CLI, "-c", with_key(tmp_path, "maybe"), "--check-config"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "gpu.moments" in r.stderr


def test_moments_flag_leaves_the_plan_alone():
    out = []
    for extra in ([], ["--moments"]):
        r = subprocess.run([sys.executable, "-m", "wafer_amd.sweep", "--plan", *extra, "-c", CASE, "-c", CASE], capture_output=True, text=True,
                           cwd=ROOT, timeout=120)
        assert r.returncode == 0, r.stderr
        out.append(r.stdout)
    assert out[0] == out[1] and "batches" in json.loads(out[0])


def test_sweep_and_run_refuse_the_key(tmp_path):
    path = with_key(tmp_path, "true")
    for module, extra in (("wafer_amd.sweep", ["--plan"]), ("wafer_amd.run", [])):
        r = subprocess.run([sys.executable, "-m", module, "-c", path, *extra], capture_output=True, text=True, cwd=ROOT, timeout=120)
        assert r.returncode != 0 and "gpu.moments" in r.stderr and len(r.stderr.strip().splitlines()) == 1, (module, r.stderr)
    r = subprocess.run([sys.executable, "-m", "wafer_amd.sweep", "-c", with_key(tmp_path, "false"), "--plan"], capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([sys.executable, "-m", "wafer_amd.sweep", "-c", CASE, "--plan"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr                         # a file without the key
