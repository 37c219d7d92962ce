"""Rayleigh-Ritz on the stored states, the parts that need no GPU: the numpy model of the sums against the oracle's observables,
the host solver wafer_ritz_solve (wafer_amd/csrc/wafer_ritz.h) against numpy.linalg.eigh, and the four entry points' ABI.

The solver is judged by invariants -- eigenvectors inside a degenerate block are not unique: eigenvalues ascending and within
1e-12 |A|_F of numpy's, C^T B C = I and C^T A C = diag(evals) to 1e-12 (the latter times |A|_F), and the sign rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import ritz_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wafer_ritz_solve", "wafer_ritz_matrices", "wafer_rotate_states", "wafer_ritz"]


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    from wafer_amd import build
    if not os.path.exists(build.LIB):
        build.build()
    wafer_amd.load_library()
    return wafer_amd


# ---- C1: the model's diagonal is the oracle's energy and norm2 ---------------------------------------------------------------------
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_model_diagonal_is_the_oracles_energy(oracle, ext):
    cfg = oracle.Config(9, 7, 5, ext=ext, potential="Harmonic", dn=0.2, dt=0.004, mass=1.3)
    v = oracle.potential_generate(cfg)
    states = rm.random_states(cfg.work_shape, ext, 3, seed=10 + ext)
    h, s = rm.matrices(cfg, v, states)
    for j, l in enumerate(states):
        want = oracle.observables(cfg, v, l)
        assert abs(h[j, j] - want["energy"]) <= 1e-12 * abs(want["energy"]), (ext, j, h[j, j], want["energy"])
        assert abs(s[j, j] - want["norm2"]) <= 1e-12 * abs(want["norm2"]), (ext, j)
    assert np.array_equal(s, s.T)                       # a product commutes; h is symmetric only up to the frame's part
    assert not np.array_equal(h, np.diag(np.diag(h)))


def test_model_h_is_symmetric_inside_a_zero_frame(oracle):
    """with zero frames the stencil is a symmetric matrix, so h[j, i] and h[i, j] differ by rounding only"""
    cfg = oracle.Config(9, 7, 5, ext=2, potential="Coulomb", dn=0.2, dt=0.004, mass=0.7)
    v = oracle.potential_generate(cfg)
    h, _, ah, _ = rm.matrices(cfg, v, rm.random_states(cfg.work_shape, 2, 4, seed=3, frame=False), scales=True)
    assert np.all(np.abs(h - h.T) <= 1e-12 * ah)


# ---- C2: the solver ----------------------------------------------------------------------------------------------------------------
def reduced_eigenvalues(a, b):
    l = np.linalg.cholesky(b)
    x = np.linalg.solve(l, a)
    at = np.linalg.solve(l, x.T).T
    return np.linalg.eigvalsh(0.5 * (at + at.T))


def check_solution(h, s, evals, coef):
    k = len(h)
    a, b = 0.5 * (h + h.T), 0.5 * (s + s.T)
    fro = np.linalg.norm(a)
    assert evals.shape == (k,) and coef.shape == (k, k)
    assert np.all(np.diff(evals) >= 0.0), evals
    assert np.max(np.abs(evals - reduced_eigenvalues(a, b))) <= 1e-12 * fro
    assert np.max(np.abs(coef.T @ b @ coef - np.eye(k))) <= 1e-12
    assert np.max(np.abs(coef.T @ a @ coef - np.diag(evals))) <= 1e-12 * fro
    for col in coef.T:                                   # the component of largest magnitude (lowest index on ties) is positive
        assert col[int(np.argmax(np.abs(col)))] > 0.0, col


def random_problem(k, seed):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((k, k))
    s = np.eye(k) + 0.5 * (m @ m.T) / k                 # symmetric positive definite, condition number of a few
    s = s + 1e-13 * rng.standard_normal((k, k))         # ... and as unsymmetric as rounded sums are
    h = rng.standard_normal((k, k)) * 3.0
    return h, s


@pytest.mark.parametrize("k", range(1, 9))
def test_solver_against_numpy(wa, k):
    for seed in range(5):
        h, s = random_problem(k, 100 * k + seed)
        evals, coef = wa.ritz_solve(h, s)
        check_solution(h, s, evals, coef)


def threefold(scaled):
    """k = 5, eigenvalues {2, 2, 2, 7, 12} exactly: A0 = 2 I + a a^T + b b^T with orthogonal integer a, b (|a|^2 = 5, |b|^2 = 10);
    scaled: B = D^2 with powers of two on D's diagonal and A = D A0 D, the same eigenvalues, every entry still exact"""
    a, b = np.array([1., 2., 0., 0., 0.]), np.array([2., -1., 1., 2., 0.])
    assert a @ b == 0.0
    a0 = 2.0 * np.eye(5) + np.outer(a, a) + np.outer(b, b)
    d = np.diag([2.0, 1.0, 0.5, 1.0, 4.0]) if scaled else np.eye(5)
    return d @ a0 @ d, d @ d


@pytest.mark.parametrize("scaled", [False, True])
def test_solver_on_a_threefold_eigenvalue(wa, scaled):
    h, s = threefold(scaled)
    evals, coef = wa.ritz_solve(h, s)
    check_solution(h, s, evals, coef)
    assert np.max(np.abs(evals - np.array([2., 2., 2., 7., 12.]))) <= 1e-12 * np.linalg.norm(h)


def test_solver_orders_exact_ties_by_index(wa):
    """a diagonal problem needs no rotation: equal entries keep their order, and coef is the permutation"""
    h = np.diag([3.0, 1.0, 3.0, 1.0])
    evals, coef = wa.ritz_solve(h, np.eye(4))
    assert evals.tolist() == [1.0, 1.0, 3.0, 3.0]
    assert np.array_equal(coef, np.eye(4)[:, [1, 3, 0, 2]])


# ---- C3: refusals, and nothing written ---------------------------------------------------------------------------------------------
def raw_solve(wa, k, h, s):
    """wafer_ritz_solve on sentinel-filled outputs -> (rc, evals, coef)"""
    L = wa.load_library()
    dp = C.POINTER(C.c_double)
    evals, coef = np.full(8, -77.0), np.full(64, -77.0)
    rc = L.wafer_ritz_solve(k, h.ctypes.data_as(dp), s.ctypes.data_as(dp), evals.ctypes.data_as(dp), coef.ctypes.data_as(dp))
    return rc, evals, coef


def test_solver_refusals_leave_the_outputs_alone(wa):
    from wafer_amd.engine import WAFER_ERR_INVALID, WAFER_ERR_STATE
    ones = np.ones((3, 3))
    nan_s, nan_h = np.eye(3), np.eye(3)
    nan_s[1, 1] = np.nan
    nan_h[0, 2] = np.nan
    big = np.eye(9)
    cases = [(3, np.eye(3), ones, WAFER_ERR_STATE),                              # singular: three equal states
             (2, np.eye(2), np.array([[1.0, 2.0], [2.0, 1.0]]), WAFER_ERR_STATE),  # indefinite
             (3, np.eye(3), nan_s, WAFER_ERR_STATE), (3, nan_h, np.eye(3), WAFER_ERR_STATE),
             (3, np.eye(3), np.diag([1.0, 1.0, np.inf]), WAFER_ERR_STATE),
             (0, big, big, WAFER_ERR_INVALID), (9, big, big, WAFER_ERR_INVALID)]
    for k, h, s, code in cases:
        rc, evals, coef = raw_solve(wa, k, np.ascontiguousarray(h), np.ascontiguousarray(s))
        assert rc == code, (k, rc, code)
        assert np.all(evals == -77.0) and np.all(coef == -77.0), k
    with pytest.raises(wa.WaferError) as e:
        wa.ritz_solve(np.eye(3), ones)
    assert e.value.code == WAFER_ERR_STATE
    with pytest.raises(wa.WaferError) as e:
        wa.ritz_solve(big, big)
    assert e.value.code == WAFER_ERR_INVALID


# ---- C4: the ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_four_entry_points_agree_across_header_ctypes_and_rust(wa):
    import wafer_amd.engine as eng
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wafer_hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert re.search(r"#define\s+WAFER_RITZ_MAX\s+8\b", header) and eng.RITZ_MAX == 8
    L = wa.load_library()
    assert L.wafer_abi_version() == 1
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        arity = m.group(1).count(",") + 1
        assert name in eng.EXPORTS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == arity, name
        r = re.search(r"pub fn %s\s*\((.*?)\)\s*->\s*c_int" % name, rust, flags=re.S)
        assert r and len([a for a in r.group(1).split(",") if a.strip()]) == arity, name
