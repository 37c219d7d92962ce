"""Chebyshev-filtered subspace iteration, the parts that need no GPU: wafer_filter_coefficients against the model on the bits, the
launch plan of a call (wafer_amd/csrc/wafer_batch_plan.h, compiled with g++ and the sanitizers), the new entry points' ABI, and
wafer_amd.engine.filtered_solve_loop on the numpy backend of tests/filter_model.py against a dense numpy.linalg.eigh of H.

Why the filter: the plain block solver's fixed points are not H's eigenvectors (tests/test_store_step_host.py pins its rho floor), so
with V = 200 r^2 on 9^3 it settles 1.4e-4 (relative) away from H's lowest level.  The filter is a polynomial in H: its Ritz values
meet eigh's to 1e-9 and rho falls below 1e-10 -- both asserted in test_the_filter_finds_eigenvalues_of_h, next to the plain
solver's miss.

Block counts, measured with this file's model on the CPU (k = 5, guard 1, degree 30, tolerance 1e-10, N(0, 1) starts, seed 20):
ThreePoint 9^3 free 5, harmonic 4; FivePoint 5^3 free 3, harmonic 3; SevenPoint 7^3 free 5, harmonic 4."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import filter_model as fm
from tests import store_step_model as ssm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wafer_amd", "csrc")
CALLS = {"wafer_filter_coefficients": 7, "wafer_filter_states": 6, "wafer_spectral_bound": 2, "wafer_batch_filter_states": 7,
         "wafer_batch_spectral_bound": 3, "wafer_batch_diag_filter_counts": 3}
DN = 0.1
# (ext, shape): 9^3 for ThreePoint; for the wider stencils the smallest cubes whose work area is wider than the stencil (2 ext + 1)
GRIDS = {1: (9, 9, 9), 2: (5, 5, 5), 3: (7, 7, 7)}
BLOCKS = {(1, "free"): 5, (1, "harmonic"): 4, (2, "free"): 3, (2, "harmonic"): 3, (3, "free"): 5, (3, "harmonic"): 4}
INTERVALS = [(1.0, 10.0, 0.5), (52.07, 696.0, 30.56), (-0.1, 37.5, -0.5), (-2.0, -1.0, -13.6), (1e-3, 1e6, 1e-4)]   # (a, b, a0)


@pytest.fixture(scope="module")
def lib():
    import wafer_amd
    from wafer_amd import build
    if not os.path.exists(build.LIB):
        build.build()
    return wafer_amd.load_library()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the coefficients ------------------------------------------------------------------------------------------------------------------
def raw(lib, degree, a, b, a0, n=None):
    """wafer_filter_coefficients on sentinel-filled outputs -> (rc, al, be, cc)"""
    dp = C.POINTER(C.c_double)
    n = max(degree, 1) if n is None else n
    al, be, cc = np.full(n, -77.0), np.full(n, -77.0), np.full(1, -77.0)
    rc = lib.wafer_filter_coefficients(degree, a, b, a0, al.ctypes.data_as(dp), be.ctypes.data_as(dp), cc.ctypes.data_as(dp))
    return rc, al, be, cc


@pytest.mark.parametrize("degree", [1, 2, 3, 17])
def test_coefficients_have_the_models_bits(lib, degree):
    from wafer_amd.engine import filter_coefficients
    for a, b, a0 in INTERVALS:
        want = fm.coefficients(degree, a, b, a0)
        rc, al, be, cc = raw(lib, degree, a, b, a0)
        assert rc == 0
        assert np.array_equal(bits(al), bits(want[0])), (degree, a, b, a0, al, want[0])
        assert np.array_equal(bits(be), bits(want[1])), (degree, a, b, a0, be, want[1])
        assert bits(cc)[0] == bits(np.float64(want[2])), (degree, a, b, a0)
        assert be[0] == 0.0 and np.all(np.isfinite(al)) and np.all(np.isfinite(be))
        got = filter_coefficients(degree, a, b, a0)
        assert np.array_equal(bits(got[0]), bits(al)) and np.array_equal(bits(got[1]), bits(be)) and got[2] == cc[0]


def test_the_polynomial_is_one_at_the_anchor_and_small_on_the_interval(lib):
    """the recurrence with H a number x, on the coefficients wafer_filter_coefficients gives: magnitude 1 at a0, at most
    1 / |T_m(xi(a0))| on [a, b], growing below a0"""
    a, b, a0, degree = 52.0, 700.0, 30.0, 17
    rc, al, be, cc = raw(lib, degree, a, b, a0)
    assert rc == 0
    cc = float(cc[0])

    def p(x):
        prev, cur = None, 1.0
        for i in range(degree):
            y = al[i] * (x - cc) * cur - (be[i] * prev if i else 0.0)
            prev, cur = cur, y
        return cur

    assert abs(abs(p(a0)) - 1.0) < 1e-12
    # p(x) = T_m(xi(x)) / T_m(xi(a0)) with xi = (x - cc) / e: |T_m| <= 1 on [a, b], and T_m(xi0) = cosh(m arccosh |xi0|) outside
    peak = 1.0 / np.cosh(degree * np.arccosh(abs(a0 - cc) / ((b - a) / 2.0)))
    assert peak < 0.01
    assert max(abs(p(x)) for x in np.linspace(a, b, 501)) <= peak * (1.0 + 1e-9)
    assert abs(p(a0 - 5.0)) > 1.0


def test_coefficient_refusals_write_nothing(lib):
    from wafer_amd.engine import FILTER_MAX_DEGREE, WAFER_ERR_INVALID
    inf, nan = float("inf"), float("nan")
    cases = [(0, 1.0, 2.0, 0.5), (FILTER_MAX_DEGREE + 1, 1.0, 2.0, 0.5),
             (3, 1.0, 2.0, 1.0), (3, 1.0, 2.0, 1.5), (3, 2.0, 2.0, 0.5), (3, 3.0, 2.0, 0.5),        # a0 < a < b violated
             (3, nan, 2.0, 0.5), (3, 1.0, nan, 0.5), (3, 1.0, 2.0, nan), (3, 1.0, inf, 0.5), (3, 1.0, 2.0, -inf), (3, -inf, 2.0, -inf)]
    for degree, a, b, a0 in cases:
        rc, al, be, cc = raw(lib, degree, a, b, a0, n=4)
        assert rc == WAFER_ERR_INVALID, (degree, a, b, a0, rc)
        assert np.all(al == -77.0) and np.all(be == -77.0) and cc[0] == -77.0
    assert raw(lib, FILTER_MAX_DEGREE, 1.0, 2.0, 0.5)[0] == 0
    assert lib.wafer_filter_coefficients(2, 1.0, 2.0, 0.5, None, None, None) == WAFER_ERR_INVALID


# ---- header, library, bindings ----------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_in_the_header_the_library_and_the_bindings(lib):
    import wafer_amd
    import wafer_amd.engine as eng
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wafer_hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name, nargs in CALLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m and m.group(1).count(",") + 1 == nargs, name
        assert hasattr(lib, name) and name in eng.EXPORTS
        assert len(getattr(lib, name).argtypes) == nargs
        r = re.search(r"pub fn %s\s*\((.*?)\)\s*->" % name, rust, flags=re.S)
        assert r and len([a for a in r.group(1).split(",") if a.strip()]) == nargs, name
    assert re.search(r"#define\s+WAFER_FILTER_MAX_DEGREE\s+%d\b" % eng.FILTER_MAX_DEGREE, header)
    for cls, names in ((wafer_amd.Context, ("filter_states", "spectral_bound", "solve_filtered")),
                       (wafer_amd.Batch, ("filter_states", "spectral_bound", "solve_filtered", "filter_counts"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    assert wafer_amd.filtered_solve_loop is eng.filtered_solve_loop


# ---- the plan of a call ------------------------------------------------------------------------------------------------------------------
DRIVER = r"""
#include "wafer_batch_plan.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const uint32_t degree = (uint32_t)atoi(argv[1]), max_k = (uint32_t)atoi(argv[2]);
    const WaferBatchFilterPlan p = wafer_batch_filter_plan(degree, max_k);
    printf("%llu %llu %d %d :", (unsigned long long)p.steps, (unsigned long long)p.launches, p.groups, p.copy_back ? 1 : 0);
    for (uint64_t i = 1; i <= p.steps && i <= 16; ++i) printf(" %d", wafer_batch_filter_src_is_shadow(i) ? 1 : 0);
    printf("\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("filter_plan")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(DRIVER)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I", CSRC,
                        str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

    def call(*args):
        out = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (args, out.stderr[-2000:])
        return out.stdout
    return call


def test_filter_plan(plan):
    """degree steps are degree launches, or degree + 1 with the trailing copy when it is odd; the result always ends in the slots"""
    for degree in list(range(1, 12)) + [30, 255, 256]:
        for max_k in range(0, 9):
            head, _, tail = plan(degree, max_k).partition(":")
            n, launches, groups, copy_back = [int(x) for x in head.split()]
            src = [int(x) for x in tail.split()]
            assert n == degree and groups == (max_k + 3) // 4
            if max_k == 0:
                assert launches == 0 and copy_back == 0   # nobody listed with k > 0: nothing is launched
                continue
            assert copy_back == n % 2 and launches == n + copy_back
            # step 1 reads the slots (0) and writes the shadows; step i reads what step i - 1 wrote and writes over step i - 2's
            assert src == [(i + 1) % 2 for i in range(1, min(n, 16) + 1)]
            # the last step writes the set it does not read: the shadows iff the degree is odd -- exactly when the copy runs
            assert (src[-1] == 0) == bool(copy_back) or n > 16


# ---- the solver on the numpy backend against eigh ----------------------------------------------------------------------------------------
def potential(kind, shape, ext):
    return np.zeros(tuple(n + 2 * ext for n in shape)) if kind == "free" else fm.harmonic_v(shape, ext, DN)


@pytest.mark.parametrize("kind", ["free", "harmonic"])
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_the_filter_finds_eigenvalues_of_h(oracle, ext, kind):
    from wafer_amd.engine import BLOCK_CONVERGED, FILTER_CONVERGED
    shape = GRIDS[ext]
    cfg, v = fm.Cfg(ext, DN), potential(kind, shape, ext)
    H = fm.dense_h(cfg, v, shape)
    assert H.shape == (int(np.prod(shape)),) * 2 and np.array_equal(H, H.T)
    exact = np.linalg.eigvalsh(H)
    ub = fm.bound(cfg, v)
    assert exact[-1] <= ub <= 1.2 * exact[-1]                       # Gershgorin holds, and is not wasteful
    r = fm.solve_filtered([fm.Member(cfg, v, fm.start_states(shape, ext))])[0]
    print(ext, kind, r["status"], r["blocks"], r["evals"], exact[:5], r["rho"])
    assert r["status"] == FILTER_CONVERGED and r["message"] == ""
    assert r["blocks"] == BLOCKS[ext, kind] and r["steps"] == r["blocks"] * fm.DEGREE
    n = fm.K - fm.GUARD
    assert np.all(np.abs(r["evals"][:n] - exact[:n]) <= 1e-9 * np.abs(exact[:n])), (r["evals"], exact[:fm.K])
    assert np.all(r["rho"][:n] < 1e-10), r["rho"]
    assert r["rho"][n] > 1e-6                                       # the guard state is not waited for
    # one row per block: block, steps, evals, diff, rho; diff is against the Ritz step on the starts in the first block
    assert [row["block"] for row in r["rows"]] == list(range(1, r["blocks"] + 1))
    assert [row["steps"] for row in r["rows"]] == [fm.DEGREE * b for b in range(1, r["blocks"] + 1)]
    assert all(row["evals"].shape == (fm.K,) and row["rho"].shape == (fm.K,) and np.all(np.isfinite(row["diff"])) for row in r["rows"])
    if ext == 1 and kind == "harmonic":
        # the reason for the feature: the plain block solver converges, by its own rule, to something that is not H's level
        plain = ssm.solve_block([ssm.Member(oracle, shape, DN, ssm.harmonic_v(shape, 1, DN), ssm.start_states())])[0]
        assert plain["status"] == BLOCK_CONVERGED
        assert np.array_equal(ssm.harmonic_v(shape, 1, DN), v)
        print(plain["evals"][0], r["evals"][0], exact[0])
        assert abs(plain["evals"][0] - exact[0]) > 1e-6 * exact[0]
        assert abs(r["evals"][0] - exact[0]) <= 1e-9 * exact[0]
        assert abs(exact[0] - 30.56147647) <= 1e-8


# ---- the loop's statuses ---------------------------------------------------------------------------------------------------------------------
def scripted(evals_by_block, rho_by_block, ub=100.0):
    """a backend whose Ritz values and rho are read from lists: block 0 is the Ritz step on the starts"""
    calls, block = [], {"n": 0}

    def bound(going):
        calls.append(("bound", tuple(going)))
        return {m: ub for m in going}

    def filt(going, n, iv):
        block["n"] += 1
        calls.append(("filter", tuple(going), n, dict(iv)))

    def ritz(going):
        calls.append(("ritz", tuple(going)))
        return {m: evals_by_block[m][block["n"]] for m in going}

    def residuals(going, theta):
        calls.append(("rho", tuple(going)))
        return {m: rho_by_block[m][block["n"]] for m in going}

    return calls, bound, filt, ritz, residuals


def test_statuses_are_not_exceptions_and_done_members_leave():
    from wafer_amd.engine import (FILTER_CONVERGED, FILTER_DEPENDENT, FILTER_MAX_BLOCKS, FILTER_NO_INTERVAL, WAFER_ERR_STATE, WAFER_OK,
                                  filtered_solve_loop)
    ok = lambda *e: (WAFER_OK, list(e))   # noqa: E731
    evals = {0: [ok(5.0, 9.0), ok(4.0, 8.0), ok(4.0, 8.0), ok(4.0, 8.0)],            # converges in block 2
             1: [ok(5.0, 9.0), ok(4.0, 8.0), ok(4.0, 8.0), ok(4.0, 8.0)],            # never does
             2: [ok(5.0, 9.0), (WAFER_ERR_STATE, None)],                             # Ritz fails after the first filter
             3: [ok(5.0, 5.0)],                                                      # no interval: evals[k - 1] <= evals[0]
             4: [ok(5.0, 100.0)],                                                    # no interval: evals[k - 1] >= ub
             5: [(WAFER_ERR_STATE, None)]}                                           # dependent starts
    rho = {0: [None, [0.5, 0.5], [1e-12, 0.5]], 1: [None, [0.5, 0.5], [0.4, 1e-12], [0.3, 1e-12]]}
    calls, bound, filt, ritz, residuals = scripted(evals, rho)
    r = filtered_solve_loop(bound, filt, ritz, residuals, [2, 2, 2, 2, 2, 2, 0, None], 1e-10, 7, 3)
    assert r[6] is None and r[7] is None
    assert r[0]["status"] == FILTER_CONVERGED and r[0]["blocks"] == 2 and r[0]["steps"] == 14 and r[0]["message"] == ""
    assert r[1]["status"] == FILTER_MAX_BLOCKS and r[1]["blocks"] == 3 and "max_blocks" in r[1]["message"]   # the guard state's rho does not count
    assert r[2]["status"] == FILTER_DEPENDENT and r[2]["blocks"] == 1 and "lower degree" in r[2]["message"] and "member 2" in r[2]["message"]
    assert r[3]["status"] == FILTER_NO_INTERVAL and r[3]["blocks"] == 0 and "evals[0]" in r[3]["message"]
    assert r[4]["status"] == FILTER_NO_INTERVAL and r[4]["blocks"] == 0 and "spectral bound" in r[4]["message"]
    assert r[5]["status"] == FILTER_DEPENDENT and r[5]["blocks"] == 0 and r[5]["rows"] == []
    filters = [c for c in calls if c[0] == "filter"]
    assert [c[1] for c in filters] == [(0, 1, 2), (0, 1), (1,)]
    assert all(c[2] == 7 for c in filters)
    assert filters[0][3][0] == (9.0, 100.0, 5.0) and filters[1][3][1] == (8.0, 100.0, 4.0)   # (a, b, a0) = (evals[k-1], ub, evals[0])
    assert calls[0] == ("bound", (0, 1, 2, 3, 4, 5)) and calls[1] == ("ritz", (0, 1, 2, 3, 4, 5))
    for bad in (dict(degree=0), dict(degree=257), dict(max_blocks=0), dict(tolerance=0.0), dict(guard=0), dict(guard=2)):
        kw = dict(tolerance=1e-10, degree=7, max_blocks=3, guard=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            filtered_solve_loop(bound, filt, ritz, residuals, [2], kw["tolerance"], kw["degree"], kw["max_blocks"], kw["guard"])
