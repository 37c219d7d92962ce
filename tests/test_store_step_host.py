"""Subspace iteration on the state stores, the parts that need no GPU: wafer_amd.engine.block_solve_loop driven by the numpy backend
of tests/store_step_model.py (the oracle's step, the Ritz and residual models), the loop's statuses, the new entry points' ABI and
the host-side plan of wafer_batch_evolve_states (wafer_amd/csrc/wafer_batch_plan.h, compiled with g++ and the sanitizers).

Why rho is reported and never decides: the semi-implicit step is P = 1 - dt (1 + dt V / 2)^-1 H, whose invariant subspaces are
those of H w = mu (1 + dt V / 2) w -- H's only where V is constant.  With V = 0 (case a) rho falls with the iteration; with
V = 200 r^2 (case b) the Ritz energies settle to 1e-10 while rho stops near 0.5 and 0.9."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import store_step_model as ssm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wafer_amd", "csrc")
CALLS = {"wafer_evolve_states": 3, "wafer_batch_evolve_states": 4, "wafer_batch_diag_store_step": 3, "wafer_batch_diag_store_counts": 2}
DN = 0.1


def free_member(oracle, dn=DN):
    return ssm.Member(oracle, ssm.SHAPE, dn, np.zeros(tuple(n + 2 for n in ssm.SHAPE)), ssm.start_states())


def harmonic_member(oracle, dn=DN):
    return ssm.Member(oracle, ssm.SHAPE, dn, ssm.harmonic_v(ssm.SHAPE, 1, dn), ssm.start_states())


# ---- (a), (b), (c): the loop on the numpy backend -------------------------------------------------------------------------------------
def test_free_box_converges_to_the_closed_form(oracle):
    from wafer_amd.engine import BLOCK_CONVERGED
    r = ssm.solve_block([free_member(oracle)])[0]
    exact = ssm.box_levels(DN)
    print(r["status"], r["blocks"], r["evals"], exact, r["diff"], r["rho"])
    assert r["status"] == BLOCK_CONVERGED and r["message"] == ""
    assert r["blocks"] <= ssm.MAX_BLOCKS and r["steps"] == r["blocks"] * ssm.STEPS_PER_BLOCK
    assert np.all(np.abs(r["evals"] - exact) <= 1e-9 * exact), (r["evals"], exact)
    assert np.all(r["rho"] <= 1e-4), r["rho"]
    assert np.max(r["diff"]) < ssm.TOLERANCE
    # one row per block: block, steps, evals, diff, rho; the first block has nothing to compare with
    assert [row["block"] for row in r["rows"]] == list(range(1, r["blocks"] + 1))
    assert [row["steps"] for row in r["rows"]] == [ssm.STEPS_PER_BLOCK * b for b in range(1, r["blocks"] + 1)]
    assert np.all(np.isinf(r["rows"][0]["diff"])) and all(np.all(np.isfinite(row["diff"])) for row in r["rows"][1:])
    assert all(row["evals"].shape == (ssm.K,) and row["rho"].shape == (ssm.K,) for row in r["rows"])
    # the shell (2,1,1) x 3 is resolved by construction: three equal levels, ascending
    assert np.all(np.diff(r["evals"]) >= -1e-9 * exact[1])


def test_harmonic_converges_but_rho_has_a_floor(oracle):
    """the pinned reason why rho is not the stopping rule"""
    from wafer_amd.engine import BLOCK_CONVERGED
    r = ssm.solve_block([harmonic_member(oracle)])[0]
    print(r["status"], r["blocks"], r["evals"], r["diff"], r["rho"])
    assert r["status"] == BLOCK_CONVERGED
    assert np.max(r["diff"]) < ssm.TOLERANCE
    assert np.all(r["rho"] > 0.1), r["rho"]
    assert abs(r["evals"][0] - 30.56590795) <= 1e-6 and np.all(np.abs(r["evals"][1:] - 52.09206265) <= 1e-6)


def test_a_block_that_is_too_long_is_a_status_not_an_exception(oracle):
    """20000 plain steps shrink every state by (1 - dt E)^20000 < 1e-380: the four arrays underflow to zero, S = 0 and the
    Cholesky factorisation fails whatever the rounding -- the member gets WAFER_ERR_STATE and the advice, the other goes on"""
    from wafer_amd.engine import BLOCK_DEPENDENT, block_solve_loop
    members = [free_member(oracle), free_member(oracle)]
    per_member = {0: 20000, 1: ssm.STEPS_PER_BLOCK}

    def step(going, n):
        for m in going:
            members[m].step(per_member[m])

    r = block_solve_loop(step, lambda going: {m: members[m].ritz() for m in going},
                         lambda going, theta: {m: members[m].rho(theta[m]) for m in going}, [ssm.K, ssm.K], ssm.TOLERANCE, ssm.STEPS_PER_BLOCK, 3)
    assert r[0]["status"] == BLOCK_DEPENDENT and r[0]["blocks"] == 1 and r[0]["rows"] == []
    assert "steps_per_block" in r[0]["message"] and "shorten" in r[0]["message"] and "member 0" in r[0]["message"]
    assert r[1]["blocks"] == 3 and len(r[1]["rows"]) == 3


def test_max_blocks_is_a_status_and_done_members_leave(oracle):
    from wafer_amd.engine import BLOCK_CONVERGED, BLOCK_MAX_BLOCKS, block_solve_loop
    r = ssm.solve_block([free_member(oracle)], max_blocks=2)[0]
    assert r["status"] == BLOCK_MAX_BLOCKS and r["blocks"] == 2 and "max_blocks" in r["message"]
    # a scripted backend: member 0's energies stop moving after block 2, member 1's never do; k = 0 and None take no part
    calls = []
    energy = {0: [5.0, 4.0, 4.0, 4.0], 1: [9.0, 8.0, 7.0, 6.0]}
    block = {"n": 0}

    def step(going, n):
        block["n"] += 1
        calls.append(("step", tuple(going), n))

    def ritz(going):
        calls.append(("ritz", tuple(going)))
        return {m: (0, [energy[m][block["n"] - 1]]) for m in going}

    def residuals(going, theta):
        calls.append(("rho", tuple(going)))
        assert all(theta[m][0] == energy[m][block["n"] - 1] for m in going)
        return {m: [0.5] for m in going}

    r = block_solve_loop(step, ritz, residuals, [1, 1, 0, None], 1e-3, 7, 4)
    assert r[2] is None and r[3] is None
    assert r[0]["status"] == BLOCK_CONVERGED and r[0]["blocks"] == 3 and r[0]["steps"] == 21
    assert r[1]["status"] == BLOCK_MAX_BLOCKS and r[1]["blocks"] == 4
    assert [c for c in calls if c[0] == "step"] == [("step", (0, 1), 7)] * 3 + [("step", (1,), 7)]
    assert calls[-2:] == [("ritz", (1,)), ("rho", (1,))]
    with pytest.raises(ValueError):
        block_solve_loop(step, ritz, residuals, [1], 1e-3, 0, 4)
    with pytest.raises(ValueError):
        block_solve_loop(step, ritz, residuals, [1], 0.0, 5, 4)


# ---- (d): header, library, bindings -----------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_in_the_header_the_library_and_the_bindings():
    import wafer_amd
    import wafer_amd.engine as eng
    from wafer_amd import build
    if not os.path.exists(build.LIB):
        build.build()
    lib = wafer_amd.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wafer_hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name, nargs in CALLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m and m.group(1).count(",") + 1 == nargs, name
        assert hasattr(lib, name) and name in eng.EXPORTS
        assert len(getattr(lib, name).argtypes) == nargs
        r = re.search(r"pub fn %s\s*\((.*?)\)\s*->" % name, rust, flags=re.S)
        assert r and len([a for a in r.group(1).split(",") if a.strip()]) == nargs, name
    for cls, names in ((wafer_amd.Context, ("evolve_states", "seed_states", "solve_block")),
                       (wafer_amd.Batch, ("evolve_states", "seed_states", "solve_block", "store_dispatch", "store_counts"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    assert wafer_amd.block_solve_loop is eng.block_solve_loop


# ---- the plan of a call ------------------------------------------------------------------------------------------------------------------
DRIVER = r"""
#include "wafer_batch_plan.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const uint64_t steps = strtoull(argv[1], nullptr, 10);
    const uint32_t max_k = (uint32_t)atoi(argv[2]);
    const WaferBatchStorePlan p = wafer_batch_store_plan(steps, max_k);
    printf("%llu %llu %d %d %d :", (unsigned long long)p.steps, (unsigned long long)p.launches, p.groups, p.copy_back ? 1 : 0, WAFER_STORE_SG);
    for (uint64_t s = 0; s < p.steps && s < 16; ++s) printf(" %d", wafer_batch_store_src_is_shadow(s) ? 1 : 0);
    printf("\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("store_plan")
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


def test_store_plan(plan):
    """n steps are n launches, or n + 1 with the trailing copy when n is odd; the results always end in the slots"""
    for steps in list(range(0, 12)) + [1000, 1001]:
        for max_k in range(0, 9):
            head, _, tail = plan(steps, max_k).partition(":")
            n, launches, groups, copy_back, sg = [int(x) for x in head.split()]
            src = [int(x) for x in tail.split()]
            assert n == max(steps, 1) and sg == 4
            assert groups == (max_k + sg - 1) // sg
            if max_k == 0:
                assert launches == 0 and copy_back == 0   # nobody listed with k > 0: nothing is launched
                continue
            assert copy_back == n % 2 and launches == n + copy_back
            assert src == [s % 2 for s in range(min(n, 16))]   # step s reads the slots (0) when s is even, the shadows (1) when odd
            # the last step, s = n - 1, writes the set it does not read: the shadows iff n is odd -- exactly when the copy runs
            assert (n - 1) % 2 == 1 - copy_back
