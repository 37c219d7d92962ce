"""Rayleigh-Ritz in a batch, without a GPU: the four wafer_batch_* calls are declared, exported, bound and mirrored in the Rust source
with matching argument counts; wafer_amd.Batch checks its arguments before any library call; every C call refuses a NULL batch; the
sweep's --ritz flag leaves --plan alone; and ritz_phase against a batch object that only records calls."""
import ctypes as C
import io
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from wafer_amd import sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "golden", "cli_case.yaml")

# (wafer_batch_diag_ritz_counts(b, launches, readbacks): three arguments, as wafer_batch_diag_setup_counts)
NEW_CALLS = {"wafer_batch_ritz_matrices": 5, "wafer_batch_rotate_states": 4, "wafer_batch_ritz": 8, "wafer_batch_diag_ritz_counts": 3}
NEW_METHODS = ["ritz_matrices", "rotate_states", "ritz", "ritz_counts"]


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


def _count(args):
    return len([a for a in args.split(",") if a.strip() and a.strip() != "void"])


def test_ritz_calls_are_declared_exported_bound_and_mirrored(wa):
    from wafer_amd import engine
    header = open(os.path.join(ROOT, "include", "wafer_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = dict(re.findall(r"\bint\s*(wafer_batch_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header))
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    lib = wa.load_library()
    for name, nargs in NEW_CALLS.items():
        assert name in decls, name
        assert _count(decls[name]) == nargs, (name, decls[name])
        assert name in engine.EXPORTS, name
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
        m = re.search(r"pub fn %s\s*\((.*?)\)\s*->" % name, rust, flags=re.S)
        assert m, name
        assert _count(m.group(1)) == nargs, (name, m.group(1))
    assert re.search(r"#define\s+WAFER_ABI_VERSION\s+1\b", header)
    assert re.search(r"#define\s+WAFER_RITZ_MAX\s+8\b", header) and engine.RITZ_MAX == 8


def test_batch_has_the_ritz_methods(wa):
    import inspect
    for name in NEW_METHODS:
        assert callable(getattr(wa.Batch, name, None)), name
    for name in ("ritz_matrices", "ritz"):
        p = inspect.signature(getattr(wa.Batch, name)).parameters
        assert list(p) == ["self", "k", "active"] and p["k"].default is None and p["active"].default is None
    assert list(inspect.signature(wa.Batch.rotate_states).parameters) == ["self", "coefs", "active"]


@pytest.fixture
def unbound(wa):
    """a Batch that never reached the device (tests/test_batch_states_host.py): the argument checks see the member list alone"""
    b = object.__new__(wa.Batch)
    b.members = [wa.Params(16, 16, 16, dn=0.2, dt=0.004, max_states=2), wa.Params(16, 16, 16, dn=0.2, dt=0.002, max_states=3)]

    class _NoDevice:
        def __getattr__(self, name):
            raise AssertionError("argument check missing: %s reached the library" % name)
    b._L = _NoDevice()
    b._h = None
    return b


def test_batch_ritz_arguments_are_checked_before_the_library(unbound):
    b = unbound
    eye = [np.eye(2), np.eye(2)]
    for call in (lambda a: b.ritz_matrices(2, active=a), lambda a: b.ritz(2, active=a), lambda a: b.rotate_states(eye, active=a)):
        with pytest.raises(ValueError, match="one entry per member"):
            call([1, 0, 1])
    for call in (b.ritz_matrices, b.ritz):
        for k in (0, 9, -1, [2, 0], [9, 2]):
            with pytest.raises(ValueError, match="RITZ_MAX"):
                call(k)
        with pytest.raises(ValueError, match="max_states"):
            call(3)                                          # member 0 can hold two states
        with pytest.raises(ValueError, match="max_states"):
            call([2, 4])
        with pytest.raises(ValueError, match="one entry per member"):
            call([2, 2, 2])
    for coefs in ([np.eye(2), np.zeros((2, 3))], [np.zeros(4), np.eye(2)], [np.eye(2), None]):
        with pytest.raises(ValueError, match=r"\(k, k\)"):
            b.rotate_states(coefs)
    with pytest.raises(ValueError, match="one entry per member"):
        b.rotate_states([np.eye(2)])
    with pytest.raises(ValueError, match="max_states"):
        b.rotate_states([np.eye(3), np.eye(3)])
    with pytest.raises(ValueError, match="RITZ_MAX"):
        b.rotate_states([np.eye(2), np.eye(9)])
    with pytest.raises(ValueError, match="RITZ_MAX"):
        b.rotate_states([np.eye(2), np.zeros((0, 0))])
    # a member that is not listed is not checked: only then does the call reach the library
    with pytest.raises(AssertionError, match="reached the library"):
        b.ritz_matrices([9, 3], active=[0, 1])
    with pytest.raises(AssertionError, match="reached the library"):
        b.rotate_states([None, np.eye(3)], active=[0, 1])


def test_the_c_calls_refuse_a_null_batch(wa):
    from wafer_amd.engine import WAFER_ERR_INVALID
    L = wa.load_library()
    k = (C.c_uint32 * 1)(2)
    d = np.zeros(64)
    dp = d.ctypes.data_as(C.POINTER(C.c_double))
    st = (C.c_int * 1)(0)
    n = C.c_uint64(0)
    assert L.wafer_batch_ritz_matrices(None, None, k, dp, dp) == WAFER_ERR_INVALID
    assert L.wafer_batch_rotate_states(None, None, k, dp) == WAFER_ERR_INVALID
    assert L.wafer_batch_ritz(None, None, k, dp, dp, dp, dp, st) == WAFER_ERR_INVALID
    assert L.wafer_batch_diag_ritz_counts(None, C.byref(n), C.byref(n)) == WAFER_ERR_INVALID
    assert "null" in L.wafer_last_error().decode()


def test_ritz_flag_leaves_the_plan_alone():
    out = []
    for extra in ([], ["--ritz"]):
        r = subprocess.run([sys.executable, "-m", "wafer_amd.sweep", "--plan", *extra, "-c", CASE, "-c", CASE], capture_output=True, text=True,
                           cwd=ROOT, timeout=120)
        assert r.returncode == 0, r.stderr
        out.append(json.loads(r.stdout))
    assert out[0] == out[1] and "batches" in out[0]


# ---- ritz_phase against a batch that only records calls ---------------------------------------------------------------------------------
def cfg(wavenum=0, wavemax=0, **kw):
    c = dict(project_name="p", nx=20, ny=20, nz=20, dn=0.5, dt=0.04, tolerance=1e-7, central_difference=1, max_steps=None,
             wavenum=wavenum, wavemax=wavemax, potential="Harmonic", mass=1.0, init_condition="Boolean", sig=1.0,
             init_symmetry="NotConstrained", screen_update=10, snap_update=None, file_type="Csv", save_wavefns=False,
             save_potential=False, dtype="f64")
    c.update(kw)
    return c


class FakeBatch:
    """holds[m] stored states per member; ritz answers with h = diag(10 + a), s = 1, evals = a + m / 8 and the status given"""

    def __init__(self, holds, status=None):
        self.holds, self.status, self.calls = holds, status or [0] * len(holds), []

    def num_states(self):
        return list(self.holds)

    def ritz(self, k=None, active=None):
        self.calls.append(("ritz", tuple(k), tuple(active)))
        out = []
        for m, on in enumerate(active):
            if not on:
                out.append(None)
                continue
            n, ok = k[m], self.status[m] == 0
            out.append(dict(evals=np.arange(n) + m / 8.0 if ok else None, coef=np.eye(n) if ok else None, h=np.diag(10.0 + np.arange(n)),
                            s=np.eye(n), status=self.status[m]))
        return out

    def clone_state_to_phi(self, idx, active=None):
        self.calls.append(("clone", idx, tuple(active)))

    def observables(self):
        self.calls.append(("observables",))
        return [dict(energy=2.0 + m, norm2=1.0, v_infinity=0.0, r2=4.0) for m in range(len(self.holds))]

    def download_phi(self, m):
        self.calls.append(("download_phi", m))
        return np.zeros((22, 22, 22))


def converged_run(index, slot, tmp_path, wavenum=0, wavemax=0, statuses=None, **kw):
    d = tmp_path / f"run{index}"
    d.mkdir()
    r = sweep.Run(index, cfg(wavenum, wavemax, **kw), out_dir=str(d))
    r.slot = slot
    statuses = statuses or ["Converged"] * (wavemax - wavenum + 1)
    for w, s in zip(range(wavenum, wavemax + 1), statuses):
        r.states.append(dict(state=w, status=s, steps=100, energy=1.0))
        if s == "Converged":
            (d / f"observables_{w}.csv").write_text("before\n")
            (d / f"observables_{w}.json").write_text("before\n")
    r.failed = any(s != "Converged" for s in statuses)
    r.say("the table so far")
    r.write_table()
    return r


def test_ritz_phase_on_a_recording_batch(tmp_path):
    from wafer_amd.engine import WAFER_ERR_STATE
    from wafer_amd.run import rust_lower_exp
    runs = [converged_run(10, 0, tmp_path, 0, 2, save_wavefns=True),              # three states: rotated
            converged_run(11, 1, tmp_path, 0, 1, statuses=["Converged", "MaxStep"]),  # not every state converged
            converged_run(12, 2, tmp_path, 0, 1),                                  # two states: rotated
            converged_run(13, 3, tmp_path, 0, 8),                                  # nine states: too many
            converged_run(14, 4, tmp_path, 1, 2)]                                  # three states, one from disk: its solve fails
    b = FakeBatch([3, 1, 2, 9, 3], status=[0, 0, 0, 0, WAFER_ERR_STATE])
    log = io.StringIO()
    sweep.ritz_phase(b, runs, log=log)
    assert [c for c in b.calls if c[0] == "ritz"] == [("ritz", (3, 0, 2, 0, 3), (1, 0, 1, 0, 1))]      # one call, the eligible runs only
    assert log.getvalue().splitlines() == ["run 11: Ritz: skipped, not every state converged",
                                           "run 13: Ritz: skipped, 9 stored states (the step takes 2 .. 8)",
                                           "run 14: Ritz: skipped, the overlap matrix is not positive definite"]
    # per state number one clone and one observables for the rotated runs that have it
    rest = [c for c in b.calls if c[0] in ("clone", "observables")]
    assert rest == [("clone", 0, (1, 0, 1, 0, 0)), ("observables",), ("clone", 1, (1, 0, 1, 0, 0)), ("observables",),
                    ("clone", 2, (1, 0, 0, 0, 0)), ("observables",)]
    assert [c for c in b.calls if c[0] == "download_phi"] == [("download_phi", 0)] * 3          # save_wavefns of run 10 only
    for r, k in ((runs[0], 3), (runs[2], 2)):
        table = open(r.path("table.txt")).read().splitlines()
        assert table[:2] == ["the table so far", "Ritz"] and table[-1] == "" and len(table) == 3 + k
        for a in range(k):
            assert table[2 + a] == "%3d %19s %19s" % (a, rust_lower_exp(10.0 + a, 10), rust_lower_exp(a + r.slot / 8.0, 10))
            row = open(r.path(f"observables_{a}.csv")).read().splitlines()
            assert row[0] == "state,energy,binding_energy,r,l_r" and row[1].split(",")[:2] == [str(a), repr(2.0 + r.slot)]
            assert json.load(open(r.path(f"observables_{a}.json")))["state"] == a
        assert r.ritz == dict(evals=[a + r.slot / 8.0 for a in range(k)])
    assert sorted(f for f in os.listdir(runs[0].out_dir) if f.startswith("wavefunction")) == [f"wavefunction_{a}.npy" for a in range(3)]
    for r in (runs[1], runs[3], runs[4]):                                          # not rotated: table and files as they were
        assert open(r.path("table.txt")).read() == "the table so far\n" and r.ritz is None
        for name in os.listdir(r.out_dir):
            if name.startswith("observables"):
                assert open(r.path(name)).read() == "before\n", (r.index, name)
        assert not any(f.startswith("wavefunction") for f in os.listdir(r.out_dir))


def test_ritz_phase_with_no_eligible_run_makes_no_call(tmp_path):
    runs = [converged_run(0, 0, tmp_path, 0, 0), converged_run(1, 1, tmp_path, 0, 1, statuses=["Converged", "MaxStep"])]
    b = FakeBatch([1, 1])
    log = io.StringIO()
    sweep.ritz_phase(b, runs, log=log)
    assert b.calls == []
    assert log.getvalue().splitlines() == ["run 0: Ritz: skipped, 1 stored states (the step takes 2 .. 8)",
                                           "run 1: Ritz: skipped, not every state converged"]
