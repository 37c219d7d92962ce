"""wafer_amd.sweep without a GPU: the grouping of runs into batches (plan_batches), the step between block boundaries (next_chunk),
the boundary bookkeeping of run_phase against a batch object that only records calls, and `--plan` on the command line."""
import json
import os
import subprocess
import sys

import pytest

from wafer_amd import sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "golden", "cli_case.yaml")


def cfg(n=(20, 20, 20), cd=1, dtype="f64", wavenum=0, wavemax=0, **kw):
    c = dict(project_name="p", nx=n[0], ny=n[1], nz=n[2], dn=0.5, dt=0.04, tolerance=1e-7, central_difference=cd, max_steps=None,
             wavenum=wavenum, wavemax=wavemax, potential="Harmonic", mass=1.0, init_condition="Boolean", sig=1.0,
             init_symmetry="NotConstrained", screen_update=10, snap_update=None, file_type="Csv", save_wavefns=False,
             save_potential=False, dtype=dtype)
    c.update(kw)
    return c


def every_index_once(plan, n):
    return sorted(i for b in plan for i in b["members"]) == list(range(n))


# ---- plan_batches ---------------------------------------------------------------------------------------------------------------
def test_partition_by_stencil_and_dtype():
    cfgs = [cfg(cd=1), cfg(cd=3), cfg(cd=1, dtype="f32"), cfg(cd=1), cfg(cd=3, dtype="f32"), cfg(cd=1, dtype="f32")]
    plan = sweep.plan_batches(cfgs, 64)
    assert [b["members"] for b in plan] == [[0, 3], [1], [2, 5], [4]]
    assert [(b["central_difference"], b["dtype"]) for b in plan] == [(1, "f64"), (3, "f64"), (1, "f32"), (3, "f32")]
    assert every_index_once(plan, len(cfgs))


def test_state_runs_split_by_shape_and_ground_runs_share_a_mixed_batch():
    a, b, c = (20, 20, 20), (16, 20, 12), (24, 24, 24)
    cfgs = [cfg(a), cfg(b, wavemax=2), cfg(c), cfg(a, wavemax=1), cfg(b), cfg(b, wavenum=1, wavemax=1), cfg(a, wavemax=2)]
    plan = sweep.plan_batches(cfgs, 64)
    assert [p["members"] for p in plan] == [[0, 2, 4], [1, 5], [3, 6]]
    ground, sb, sa = plan
    assert ground["mixed_shapes"] and not ground["needs_states"] and ground["shapes"] == [list(a), list(c), list(b)]
    for p, shape in ((sb, b), (sa, a)):
        assert p["needs_states"] and not p["mixed_shapes"] and p["shapes"] == [list(shape)]
    assert every_index_once(plan, len(cfgs))


def test_max_batch_cuts_in_input_order():
    cfgs = [cfg((8 + i, 8, 8)) for i in range(7)] + [cfg(wavemax=1) for _ in range(3)]
    plan = sweep.plan_batches(cfgs, 3)
    assert [p["members"] for p in plan] == [[0, 1, 2], [3, 4, 5], [6], [7, 8, 9]]
    assert all(len(p["members"]) <= 3 for p in plan) and every_index_once(plan, len(cfgs))
    assert [p["members"] for p in sweep.plan_batches(cfgs, 1)] == [[i] for i in range(10)]
    with pytest.raises(ValueError):
        sweep.plan_batches(cfgs, 0)


def test_single_config():
    plan = sweep.plan_batches([cfg((24, 20, 28), wavemax=1)])
    assert plan == [dict(members=[0], central_difference=1, dtype="f64", needs_states=True, mixed_shapes=False, shapes=[[24, 20, 28]])]
    plan = sweep.plan_batches([cfg((24, 20, 28))])
    assert plan[0]["members"] == [0] and plan[0]["mixed_shapes"] and not plan[0]["needs_states"]


# ---- next_chunk and the boundaries ----------------------------------------------------------------------------------------------
def test_next_chunk():
    assert sweep.next_chunk([10, 25, 40]) == 10
    assert sweep.next_chunk([5, 10, 30]) == 5
    assert sweep.next_chunk([7]) == 7
    with pytest.raises(ValueError):
        sweep.next_chunk([0, 3])


class FakeBatch:
    """records the calls of run_phase; member m's energy falls by 2^-k at its k-th boundary, so a run converges where its tolerance
    says, independently of the others"""

    def __init__(self, n):
        self.n, self.steps, self.calls = n, [0] * n, []
        self.seen = [0] * n

    def observables(self):
        self.calls.append(("observables",))
        return [dict(energy=1.0 + 2.0 ** -(self.steps[m] // 5), norm2=1.0, v_infinity=0.0, r2=1.0) for m in range(self.n)]

    def evolve(self, d, active=None, wnum=0):
        self.calls.append(("evolve", d, tuple(active), wnum))
        for m in range(self.n):
            if active[m]:
                self.steps[m] += d

    def normalise(self, norm2s, active=None):
        self.calls.append(("normalise", tuple(active)))

    def orthogonalise(self, wnum, active=None):
        self.calls.append(("orthogonalise", wnum, tuple(active)))

    def symmetrise(self, cons, active=None):
        self.calls.append(("symmetrise", tuple(cons), tuple(active)))

    def push_state(self, active=None):
        self.calls.append(("push_state", tuple(active)))

    def norm2(self):
        return [1.0] * self.n


def make_runs(specs):
    runs = [sweep.Run(i, cfg(**s)) for i, s in enumerate(specs)]
    for i, r in enumerate(runs):
        r.slot = i
    return runs


def test_boundaries_of_members_with_their_own_screen_update():
    # energies 1 + 2^-(step / 5): the difference between boundaries su apart is below tol once 2^-((step - su) / 5) < tol, roughly
    runs = make_runs([dict(screen_update=10, tolerance=2.0 ** -20), dict(screen_update=25, tolerance=2.0 ** -30),
                      dict(screen_update=40, tolerance=2.0 ** -10, max_steps=70)])
    b = FakeBatch(3)
    sweep.run_phase(b, runs, 0, progress=True, push=True)
    # every run's boundaries are the multiples of its own screen_update, up to where it stopped
    for r in runs:
        su = r.cfg["screen_update"]
        assert r.boundaries == list(range(0, r.states[0]["steps"] + 1, su)), r.index
        assert r.states[0]["steps"] == b.steps[r.slot]
    # the evolve calls stop at exactly the union of the boundaries: 10, 20, 25, 30, 40, 50, ...
    at, reached = 0, []
    for c in b.calls:
        if c[0] == "evolve":
            at += c[1]
            reached.append(at)
    assert reached[:8] == [10, 20, 25, 30, 40, 50, 60, 70]
    union = sorted({s for r in runs for s in r.boundaries if s > 0})
    assert reached == union
    # every evolve carries all running members; a finished member is in no later mask
    done_at = [r.states[0]["steps"] for r in runs]
    at = 0
    for c in b.calls:
        if c[0] == "evolve":
            assert c[2] == tuple(1 if at < done_at[m] else 0 for m in range(3)), at
            assert c[3] == 0
            at += c[1]
    # statuses: the tolerances are met where the energy law says; the third run passes its max_steps first
    assert [r.states[0]["status"] for r in runs] == ["Converged", "Converged", "MaxStep"]
    assert done_at == [110, 175, 80]
    assert [r.failed for r in runs] == [False, False, True]
    # one normalise per boundary moment, with the members at that boundary; pushes only for converged members
    norm_masks = [c[1] for c in b.calls if c[0] == "normalise"]
    assert norm_masks[0] == (1, 1, 1)                       # step 0
    assert norm_masks[1] == (1, 0, 0)                       # step 10
    assert norm_masks[3] == (0, 1, 0)                       # step 25
    assert norm_masks[5] == (1, 0, 1)                       # step 40
    assert norm_masks[6] == (1, 1, 0)                       # step 50
    pushed = [c[1] for c in b.calls if c[0] == "push_state"]
    assert sorted(m for mask in pushed for m in range(3) if mask[m]) == [r.slot for r in runs if r.states[0]["status"] == "Converged"]
    # the table: a header, a row per boundary (progress), and the summary of a converged run
    for r in runs:
        rows = [l for l in r.lines if l.lstrip().startswith("│")]
        assert len(rows) == len(r.boundaries)
        assert ("Ground state energy" in "\n".join(r.lines)) == (r.states[0]["status"] == "Converged")


def test_max_steps_fails_one_member_and_the_others_go_on():
    runs = make_runs([dict(screen_update=10, tolerance=2.0 ** -12), dict(screen_update=25, tolerance=0.0, max_steps=60)])
    b = FakeBatch(2)
    sweep.run_phase(b, runs, 0)
    assert runs[1].failed and runs[1].states[0] == dict(state=0, status="MaxStep", steps=75, energy=runs[1].states[0]["energy"])
    assert not runs[0].failed and runs[0].states[0]["status"] == "Converged"
    assert not any(c[0] == "push_state" for c in b.calls)              # push=False: a ground-state batch
    rows = [l for l in runs[0].lines if l.lstrip().startswith("│")]
    assert len(rows) == 1                                               # without progress: the converging row alone
    assert not runs[1].takes_part(1) and not runs[0].takes_part(1)


def test_excited_phase_and_snapshots():
    runs = make_runs([dict(screen_update=10, tolerance=2.0 ** -8, wavemax=1, central_difference=3, init_symmetry="AboutY", snap_update=20),
                      dict(screen_update=10, tolerance=2.0 ** -8, wavemax=0, central_difference=3),
                      dict(screen_update=5, tolerance=2.0 ** -8, wavemax=1, central_difference=3)])
    b = FakeBatch(3)
    sweep.run_phase(b, runs, 1, push=True)
    assert runs[1].states == []                                         # wavemax 0: no part in phase 1
    ev = [c for c in b.calls if c[0] == "evolve"]
    assert ev and all(c[3] == 1 and c[2][1] == 0 for c in ev)
    orth = [c for c in b.calls if c[0] == "orthogonalise"]
    assert len(orth) == len([c for c in b.calls if c[0] == "normalise"]) and all(c[1] == 1 for c in orth)
    sym = [c for c in b.calls if c[0] == "symmetrise"]
    snap_steps = [s for s in runs[0].boundaries if s % 20 == 0]
    assert len(sym) == len(snap_steps) and all(c[1] == ("AboutY", "NotConstrained", "NotConstrained") and c[2] == (1, 0, 0) for c in sym)


# ---- --plan ---------------------------------------------------------------------------------------------------------------------
def test_plan_on_the_command_line(tmp_path):
    text = open(CASE).read()
    edits = [[], [("x: 24", "x: 16"), ("wavemax: 1", "wavemax: 0")], [("wavemax: 1", "wavemax: 0"), ("dn: 0.5", "dn: 0.6")]]
    paths = []
    for k, ed in enumerate(edits):
        t = text
        for old, new in ed:
            assert old in t
            t = t.replace(old, new)
        p = tmp_path / f"run{k}.yaml"
        p.write_text(t)
        paths.append(str(p))
    cmd = [sys.executable, "-m", "wafer_amd.sweep", "--plan", "--max-batch", "8"]
    for p in paths:
        cmd += ["-c", p]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out["configs"] == paths
    assert out["batches"] == [
        dict(members=[0], central_difference=1, dtype="f64", needs_states=True, mixed_shapes=False, shapes=[[24, 20, 28]]),
        dict(members=[1, 2], central_difference=1, dtype="f64", needs_states=False, mixed_shapes=True, shapes=[[16, 20, 28], [24, 20, 28]]),
    ]
    bad = tmp_path / "bad.yaml"
    bad.write_text(text.replace("dt: 0.04", "dt: 0.09"))
    r = subprocess.run(cmd + ["-c", str(bad)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "LargeDt" in r.stderr
