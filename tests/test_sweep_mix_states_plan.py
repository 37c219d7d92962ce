"""wafer_amd.sweep's opt-in grouping of state runs of several shapes into one batch (plan_batches(..., mix_states=True), --mix-states),
without a GPU: the plan, the command line, and the scheduling of an excited phase over two shapes against the recording batch of
tests/test_sweep_plan.py."""
import json
import subprocess
import sys

import pytest

from tests.test_sweep_plan import CASE, ROOT, FakeBatch, cfg, every_index_once, make_runs
from wafer_amd import sweep

A, B, C = (20, 20, 20), (16, 20, 12), (24, 24, 24)


def mixed_cfgs():
    return [cfg(A), cfg(B, wavemax=2), cfg(C), cfg(A, wavemax=1), cfg(B), cfg(B, wavenum=1, wavemax=1), cfg(A, wavemax=2)]


def test_state_runs_of_all_shapes_share_a_batch():
    cfgs = mixed_cfgs()
    plan = sweep.plan_batches(cfgs, 64, mix_states=True)
    assert [p["members"] for p in plan] == [[0, 2, 4], [1, 3, 5, 6]]
    ground, states = plan
    assert ground == dict(members=[0, 2, 4], central_difference=1, dtype="f64", needs_states=False, mixed_shapes=True,
                          shapes=[list(A), list(C), list(B)])
    assert states == dict(members=[1, 3, 5, 6], central_difference=1, dtype="f64", needs_states=True, mixed_shapes=True,
                          shapes=[list(B), list(A)])
    assert every_index_once(plan, len(cfgs))


def test_without_the_flag_the_plan_is_todays():
    for cfgs in (mixed_cfgs(), [cfg((24, 20, 28), wavemax=1)], [cfg((8 + i, 8, 8)) for i in range(7)] + [cfg(wavemax=1) for _ in range(3)]):
        for max_batch in (1, 3, 64):
            assert sweep.plan_batches(cfgs, max_batch, mix_states=False) == sweep.plan_batches(cfgs, max_batch)
    plan = sweep.plan_batches(mixed_cfgs(), 64)   # (tests/test_sweep_plan.py pins these)
    assert [p["members"] for p in plan] == [[0, 2, 4], [1, 5], [3, 6]]
    assert [(p["needs_states"], p["mixed_shapes"]) for p in plan] == [(False, True), (True, False), (True, False)]


def test_max_batch_cuts_the_state_group_in_input_order():
    cfgs = [cfg((8 + i, 8, 8), wavemax=1) for i in range(7)] + [cfg() for _ in range(2)]
    plan = sweep.plan_batches(cfgs, 3, mix_states=True)
    assert [p["members"] for p in plan] == [[0, 1, 2], [3, 4, 5], [6], [7, 8]]
    assert [p["shapes"] for p in plan[:3]] == [[[8, 8, 8], [9, 8, 8], [10, 8, 8]], [[11, 8, 8], [12, 8, 8], [13, 8, 8]], [[14, 8, 8]]]
    assert all(p["needs_states"] and p["mixed_shapes"] for p in plan[:3]) and not plan[3]["needs_states"]
    assert all(len(p["members"]) <= 3 for p in plan) and every_index_once(plan, len(cfgs))
    with pytest.raises(ValueError):
        sweep.plan_batches(cfgs, 0, mix_states=True)


def test_stencil_and_dtype_still_partition():
    cfgs = [cfg(A, wavemax=1), cfg(B, cd=3, wavemax=1), cfg(B, dtype="f32", wavemax=2), cfg(C, wavemax=1), cfg(C, cd=3, wavemax=1),
            cfg(A, dtype="f32", wavemax=1), cfg(A, cd=3)]
    plan = sweep.plan_batches(cfgs, 64, mix_states=True)
    assert [p["members"] for p in plan] == [[0, 3], [1, 4], [2, 5], [6]]
    assert [(p["central_difference"], p["dtype"]) for p in plan] == [(1, "f64"), (3, "f64"), (1, "f32"), (3, "f64")]
    assert [p["shapes"] for p in plan] == [[list(A), list(C)], [list(B), list(C)], [list(B), list(A)], [list(A)]]
    assert every_index_once(plan, len(cfgs))


def test_a_single_state_run_is_a_mixed_group_of_one_shape():
    plan = sweep.plan_batches([cfg((24, 20, 28), wavemax=1)], mix_states=True)
    assert plan == [dict(members=[0], central_difference=1, dtype="f64", needs_states=True, mixed_shapes=True, shapes=[[24, 20, 28]])]


def test_excited_phase_over_two_shapes():
    """run_phase does not know shapes: members of two shapes at their own boundaries share every call of the phase"""
    runs = make_runs([dict(n=A, screen_update=10, tolerance=2.0 ** -8, wavemax=1), dict(n=B, screen_update=25, tolerance=2.0 ** -12, wavemax=2),
                      dict(n=A, screen_update=10, tolerance=2.0 ** -8, wavemax=0), dict(n=B, screen_update=40, tolerance=2.0 ** -6, wavemax=1, max_steps=30)])
    plan = sweep.plan_batches([r.cfg for r in runs], mix_states=True)
    assert [p["members"] for p in plan] == [[0, 1, 3], [2]] and plan[0]["shapes"] == [list(A), list(B)]
    members = [runs[i] for i in plan[0]["members"]]
    for slot, r in enumerate(members):
        r.slot = slot
    b = FakeBatch(3)
    sweep.run_phase(b, members, 1, progress=True, push=plan[0]["needs_states"])
    for r in members:
        su = r.cfg["screen_update"]
        assert r.boundaries == list(range(0, r.states[0]["steps"] + 1, su)) and r.states[0]["steps"] == b.steps[r.slot]
    ev = [c for c in b.calls if c[0] == "evolve"]
    assert ev and all(c[3] == 1 for c in ev)
    assert ev[0][2] == (1, 1, 1)                                        # one evolve for the members of both shapes
    at, reached = 0, []
    for c in ev:
        at += c[1]
        reached.append(at)
    assert reached == sorted({s for r in members for s in r.boundaries if s > 0})
    orth = [c for c in b.calls if c[0] == "orthogonalise"]
    norm = [c for c in b.calls if c[0] == "normalise"]
    assert len(orth) == len(norm) and all(o[1] == 1 and o[2] == m[1] for o, m in zip(orth, norm))
    assert norm[0][1] == (1, 1, 1)
    assert [r.states[0]["status"] for r in members] == ["Converged", "Converged", "MaxStep"]
    pushed = [c[1] for c in b.calls if c[0] == "push_state"]
    assert sorted(m for mask in pushed for m in range(3) if mask[m]) == [0, 1]
    # phase 2: only the run with wavemax 2 takes part
    b2 = FakeBatch(3)
    sweep.run_phase(b2, members, 2, push=True)
    assert all(c[2] == (0, 1, 0) and c[3] == 2 for c in b2.calls if c[0] == "evolve")
    assert [len(r.states) for r in members] == [1, 2, 1]


def test_run_batch_asks_for_state_stores_only_for_such_a_group(monkeypatch):
    import wafer_amd
    seen = []

    class Stop(Exception):
        pass

    def fake(pars, **kw):
        seen.append(kw)
        raise Stop

    monkeypatch.setattr(wafer_amd, "Batch", fake)
    cfgs = [cfg(A, wavemax=1), cfg(B, wavemax=1), cfg(C)]
    for mix in (True, False):
        for p in sweep.plan_batches(cfgs, mix_states=mix):
            with pytest.raises(Stop):
                sweep.run_batch(p, [sweep.Run(i, cfgs[i]) for i in p["members"]], 7, False)
    assert seen == [dict(mixed_shapes=True, state_stores=True), dict(mixed_shapes=True),
                    dict(mixed_shapes=False), dict(mixed_shapes=False), dict(mixed_shapes=True)]


def test_plan_with_mix_states_on_the_command_line(tmp_path):
    text = open(CASE).read()
    edits = [[], [("x: 24", "x: 16")], [("wavemax: 1", "wavemax: 0"), ("dn: 0.5", "dn: 0.6")]]
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
    r = subprocess.run(cmd + ["--mix-states"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out["configs"] == paths
    assert out["batches"] == [
        dict(members=[0, 1], central_difference=1, dtype="f64", needs_states=True, mixed_shapes=True, shapes=[[24, 20, 28], [16, 20, 28]]),
        dict(members=[2], central_difference=1, dtype="f64", needs_states=False, mixed_shapes=True, shapes=[[24, 20, 28]]),
    ]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)   # without the flag: one batch per shape, as before
    assert r.returncode == 0, r.stderr
    assert [(b["members"], b["mixed_shapes"]) for b in json.loads(r.stdout)["batches"]] == [([0], False), ([1], False), ([2], True)]
