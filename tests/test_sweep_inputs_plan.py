"""wafer_amd.sweep's input files without a GPU: plan_inputs groups the runs of a batch by role and file, a file of a run's own size
is copied and anything else resampled, set_up_batch / start_phase turn every group into ONE Batch.resample_* call with its mask
(against a batch object that only records calls), and `--plan` prints the groups."""
import json
import os
import subprocess
import sys

import numpy as np

from wafer_amd import sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "golden", "cli_case.yaml")


def cfg(n=(24, 20, 28), cd=1, wavenum=0, wavemax=0, **kw):
    c = dict(project_name="p", nx=n[0], ny=n[1], nz=n[2], dn=0.5, dt=0.04, tolerance=1e-7, central_difference=cd, max_steps=None,
             wavenum=wavenum, wavemax=wavemax, potential="FromFile", mass=1.0, init_condition="Boolean", sig=1.0,
             init_symmetry="NotConstrained", screen_update=10, snap_update=None, file_type="Csv", save_wavefns=False,
             save_potential=False, dtype="f64")
    c.update(kw)
    return c


def make_runs(specs, dirs):
    runs = [sweep.Run(i, cfg(**s), f"run{i}.yaml", str(d)) for i, (s, d) in enumerate(zip(specs, dirs))]
    for i, r in enumerate(runs):
        r.slot = i
    return runs


def save(d, stem, shape, seed=0):
    d.mkdir(exist_ok=True)
    a = np.random.default_rng(seed).standard_normal(shape)
    np.save(d / f"{stem}.npy", a)
    return a


class Recorder:
    """a Batch that only records: (name, arguments with arrays replaced by their shapes, mask)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args, active=None, **kw):
            shown = tuple(tuple(a.shape) if isinstance(a, np.ndarray) else a for a in args)
            self.calls.append((name, shown, None if active is None else tuple(active), kw))
        return call

    def named(self, name):
        return [c for c in self.calls if c[0] == name]


# ---- plan_inputs ----------------------------------------------------------------------------------------------------------------
def test_groups_by_role_and_real_path(tmp_path):
    """three runs read one directory (one of them through a symbolic link), a fourth its own: one group per role and file"""
    shared, own = tmp_path / "shared", tmp_path / "own"
    save(shared, "potential", (12, 10, 14))
    save(shared, "potential_sub", (6, 5, 7), 1)
    save(own, "potential", (12, 10, 14))
    os.symlink(shared, tmp_path / "link")
    runs = make_runs([dict(), dict(n=(16, 20, 28)), dict(), dict(n=(16, 20, 28))], [shared, shared, own, tmp_path / "link"])
    groups = sweep.plan_inputs(runs)
    assert [(g["role"], g["members"]) for g in groups] == [("potential", [0, 1, 3]), ("potential", [2]), ("potential_sub", [0, 1, 3])]
    assert groups[0]["path"] == os.path.realpath(shared / "potential.npy") and groups[0]["shape"] == [12, 10, 14]
    assert all(g["copy"] == [] and g["resample"] == g["members"] for g in groups)
    # the same path rewritten later is another file
    before = groups[0]["mtime"]
    os.utime(shared / "potential.npy", (before + 10, before + 10))
    assert sweep.plan_inputs(runs)[0]["mtime"] == before + 10


def test_a_file_of_a_runs_own_size_is_copied(tmp_path):
    d = tmp_path / "in"
    save(d, "potential", (16, 20, 28))            # run 1's work size
    save(d, "potential_sub", (24, 20, 28), 1)     # run 0's work size
    runs = make_runs([dict(), dict(n=(16, 20, 28)), dict(n=(14, 18, 26))], [d] * 3)
    pot, sub = sweep.plan_inputs(runs)
    # (16, 20, 28) is run 1's work size and, the file being a ready-made .npy, run 2's framed array: both are copied
    assert (pot["role"], pot["copy"], pot["resample"]) == ("potential", [1, 2], [0])
    assert (sub["role"], sub["copy"], sub["resample"]) == ("potential_sub", [0], [1, 2])
    # a ready-made .npy of a run's padded size is that run's framed array; for every other run it is plain data
    assert sweep.how_to_set(runs[2].cfg, "potential", str(d / "potential.npy"), (16, 20, 28)) == "framed"
    assert sweep.how_to_set(runs[2].cfg, "potential", str(d / "potential.csv"), (16, 20, 28)) == "resample"
    assert sweep.how_to_set(runs[1].cfg, "potential", str(d / "potential.csv"), (16, 20, 28)) == "copy"
    assert sweep.how_to_set(runs[1].cfg, "potential_sub", str(d / "potential_sub.npy"), ()) == "copy"


def test_lower_states_and_starts(tmp_path):
    d = tmp_path / "in"
    save(d, "potential", (12, 10, 14))
    save(d, "wavefunction_0", (12, 10, 14), 1)
    save(d, "wavefunction_1_partial", (12, 10, 14), 2)
    runs = make_runs([dict(wavenum=1, wavemax=1), dict(n=(16, 20, 28), wavenum=1, wavemax=2), dict(wavemax=1)], [d] * 3)
    groups = sweep.plan_inputs(runs)
    assert [(g["role"], g["state"], g["members"]) for g in groups] == \
        [("potential", 0, [0, 1, 2]), ("state", 0, [0, 1]), ("start", 1, [0, 1, 2])]
    assert groups[2]["path"].endswith("wavefunction_1_partial.npy")
    only = sweep.plan_inputs(runs, roles={("start", 1)})
    assert [(g["role"], g["state"]) for g in only] == [("start", 1)]
    # state 0 of run 2 starts from its Boolean condition, not from the file; with init_condition FromFile it reads it
    runs[2].cfg["init_condition"] = "FromFile"
    assert [(g["role"], g["state"], g["members"]) for g in sweep.plan_inputs(runs)][2] == ("start", 0, [2])


# ---- the calls ------------------------------------------------------------------------------------------------------------------
def test_one_resample_call_per_distinct_file_with_the_right_mask(tmp_path):
    shared, own = tmp_path / "shared", tmp_path / "own"
    save(shared, "potential", (16, 20, 28))
    save(shared, "wavefunction_0", (12, 10, 14), 2)
    save(own, "potential", (9, 9, 9), 3)
    runs = make_runs([dict(wavenum=1, wavemax=1), dict(n=(16, 20, 28)), dict(), dict(wavenum=1, wavemax=1), dict(potential="Harmonic")],
                     [shared, shared, own, shared, shared])
    b = Recorder()
    sweep.set_up_batch(b, runs)
    pot = b.named("resample_potential")
    assert [(c[1], c[2], c[3]) for c in pot] == [(((16, 20, 28),), (1, 0, 0, 1, 0), dict(basis="padded")),
                                                 (((9, 9, 9),), (0, 0, 1, 0, 0), dict(basis="padded"))]
    assert [c[1][0] for c in b.named("set_potential_host")] == [1]                # run 1: its own size, in its zero frame
    assert b.named("set_potential_host")[0][1][1] == (18, 22, 30)
    assert [c[1] for c in b.named("set_potential")] == [(4, "Harmonic")]
    st = b.named("resample_state")
    assert [(c[1], c[2], c[3]) for c in st] == [((0, (12, 10, 14)), (1, 0, 0, 1, 0), dict(basis="padded"))]
    assert not b.named("load_state") and not b.named("set_potsub") and not b.named("resample_potsub")


def test_potential_sub_is_resampled_with_the_work_basis(tmp_path):
    """an array suits FullCornell only (potential.rs:113-131); the run whose size it has is set as before, the others in one call,
    after every potential (setting a potential resets pot_sub)"""
    d = tmp_path / "in"
    save(d, "potential_sub", (16, 20, 28))
    runs = make_runs([dict(potential="FullCornell"), dict(n=(16, 20, 28), potential="FullCornell"), dict(n=(8, 9, 10), potential="FullCornell")],
                     [d] * 3)
    b = Recorder()
    sweep.set_up_batch(b, runs)
    assert [(c[1], c[2], c[3]) for c in b.named("resample_potsub")] == [(((16, 20, 28),), (1, 0, 1), dict(basis="work"))]
    assert [c[1] for c in b.named("set_potsub")] == [(1, 2, 0.0, (16, 20, 28))]
    names = [c[0] for c in b.calls]
    assert max(i for i, n in enumerate(names) if n == "set_potential") < min(names.index("resample_potsub"), names.index("set_potsub"))
    runs[2].cfg["potential"] = "Harmonic"
    try:
        sweep.set_up_batch(Recorder(), runs)
    except SystemExit as e:
        assert "WrongPotentialSubDims" in str(e) and "run2.yaml" in str(e)
    else:
        raise AssertionError("an array for a potential with a scalar pot_sub was accepted")


def test_starts_of_a_phase_are_one_call(tmp_path):
    d = tmp_path / "in"
    save(d, "wavefunction_1", (12, 10, 14))
    runs = make_runs([dict(wavemax=1, potential="Harmonic"), dict(n=(12, 10, 14), wavemax=1, potential="Harmonic"),
                      dict(wavemax=1, potential="Harmonic")], [d, d, tmp_path / "none"])
    b = Recorder()
    sweep.start_phase(b, runs, None, 1, seed=3)
    assert [(c[1], c[2]) for c in b.named("resample_phi")] == [(((12, 10, 14),), (1, 0, 0))]
    assert [c[1] for c in b.named("upload_phi")] == [(1, (14, 12, 16))]          # its own size: copied into its frame
    assert [(c[1], c[2]) for c in b.named("clone_state_to_phi")] == [((0,), (0, 0, 1))] and runs[2].cloned and not runs[0].cloned
    b = Recorder()
    sweep.start_phase(b, runs, None, 0, seed=3)
    assert [c[1] for c in b.named("set_initial_condition")] == [(0, "Boolean"), (1, "Boolean"), (2, "Boolean")]
    assert len(b.named("symmetrise")) == 1 and not b.named("resample_phi")


# ---- --plan ---------------------------------------------------------------------------------------------------------------------
def test_plan_prints_the_inputs(tmp_path):
    text = open(CASE).read()
    assert "potential: " in text
    edits = [[], [("x: 24", "x: 16"), ("wavemax: 1", "wavemax: 0")], [("wavemax: 1", "wavemax: 0")]]
    paths = []
    for k, ed in enumerate(edits):
        t = text
        for old, new in ed:
            assert old in t
            t = t.replace(old, new)
        p = tmp_path / f"run{k}.yaml"
        p.write_text(t)
        paths.append(str(p))
    inp = tmp_path / "inp"
    save(inp, "potential_sub", (12, 10, 14))
    save(inp, "wavefunction_1", (24, 20, 28), 1)
    base = [sys.executable, "-m", "wafer_amd.sweep", "--plan", "--max-batch", "8"]
    for p in paths:
        base += ["-c", p]
    r = subprocess.run(base + ["--input-dir", str(inp)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert list(out) == ["configs", "batches", "inputs"]
    sub = os.path.realpath(inp / "potential_sub.npy")
    assert out["inputs"] == [
        dict(batch=0, role="potential_sub", state=0, path=sub, shape=[12, 10, 14], members=[0], copy=[], resample=[0]),
        dict(batch=0, role="start", state=1, path=os.path.realpath(inp / "wavefunction_1.npy"), shape=[24, 20, 28], members=[0], copy=[0],
             resample=[]),
        dict(batch=1, role="potential_sub", state=0, path=sub, shape=[12, 10, 14], members=[1, 2], copy=[], resample=[1, 2]),
    ]
    bare = subprocess.run(base, capture_output=True, text=True, cwd=ROOT)   # no input directory: the same plan, no inputs
    assert bare.returncode == 0, bare.stderr
    bare = json.loads(bare.stdout)
    assert bare["inputs"] == [] and bare["configs"] == out["configs"] == paths and bare["batches"] == out["batches"]
    assert out["batches"] == [
        dict(members=[0], central_difference=1, dtype="f64", needs_states=True, mixed_shapes=False, shapes=[[24, 20, 28]]),
        dict(members=[1, 2], central_difference=1, dtype="f64", needs_states=False, mixed_shapes=True, shapes=[[16, 20, 28], [24, 20, 28]]),
    ]


def test_plan_looks_without_converting(tmp_path):
    """--plan reads the shape of a .csv from its last row and of a .npy from its header; it runs no converter and leaves no cache"""
    inp = tmp_path / "inp"
    inp.mkdir()
    a = np.arange(3 * 4 * 5, dtype=float).reshape(3, 4, 5)
    with open(inp / "potential.csv", "w") as f:
        for (i, j, k), v in np.ndenumerate(a):
            f.write(f"{i},{j},{k},{float(v)!r}\n")
    (inp / "potential_sub.csv").write_text("0.75\n")
    (inp / "wavefunction_0.json").write_text("[]")
    assert sweep.peek_shape(str(inp / "potential.csv")) == [3, 4, 5] and sweep.peek_shape(str(inp / "potential_sub.csv")) == []
    assert sweep.peek_shape(str(inp / "wavefunction_0.json")) is None
    runs = make_runs([dict(n=(3, 4, 5)), dict(init_condition="FromFile")], [inp, inp])
    groups = sweep.plan_inputs(runs, load=None)
    assert [(g["role"], g["shape"], g["copy"], g["resample"]) for g in groups] == \
        [("potential", [3, 4, 5], [0], [1]), ("potential_sub", [], [0, 1], []), ("start", None, None, None)]
    assert groups[2]["members"] == [1] and all("array" not in g for g in groups)
    assert sorted(os.listdir(inp)) == ["potential.csv", "potential_sub.csv", "wavefunction_0.json"]
    # set-up reads every file once and hands the array on
    seen = []
    def load(run, stem):
        seen.append(stem)
        return a if stem == "potential" else np.float64(0.75)
    runs[0].cfg["potential"] = runs[1].cfg["potential"] = "FromFile"
    b = Recorder()
    sweep.set_up_batch(b, runs, load)
    assert seen == ["potential", "potential_sub"] and len(b.named("resample_potential")) == 1 and len(b.named("set_potsub")) == 2
