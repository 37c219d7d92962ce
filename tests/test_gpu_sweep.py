"""python -m wafer_amd.sweep on the MI355X: many wafer.yaml files through batches, each run's table.txt, observables and
wavefunction against a Context (and once the native driver) solving the same file alone."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "golden", "cli_case.yaml")
CLI = os.path.join(ROOT, "wafer_amd", "wafer-hip")


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


@pytest.fixture(scope="module")
def sweep():
    from wafer_amd import sweep
    return sweep


# ---- configs: text edits of the golden case -----------------------------------------------------------------------------------
def yaml_text(size=(20, 20, 20), dtype=None, snap_update=None, **kw):
    """tests/golden/cli_case.yaml with the given keys replaced (every key must be in the file)"""
    t = open(CASE).read()
    kw = dict(dict(wavemax=0, save_potential="false"), **kw)
    for axis, n in zip("xyz", size):
        t, k = re.subn(rf"(?m)^(\s+{axis}:) \S+", rf"\g<1> {n}", t)
        assert k == 1
    for key, val in kw.items():
        t, k = re.subn(rf"(?m)^(\s*{key}:) [^#\n]+", rf"\g<1> {val} ", t)
        assert k == 1, key
    if snap_update is not None:
        t, k = re.subn(r"(?m)^(\s*)# snap_update: \S+", rf"\g<1>snap_update: {snap_update}", t)
        assert k == 1
    if dtype is not None:
        t += f"\ngpu:\n    dtype: {dtype}\n"
    return t


def write_run(tmp_path, name, inputs=None, **kw):
    """tmp_path/name/wafer.yaml, with framed arrays in tmp_path/name/input/<stem>.npy"""
    d = tmp_path / name
    d.mkdir()
    (d / "wafer.yaml").write_text(yaml_text(**kw))
    if inputs:
        (d / "input").mkdir()
        for stem, arr in inputs.items():
            np.save(d / "input" / f"{stem}.npy", arr)
    return str(d / "wafer.yaml")


def run_sweep(sweep, capsys, paths, out, *extra):
    """the sweep in this process -> (exit code, the JSON line of every run, every run's directory)"""
    capsys.readouterr()
    argv = ["--output-dir", str(out), "--seed", "7", *extra]
    for p in paths:
        argv += ["-c", p]
    rc = sweep.main(argv)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["index"] for l in lines] == list(range(len(paths)))
    for i, l in enumerate(lines):
        assert l["config"] == paths[i] and os.path.basename(l["directory"]).startswith(f"{i:03d}_cli_test_,35,1_")
        assert open(os.path.join(l["directory"], "wafer.yaml")).read() == open(paths[i]).read()
    return rc, lines, [l["directory"] for l in lines]


# ---- the reference: a Context solving one config alone --------------------------------------------------------------------------
def context_solve(wa, sweep, path, progress=True, inputs=None):
    """-> (table text, finals per state, phi per state (work area), rows per state, converged per state): Context.solve_state per
    state, printed through wafer_amd.run's formatting functions as wafer_amd.run prints"""
    c = sweep.load_config(path)
    e = c["central_difference"]
    par = wa.Params(c["nx"], c["ny"], c["nz"], dn=c["dn"], dt=c["dt"], mass=c["mass"], sig=c["sig"], central_difference=e,
                    dtype=c["dtype"], max_states=c["wavemax"] + 1)
    text, finals, phis, all_rows, convs = [], [], [], [], []
    with wa.Context(par) as ctx:
        ctx.set_potential(c["potential"])
        for w in range(c["wavemax"] + 1):
            if w == 0:
                ctx.set_initial_condition(c["init_condition"], seed=7)
            else:
                ctx.upload_phi(inputs[f"wavefunction_{w}"])
            rows, fin, conv = ctx.solve_state(w, c["tolerance"], c["screen_update"], c["max_steps"])
            text.append(sweep.observable_header(w))
            shown = rows if progress else rows[-1:] if conv else []
            text += [sweep.measurement_row(r["tau"], r["diff"], r) for r in shown]
            if conv:
                text.append(sweep.summary(fin))
            finals.append(fin)
            phis.append(ctx.download_phi()[e:-e, e:-e, e:-e])
            all_rows.append(rows)
            convs.append(conv)
            if not conv:
                break
    return "".join(l + "\n" for l in text), finals, phis, all_rows, convs


def check_ground_run(wa, sweep, path, directory, line, progress=True):
    """a ground-state run of the sweep against its Context: text, observables and wavefunction, value for value"""
    text, finals, phis, rows, convs = context_solve(wa, sweep, path, progress)
    assert open(os.path.join(directory, "table.txt")).read() == text
    st = line["states"]
    assert len(st) == 1 and st[0]["state"] == 0 and st[0]["steps"] == rows[0][-1]["step"]
    assert st[0]["status"] == ("Converged" if convs[0] else "MaxStep") and line["converged"] == convs[0]
    if convs[0]:
        assert json.load(open(os.path.join(directory, "observables_0.json"))) == finals[0]
        assert st[0]["energy"] == finals[0]["energy"]
        assert np.array_equal(np.load(os.path.join(directory, "wavefunction_0.npy")), phis[0])
        assert not os.path.exists(os.path.join(directory, "wavefunction_0_partial.npy"))
    else:
        assert not os.path.exists(os.path.join(directory, "observables_0.json"))
        assert np.array_equal(np.load(os.path.join(directory, "wavefunction_0_partial.npy")), phis[0])
    return rows[0], convs[0]


# ---- 6. ground states, mixed shapes, per-run controls ---------------------------------------------------------------------------
GROUND = [   # sizes, potentials, dn, dt, mass, screen_update and tolerance all differ; run 3 passes its max_steps
    dict(size=(20, 20, 20), potential="Harmonic", dn=0.5, dt=0.04, mass=1.0, init_condition="Boolean", screen_update=10, tolerance="1e-7"),
    dict(size=(16, 20, 12), potential="Harmonic", dn=0.6, dt=0.05, mass=1.0, init_condition="Constant", screen_update=25, tolerance="1e-8"),
    dict(size=(24, 24, 24), potential="Coulomb", dn=0.4, dt=0.03, mass=1.0, init_condition="Boolean", screen_update=40, tolerance="1e-6"),
    dict(size=(20, 20, 20), potential="Coulomb", dn=0.45, dt=0.02, mass=2.0, init_condition="Constant", screen_update=10, tolerance="1e-12",
         max_steps=55),
    dict(size=(20, 20, 20), potential="Harmonic", dn=0.4, dt=0.025, mass=1.5, init_condition="Boolean", screen_update=25, tolerance="1e-9"),
]


@pytest.mark.parametrize("dtypes", [("f64",) * 5, ("f64", "f32", "f64", "f64", "f32")])
def test_ground_states_of_mixed_shapes_with_their_own_controls(wa, sweep, tmp_path, capsys, dtypes):
    paths = [write_run(tmp_path, f"run{k}", dtype=None if dtypes[k] == "f64" else dtypes[k], **GROUND[k]) for k in range(5)]
    rc, lines, dirs = run_sweep(sweep, capsys, paths, tmp_path / "out", "--progress")
    assert rc == 1                                              # run 3 reaches its max_steps
    groups = [[k for k in range(5) if dtypes[k] == d] for d in ("f64", "f32") if d in dtypes]
    for members in groups:                                      # one mixed batch per dtype
        for k in members:
            assert lines[k]["batch_members"] == members and lines[k]["mixed_shapes"], k
    assert len({l["batch"] for l in lines}) == len(groups)
    assert sweep.plan_batches([sweep.load_config(p) for p in paths]) == \
        [dict(members=m, central_difference=1, dtype=d, needs_states=False, mixed_shapes=True,
              shapes=[list(s) for s in dict.fromkeys(GROUND[k]["size"] for k in m)]) for m, d in zip(groups, ("f64", "f32"))]
    steps = []
    for k in range(5):
        rows, conv = check_ground_run(wa, sweep, paths[k], dirs[k], lines[k])
        assert conv == (k != 3), k
        su = GROUND[k]["screen_update"]
        assert [r["step"] for r in rows] == list(range(0, rows[-1]["step"] + 1, su))
        steps.append(rows[-1]["step"])
    assert lines[3]["states"][0]["status"] == "MaxStep" and steps[3] == 60
    for members in groups:   # one launch per step for ALL runs of a batch: as many as the longest run took, not the sum
        assert lines[members[0]]["fused_passes"] == 0
        assert lines[members[0]]["single_steps"] == max(steps[k] for k in members), (steps, members)


# ---- 7. the native driver's text, once ------------------------------------------------------------------------------------------
def test_table_is_the_native_drivers_stdout(sweep, tmp_path, capsys):
    paths = [write_run(tmp_path, f"run{k}", **GROUND[k]) for k in (0, 1)]
    rc, lines, dirs = run_sweep(sweep, capsys, paths, tmp_path / "out", "--progress")
    assert rc == 0
    r = subprocess.run([CLI, "-c", paths[1], "--progress", "--output-dir", str(tmp_path / "native"), "--input-dir", str(tmp_path / "none")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = r.stdout[:r.stdout.index("Simulation complete")]
    assert open(os.path.join(dirs[1], "table.txt")).read() == want


# ---- 8. symmetry ----------------------------------------------------------------------------------------------------------------
SYM = [
    # The reference's mirror lies half a cell off the potential's centre, so a run that symmetrises at every second block never
    # settles: its energy alternates (by 0.17 here) between the block after a snapshot and the one before the next.  Its tolerance
    # is one such a run can meet -- at step 60, after the snapshot blocks 0 and 40; 1e-7, with max_steps, makes the run that stops.
    dict(size=(20, 16, 18), potential="Harmonic", dn=0.5, dt=0.04, init_condition="Constant", init_symmetry="AntisymAboutZ",
         screen_update=20, snap_update=40, tolerance="0.2"),
    dict(size=(20, 16, 18), potential="Harmonic", dn=0.5, dt=0.03, init_condition="Boolean", init_symmetry="AboutY",
         screen_update=25, tolerance="1e-7"),
    dict(size=(15, 21, 17), potential="Harmonic", dn=0.5, dt=0.04, init_condition="Coulomb", init_symmetry="NotConstrained",   # (odd sizes: the Coulomb start has no cell at r = 0)
         screen_update=30, tolerance="1e-7"),
]


def context_loop(wa, sweep, path):
    """wafer_cli.cpp:659-719 on a Context: symmetrise at the start and at the snapshot blocks -> (table text, final, phi, steps, converged)"""
    c = sweep.load_config(path)
    e = c["central_difference"]
    par = wa.Params(c["nx"], c["ny"], c["nz"], dn=c["dn"], dt=c["dt"], mass=c["mass"], sig=c["sig"], central_difference=e, dtype=c["dtype"])
    text = [sweep.observable_header(0)]
    with wa.Context(par) as ctx:
        ctx.set_potential(c["potential"])
        ctx.set_initial_condition(c["init_condition"], seed=7)
        ctx.symmetrise(c["init_symmetry"])
        step, last, converged = 0, sys.float_info.max, False
        while True:
            obs = ctx.observables()
            ne = obs["energy"] / obs["norm2"]
            ctx.normalise(obs["norm2"])
            if c["snap_update"] is not None and step % c["snap_update"] == 0:
                ctx.symmetrise(c["init_symmetry"])
            diff = abs(ne - last)
            if diff < c["tolerance"]:
                text.append(sweep.measurement_row(step * c["dt"], diff, obs))
                converged = True
                break
            text.append(sweep.measurement_row(step * c["dt"], diff, obs))
            last = ne
            if c["max_steps"] is not None and step > c["max_steps"]:
                break
            ctx.evolve(0, c["screen_update"])
            step += c["screen_update"]
        r = math.sqrt(obs["r2"] / obs["norm2"])
        fin = dict(state=0, energy=ne, binding_energy=(obs["energy"] - obs["v_infinity"]) / obs["norm2"], r=r, l_r=c["nx"] / r)
        if converged:
            text.append(sweep.summary(fin))
        return "".join(l + "\n" for l in text), fin, ctx.download_phi()[e:-e, e:-e, e:-e], step, converged


@pytest.mark.parametrize("stop_early", [False, True])
def test_symmetry_constraints_at_the_start_and_at_snapshot_blocks(wa, sweep, tmp_path, capsys, stop_early):
    extra = dict(max_steps=70, tolerance="1e-7") if stop_early else {}
    paths = [write_run(tmp_path, f"run{k}", central_difference="SevenPoint", **dict(SYM[k], **(extra if k == 0 else {}))) for k in range(3)]
    rc, lines, dirs = run_sweep(sweep, capsys, paths, tmp_path / "out", "--progress")
    assert rc == (1 if stop_early else 0)
    assert all(l["batch_members"] == [0, 1, 2] for l in lines)
    for k in range(3):
        text, fin, phi, step, conv = context_loop(wa, sweep, paths[k])
        assert conv == (not (stop_early and k == 0)), k
        assert open(os.path.join(dirs[k], "table.txt")).read() == text, k
        assert lines[k]["states"][0]["steps"] == step and lines[k]["states"][0]["energy"] == fin["energy"]
        name = "wavefunction_0.npy" if conv else "wavefunction_0_partial.npy"
        assert np.array_equal(np.load(os.path.join(dirs[k], name)), phi), k
        if conv:
            assert json.load(open(os.path.join(dirs[k], "observables_0.json"))) == fin
            assert not os.path.exists(os.path.join(dirs[k], "wavefunction_0_partial.npy"))   # removed on convergence
    if not stop_early:
        assert step_of(lines[0]) == 60   # the snapshot blocks 0 and 40, and one more
    else:   # the run that stopped keeps its partial file: the symmetrised wavefunction of its last block
        assert step_of(lines[0]) == 80 and os.path.exists(os.path.join(dirs[0], "wavefunction_0_partial.npy"))
        # step 80 is a snapshot block: what was saved is antisymmetric about the reference's mirror (work plane k <-> n - 2 - k;
        # plane 8 mirrors onto itself and only changes sign, the last work plane mirrors onto the frame)
        p0 = np.load(os.path.join(dirs[0], "wavefunction_0_partial.npy"))
        lower, upper = p0[:, :, :8], p0[:, :, 16:8:-1]
        assert lower.any() and np.array_equal(lower, -upper) and not p0[:, :, 17].any()


def step_of(line):
    return line["states"][0]["steps"]


# ---- 9. excited states ----------------------------------------------------------------------------------------------------------
# Two 20^3 Harmonic runs to the second excited state that differ in dt and screen_update.  The tolerances lie, for all three states
# of the Context run, at least a factor of two below the last difference that is above them and above the first that is below
# (check_excited_run asserts it): blocks this long shrink the difference 60- and 130-fold, so the sweep's other summation order
# cannot move the stopping step.
EXCITED = [
    dict(size=(20, 20, 20), potential="Harmonic", dn=0.4, dt=0.04, init_condition="Boolean", screen_update=50, tolerance="1.4e-8", wavemax=2),
    dict(size=(20, 20, 20), potential="Harmonic", dn=0.4, dt=0.03, init_condition="Constant", screen_update=80, tolerance="4.7e-9", wavemax=2),
]


def excited_inputs(k):
    """fresh O(1) starts for states 1 and 2 (the clone of the state below, reduced to rounding noise by Gram-Schmidt, would start
    the sweep and the Context from different noise): framed arrays for the run's input directory"""
    out = {}
    for w in (1, 2):
        phi = np.zeros((22, 22, 22))
        phi[1:-1, 1:-1, 1:-1] = np.random.default_rng(10 * k + w).standard_normal((20, 20, 20))
        out[f"wavefunction_{w}"] = phi
    return out


def check_excited_run(wa, sweep, path, directory, line, inputs):
    text, finals, phis, rows, convs = context_solve(wa, sweep, path, inputs=inputs)
    tol = sweep.load_config(path)["tolerance"]
    assert convs == [True, True, True]
    for w in range(3):   # the precondition: the Context's stopping step is not within a factor of two of the tolerance
        print(path, "state", w, "diffs", [r["diff"] for r in rows[w][-3:]], "tolerance", tol)
        assert rows[w][-1]["diff"] < tol / 2 and rows[w][-2]["diff"] > 2 * tol, (w, rows[w][-2]["diff"], rows[w][-1]["diff"])
    got = open(os.path.join(directory, "table.txt")).read()
    blocks = got.split("caclulation")[1:]
    assert len(blocks) == 3
    for w in range(3):
        got_rows = [l for l in blocks[w].splitlines() if re.match(r"^\s+│\s*[0-9.]+ │", l)]
        assert len(got_rows) == len(rows[w]), w
        for l, r in zip(got_rows, rows[w]):
            cols = [c.strip() for c in l.split("│")[1:5]]
            assert cols[0] == f"{r['tau']:.3f}"
            assert float(cols[1]) == pytest.approx(r["energy"] / r["norm2"], abs=2e-9)
            assert float(cols[2]) == pytest.approx(math.sqrt(r["r2"] / r["norm2"]), rel=1e-7, abs=1e-5)   # (printed to 5 decimals)
        obs = json.load(open(os.path.join(directory, f"observables_{w}.json")))
        assert obs["state"] == w and obs["energy"] == pytest.approx(finals[w]["energy"], abs=2e-9)
        assert obs["r"] == pytest.approx(finals[w]["r"], rel=1e-7)
        assert line["states"][w] == dict(state=w, status="Converged", steps=rows[w][-1]["step"], energy=obs["energy"])
        assert np.load(os.path.join(directory, f"wavefunction_{w}.npy")).shape == (20, 20, 20)
    e = [json.load(open(os.path.join(directory, f"observables_{w}.json")))["energy"] for w in range(3)]
    assert e[0] == pytest.approx(1.5, abs=0.02) and e[1] == pytest.approx(2.5, abs=0.04) and e[2] == pytest.approx(2.5, abs=0.04)


def test_excited_states_in_a_one_shape_batch(wa, sweep, tmp_path, capsys):
    inputs = [excited_inputs(k) for k in range(2)]
    paths = [write_run(tmp_path, f"run{k}", inputs=inputs[k], **EXCITED[k]) for k in range(2)]
    rc, lines, dirs = run_sweep(sweep, capsys, paths, tmp_path / "out", "--progress")
    assert rc == 0
    assert all(l["batch_members"] == [0, 1] and not l["mixed_shapes"] and l["converged"] for l in lines)
    for k in range(2):
        check_excited_run(wa, sweep, paths[k], dirs[k], lines[k], inputs[k])


# ---- 10. a run that needs states beside runs that do not --------------------------------------------------------------------------
def test_state_run_beside_ground_runs_of_other_shapes(wa, sweep, tmp_path, capsys):
    inputs = excited_inputs(0)
    paths = [write_run(tmp_path, "run0", **GROUND[1]), write_run(tmp_path, "run1", inputs=inputs, **EXCITED[0]),
             write_run(tmp_path, "run2", **GROUND[2])]
    plan = sweep.plan_batches([sweep.load_config(p) for p in paths])
    assert [(b["members"], b["mixed_shapes"], b["needs_states"]) for b in plan] == [([0, 2], True, False), ([1], False, True)]
    rc, lines, dirs = run_sweep(sweep, capsys, paths, tmp_path / "out", "--progress")
    assert rc == 0 and [l["batch"] for l in lines] == [0, 1, 0]
    for k in (0, 2):
        assert check_ground_run(wa, sweep, paths[k], dirs[k], lines[k])[1]
    check_excited_run(wa, sweep, paths[1], dirs[1], lines[1], inputs)
