"""python -m wafer_amd.sweep with a potential file of another resolution on the MI355X: runs at (24, 20, 28) and (16, 20, 28) read
ONE `potential` file through --input-dir; it is resampled for them in one Batch.resample_potential call (copied for a run whose own
size it has), and each run's table, observables and wavefunction equal a Context that solved its file with
set_potential_resampled."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_sweep import run_sweep, yaml_text  # noqa: E402

RUNS = [   # a few hundred steps at the most: max_steps is fixed
    dict(size=(24, 20, 28), dn=0.5, dt=0.04, mass=1.0, init_condition="Boolean", screen_update=10, tolerance="1e-6", max_steps=300),
    dict(size=(16, 20, 28), dn=0.6, dt=0.05, mass=1.0, init_condition="Constant", screen_update=25, tolerance="1e-6", max_steps=300),
    dict(size=(24, 20, 28), dn=0.5, dt=0.03, mass=1.5, init_condition="Boolean", screen_update=20, tolerance="1e-9", max_steps=90),
]


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


@pytest.fixture(scope="module")
def sweep():
    from wafer_amd import sweep
    return sweep


def well(shape):
    """a harmonic well on a box of 12 x 10 x 14 length units, sampled on `shape` points, with a ripple that no mirror keeps"""
    ax = [np.linspace(-l / 2, l / 2, n) for l, n in zip((12.0, 10.0, 14.0), shape)]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    return 0.5 * (x * x + y * y + z * z) + 0.05 * np.sin(1.3 * x + 0.7 * y - 0.4 * z)


def write_csv(path, a):
    """output.rs:148-165: i,j,k,data without a header"""
    with open(path, "w") as f:
        for (i, j, k), v in np.ndenumerate(a):
            f.write(f"{i},{j},{k},{float(v)!r}\n")


def context_ground(wa, sweep, path, src):
    """the run of `path` on a Context: V from `src` -- copied into the zero frame if it has the run's size, else resampled as
    wafer-hip resamples it -- then Context.solve_state, printed as wafer_amd.run prints -> (table, final, phi, rows, converged)"""
    c = sweep.load_config(path)
    e = c["central_difference"]
    par = wa.Params(c["nx"], c["ny"], c["nz"], dn=c["dn"], dt=c["dt"], mass=c["mass"], sig=c["sig"], central_difference=e, dtype=c["dtype"],
                    max_states=c["wavemax"] + 1)
    with wa.Context(par) as ctx:
        if src.shape == par.work_shape:
            v = np.zeros(par.padded_shape)
            v[e:-e, e:-e, e:-e] = src
            ctx.set_potential_host(v)
        else:
            ctx.set_potential_resampled(np.ascontiguousarray(src))
        ctx.set_initial_condition(c["init_condition"], seed=7)
        rows, fin, conv = ctx.solve_state(0, c["tolerance"], c["screen_update"], c["max_steps"])
        text = [sweep.observable_header(0)] + [sweep.measurement_row(r["tau"], r["diff"], r) for r in rows]
        if conv:
            text.append(sweep.summary(fin))
        return "".join(l + "\n" for l in text), fin, ctx.download_phi()[e:-e, e:-e, e:-e], rows, conv


@pytest.mark.parametrize("file_shape,copied", [((12, 10, 14), []), ((16, 20, 28), [1])], ids=["resampled-for-all", "copied-for-one"])
def test_one_potential_file_for_runs_of_other_resolutions(wa, sweep, tmp_path, capsys, monkeypatch, file_shape, copied):
    paths = []
    for k, spec in enumerate(RUNS):
        d = tmp_path / f"run{k}"
        d.mkdir()
        (d / "wafer.yaml").write_text(yaml_text(potential="FromFile", **spec))
        paths.append(str(d / "wafer.yaml"))
    inp = tmp_path / "input"
    inp.mkdir()
    src = well(file_shape)
    write_csv(inp / "potential.csv", src)
    calls = []
    real = wa.Batch.resample_potential
    monkeypatch.setattr(wa.Batch, "resample_potential",
                        lambda self, s, active=None, basis="padded": (calls.append((s.shape, list(active), basis)), real(self, s, active, basis))[1])
    rc, lines, dirs = run_sweep(sweep, capsys, paths, tmp_path / "out", "--progress", "--input-dir", str(inp))
    assert calls == [(file_shape, [0 if k in copied else 1 for k in range(3)], "padded")]   # one call for the whole batch
    assert all(l["batch_members"] == [0, 1, 2] and l["mixed_shapes"] for l in lines)
    plan = sweep.plan_inputs([sweep.Run(i, sweep.load_config(p), p, str(inp)) for i, p in enumerate(paths)])
    assert [(g["role"], g["members"], g["copy"]) for g in plan] == [("potential", [0, 1, 2], copied)]
    convs = []
    for k in range(3):
        text, fin, phi, rows, conv = context_ground(wa, sweep, paths[k], src)
        convs.append(conv)
        assert open(os.path.join(dirs[k], "table.txt")).read() == text, k
        st = lines[k]["states"]
        assert len(st) == 1 and st[0]["steps"] == rows[-1]["step"] and st[0]["status"] == ("Converged" if conv else "MaxStep"), k
        if conv:
            assert json.load(open(os.path.join(dirs[k], "observables_0.json"))) == fin, k
            assert st[0]["energy"] == fin["energy"]
            assert np.array_equal(np.load(os.path.join(dirs[k], "wavefunction_0.npy")), phi), k
        else:
            assert np.array_equal(np.load(os.path.join(dirs[k], "wavefunction_0_partial.npy")), phi), k
        assert rows[-1]["step"] <= 320, k
    assert convs[2] is False and any(convs[:2])        # run 2 stops at its max_steps; the sweep's exit code says so
    assert rc == 1
