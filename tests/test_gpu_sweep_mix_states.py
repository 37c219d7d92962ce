"""python -m wafer_amd.sweep --mix-states on the MI355X: excited-state runs of two grid shapes in ONE mixed-shape batch with state
stores give, run for run, the files the default grouping (one batch per shape) gives."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_sweep import EXCITED, run_sweep, write_run  # noqa: E402

# tests/test_gpu_sweep.py's two excited runs, and the same pair on a second shape
SIZES = [(20, 20, 20), (20, 20, 20), (24, 24, 24), (24, 24, 24)]   # cubes: the first excited level stays exactly degenerate, no phase crawls
RUNS = [dict(EXCITED[k % 2], size=SIZES[k]) for k in range(4)]


@pytest.fixture(scope="module")
def sweep():
    from wafer_amd import sweep
    return sweep


def inputs_of(k):
    """fresh O(1) starts for states 1 and 2, as tests/test_gpu_sweep.py's excited_inputs, framed for run k's shape"""
    out = {}
    for w in (1, 2):
        phi = np.zeros(tuple(n + 2 for n in SIZES[k]))
        phi[1:-1, 1:-1, 1:-1] = np.random.default_rng(10 * k + w).standard_normal(SIZES[k])
        out[f"wavefunction_{w}"] = phi
    return out


def test_mix_states_gives_the_files_of_the_default_grouping(sweep, tmp_path, capsys):
    paths = [write_run(tmp_path, f"run{k}", inputs=inputs_of(k), **RUNS[k]) for k in range(4)]
    cfgs = [sweep.load_config(p) for p in paths]
    plan = sweep.plan_batches(cfgs, mix_states=True)
    assert [(b["members"], b["needs_states"], b["mixed_shapes"], b["shapes"]) for b in plan] == [([0, 1, 2, 3], True, True, [[20, 20, 20], [24, 24, 24]])]
    assert [b["members"] for b in sweep.plan_batches(cfgs)] == [[0, 1], [2, 3]]
    rc1, lines1, dirs1 = run_sweep(sweep, capsys, paths, tmp_path / "mixed", "--progress", "--mix-states")
    rc0, lines0, dirs0 = run_sweep(sweep, capsys, paths, tmp_path / "default", "--progress")
    assert all(l["batch"] == 0 and l["batch_members"] == [0, 1, 2, 3] and l["mixed_shapes"] for l in lines1)
    assert [l["batch"] for l in lines0] == [0, 0, 1, 1] and not any(l["mixed_shapes"] for l in lines0)
    assert rc1 == 0 and rc0 == 0
    for k in range(4):
        assert lines1[k]["states"] == lines0[k]["states"] and lines1[k]["converged"] == lines0[k]["converged"], k
        assert len(lines1[k]["states"]) == 3, k
        names = sorted(n for n in os.listdir(dirs0[k]))
        assert names == sorted(os.listdir(dirs1[k])), k
        assert "table.txt" in names and "observables_2.json" in names and "wavefunction_2.npy" in names, names
        for n in names:
            a, b = open(os.path.join(dirs0[k], n), "rb").read(), open(os.path.join(dirs1[k], n), "rb").read()
            if n == "table.txt":   # (its last lines carry the wall-clock time and the output directory)
                strip = lambda t: [l for l in t.decode().splitlines() if "Elapsed" not in l and "directory" not in l.lower()]  # noqa: E731
                assert strip(a) == strip(b), (k, n)
            else:
                assert a == b, (k, n)
