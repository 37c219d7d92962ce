"""python -m wafer_amd.run on one rank with a potential_sub array of another resolution: it is resampled onto the grid
(Context.set_potsub_resampled, input::fill_sub_data) instead of refused, and the run's observables are those of a Context set up the
same way."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_sweep import yaml_text  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_potential_sub_of_another_resolution_is_resampled(tmp_path):
    import wafer_amd
    from wafer_amd import sweep
    path = tmp_path / "wafer.yaml"
    path.write_text(yaml_text(size=(24, 20, 28), potential="FullCornell", init_condition="Boolean", screen_update=10, tolerance="1e-3",
                              max_steps=600, save_wavefns="false"))
    inp = tmp_path / "input"
    inp.mkdir()
    sub = 4.0 + np.random.default_rng(3).random((7, 9, 5))
    np.save(inp / "potential_sub.npy", sub)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "-m", "wafer_amd.run", "-c", str(path), "--output-dir", str(tmp_path / "out"), "--input-dir", str(inp)],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Potential_sub loaded from disk" in r.stderr and "resample it once" not in r.stderr
    (out,) = os.listdir(tmp_path / "out")
    got = json.load(open(tmp_path / "out" / out / "observables_0.json"))
    c = sweep.load_config(str(path))
    par = wafer_amd.Params(c["nx"], c["ny"], c["nz"], dn=c["dn"], dt=c["dt"], mass=c["mass"], sig=c["sig"],
                           central_difference=c["central_difference"], dtype=c["dtype"], max_states=c["wavemax"] + 1)
    with wafer_amd.Context(par) as ctx:
        ctx.set_potential("FullCornell")
        ctx.set_potsub_resampled(sub)
        ctx.set_initial_condition("Boolean")
        rows, fin, conv = ctx.solve_state(0, c["tolerance"], c["screen_update"], c["max_steps"])
        assert conv
        plain = dict(fin)
    with wafer_amd.Context(par) as ctx:   # without the file the binding energy is another: the array was used
        ctx.set_potential("FullCornell")
        ctx.set_initial_condition("Boolean")
        _, other, _ = ctx.solve_state(0, c["tolerance"], c["screen_update"], c["max_steps"])
    assert got == plain and got["energy"] == other["energy"] and got["binding_energy"] != other["binding_energy"]
