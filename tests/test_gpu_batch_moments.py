"""Moment matrices of the stored states of a batch, on the device: wafer_k_batch_moment_sums and wafer_k_batch_moment_reduce through
Batch.moments, held bit for bit (==, uint64 views) to a Context of each member's own Params holding the same states -- in a batch
of one shape and in a mixed-shape batch with state stores over the six shapes of tests/test_gpu_batch_mixed.py, members with
different k -- with what the call leaves alone, its launch counts, its refusal, and the sweep's --moments flag against wafer-hip's
`gpu.moments` section on the same files."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import moments_model as mm  # noqa: E402
from tests import ritz_model as rm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.004
MIXED_SHAPES = [(50, 50, 50), (64, 64, 64), (37, 50, 23), (130, 6, 5), (8, 8, 8), (65, 13, 3)]   # tests/test_gpu_batch_mixed.py's S
MIXED_KS = (2, 1, 4, 8, 3, 5)
ONE_SHAPE, ONE_KS = (12, 10, 9), (1, 4, 8, 2)
KK = 64   # WAFER_RITZ_MAX^2
COMBOS = [(dtype, ext) for dtype in ("f64", "f32") for ext in (1, 2, 3)]


def storage_of(dtype):
    return np.float64 if dtype == "f64" else np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


def member(wa, shape, ext, dtype, m):
    return wa.Params(*shape, dn=0.2 + 0.03 * m, dt=DT, mass=1.3 - 0.1 * m, central_difference=ext, dtype=dtype, max_states=9)


def make_batch(wa, members, states, phis):
    """a Batch (mixed with state stores where the shapes differ), no potential, states[m][j] loaded and phi uploaded"""
    mixed = len({p.work_shape for p in members}) > 1
    b = wa.Batch(members, mixed_shapes=mixed, state_stores=mixed)
    for m, ls in enumerate(states):
        for j, l in enumerate(ls):
            b.load_state(m, j, l)
        b.upload_phi(m, phis[m])
    return b


@functools.lru_cache(maxsize=None)
def measured(dtype, ext, mixed):
    """one batch: every member's moments with all listed and with two subsets listed, the raw call's output array under a NaN
    sentinel, the counts, the stores and phi afterwards; and the moments of a Context of each member's own -- computed once"""
    import wafer_amd as wa
    shapes, ks = (MIXED_SHAPES, MIXED_KS) if mixed else ([ONE_SHAPE] * len(ONE_KS), ONE_KS)
    B = len(shapes)
    members = [member(wa, shape, ext, dtype, m) for m, shape in enumerate(shapes)]
    seed = 1000 * ext + (500 if mixed else 0) + (7 if dtype == "f32" else 0)
    states = [rm.random_states(p.work_shape, ext, ks[m] + 1, seed + m, storage=storage_of(dtype)) for m, p in enumerate(members)]
    out = dict(members=members, ks=ks, states=states)
    odd = [1 if m % 2 else 0 for m in range(B)]
    with make_batch(wa, members, [s[:-1] for s in states], [s[-1] for s in states]) as b:
        assert b.num_shapes() == (6 if mixed else 1)
        out["counts"] = [b.moment_counts()]
        out["all"] = b.moments(list(ks))
        out["counts"].append(b.moment_counts())
        out["odd"] = b.moments(list(ks), active=odd)
        out["default_k"] = b.moments(active=[1] + [0] * (B - 1))            # k = None: the member's state count
        out["counts"].append(b.moment_counts())
        raw = np.full((B, 5, KK), np.nan)
        a = np.ascontiguousarray(odd, dtype=np.uint8)
        rc = b._L.wafer_batch_moment_matrices(b._h, a.ctypes.data_as(C.POINTER(C.c_uint8)), (C.c_uint32 * B)(*ks),
                                              raw.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == 0
        out["raw"] = raw
        none = np.zeros(B, dtype=np.uint8)
        assert b._L.wafer_batch_moment_matrices(b._h, none.ctypes.data_as(C.POINTER(C.c_uint8)), (C.c_uint32 * B)(*ks),
                                                raw.ctypes.data_as(C.POINTER(C.c_double))) == 0
        out["counts"].append(b.moment_counts())
        out["store"] = [[b.download_state(m, j) for j in range(ks[m])] for m in range(B)]
        out["phi"] = [b.download_phi(m) for m in range(B)]
    out["ctx"] = []
    for m, p in enumerate(members):
        with wa.Context(p) as ctx:
            for j in range(ks[m]):
                ctx.load_state(j, states[m][j])
            out["ctx"].append(ctx.moments(ks[m]))
    return out


CASES = [(dtype, ext, mixed) for dtype, ext in COMBOS for mixed in (False, True)]
IDS = ["%s-ext%d-%s" % (d, e, "mixed" if x else "one_shape") for d, e, x in CASES]


@pytest.mark.parametrize("dtype,ext,mixed", CASES, ids=IDS)
def test_every_member_gets_its_contexts_bits(dtype, ext, mixed):
    r = measured(dtype, ext, mixed)
    for m, k in enumerate(r["ks"]):
        got, want = r["all"][m], r["ctx"][m]
        assert got["origin"] == want["origin"] == mm.centres(r["members"][m].work_shape)
        for name in mm.NAMES:
            assert got[name].shape == (k, k)
            assert same(got[name], want[name]), (m, name, int(np.count_nonzero(bits(got[name]) != bits(want[name]))))
    assert same(r["default_k"][0]["r2"], r["ctx"][0]["r2"]) and all(x is None for x in r["default_k"][1:])


@pytest.mark.parametrize("dtype,ext,mixed", CASES, ids=IDS)
def test_the_listed_set_changes_nothing_and_unlisted_entries_are_not_written(dtype, ext, mixed):
    r = measured(dtype, ext, mixed)
    for m, k in enumerate(r["ks"]):
        if m % 2 == 0:
            assert r["odd"][m] is None
            assert np.all(np.isnan(r["raw"][m]))                         # the sentinel survives
            continue
        for q, name in enumerate(mm.NAMES):
            assert same(r["odd"][m][name], r["all"][m][name]), (m, name)
            assert same(r["raw"][m, q, :k * k].reshape(k, k), r["all"][m][name]), (m, name)
            assert np.all(np.isnan(r["raw"][m, q, k * k:]))


@pytest.mark.parametrize("dtype,ext,mixed", CASES, ids=IDS)
def test_counts_and_read_only(dtype, ext, mixed):
    r = measured(dtype, ext, mixed)
    # 2 launches and 1 read-back per call, for six listed members as for one; an empty list launches nothing
    assert r["counts"] == [(0, 0), (2, 1), (6, 3), (8, 4)], r["counts"]
    for m, k in enumerate(r["ks"]):
        for j in range(k):
            assert same(r["store"][m][j], r["states"][m][j]), (m, j)
        assert same(r["phi"][m], r["states"][m][-1]), m


def test_counts_for_one_member(wa):
    p = member(wa, ONE_SHAPE, 1, "f64", 0)
    states = rm.random_states(ONE_SHAPE, 1, 3, 5)
    with make_batch(wa, [p], [states[:2]], [states[2]]) as b:
        got = b.moments()
        assert b.moment_counts() == (2, 1)
    with wa.Context(p) as ctx:
        for j in range(2):
            ctx.load_state(j, states[j])
        want = ctx.moments()
    for name in mm.NAMES:
        assert same(got[0][name], want[name]), name


def test_refusals(wa):
    from wafer_amd.engine import WAFER_ERR_INVALID, WAFER_ERR_STATE
    shapes = [(12, 10, 9), (17, 17, 17)]
    members = [member(wa, s, 1, "f64", m) for m, s in enumerate(shapes)]
    phis = [rm.random_states(s, 1, 1, 3 + m)[0] for m, s in enumerate(shapes)]
    with wa.Batch(members, mixed_shapes=True) as b:                      # several shapes, no state stores
        for m in range(2):
            b.upload_phi(m, phis[m])
        raw = np.full((2, 5, KK), np.nan)
        rc = b._L.wafer_batch_moment_matrices(b._h, None, (C.c_uint32 * 2)(1, 1), raw.ctypes.data_as(C.POINTER(C.c_double)))
        msg = b._L.wafer_last_error().decode()
        assert rc == WAFER_ERR_INVALID and "mixed-shape" in msg and "wafer_batch_moment_matrices" in msg, (rc, msg)
        assert np.all(np.isnan(raw)) and b.moment_counts() == (0, 0)
        with pytest.raises(wa.WaferError, match="mixed-shape"):
            b.moments(1)
    states = [rm.random_states(s, 1, 2, 9 + m) for m, s in enumerate(shapes)]
    with make_batch(wa, members, states, phis) as b:
        raw = np.full((2, 5, KK), np.nan)
        for ks, code, who in (((2, 3), WAFER_ERR_STATE, "member 1"), ((0, 2), WAFER_ERR_INVALID, "member 0"), ((2, 9), WAFER_ERR_INVALID, "member 1")):
            rc = b._L.wafer_batch_moment_matrices(b._h, None, (C.c_uint32 * 2)(*ks), raw.ctypes.data_as(C.POINTER(C.c_double)))
            msg = b._L.wafer_last_error().decode()
            assert rc == code and who in msg, (ks, rc, msg)
        assert np.all(np.isnan(raw)) and b.moment_counts() == (0, 0)     # checked before any launch; nothing written
        for m in range(2):
            for j in range(2):
                assert same(b.download_state(m, j), states[m][j])


# ---- the sweep's --moments flag ---------------------------------------------------------------------------------------------------------------
YAML = """project_name: {name}
grid:
    size:
        x: 20
        y: 20
        z: 20
    dn: 0.5
    dt: {dt}
tolerance: 1e-7
central_difference: ThreePoint
max_steps: 200000
wavenum: 0
wavemax: {wavemax}
potential: Harmonic
mass: 1.0
init_condition: Boolean
sig: 1.0
init_symmetry: NotConstrained
output:
    screen_update: 100
    file_type: Csv
    save_wavefns: false
    save_potential: false
"""
SWEEP_RUNS = [("one", 0.04, 1), ("two", 0.03, 2)]


@pytest.fixture(scope="module")
def swept(tmp_path_factory):
    """the two runs as one sweep without and with --moments (the same seed), and each file alone through wafer-hip with
    `gpu.moments: true` -> (the sweeps' stdout per variant, wafer-hip's stdout per run).  The excited states start from files, as in
    tests/test_gpu_sweep.py: a clone of the state below is reduced to rounding noise by Gram-Schmidt, so the sweep and the driver
    would start them from different noise and end in different mixtures of the degenerate shell.  The files are the states a first
    wafer-hip run (another dt) saved, in the driver's own Csv."""
    import shutil
    from wafer_amd import build
    tmp = str(tmp_path_factory.mktemp("sweep"))

    def driver(config, d):
        r = subprocess.run([build.CLI, "-c", config, "--output-dir", os.path.join(d, "out"), "--input-dir", os.path.join(d, "input")],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        (od,) = os.listdir(os.path.join(d, "out"))
        return r.stdout, os.path.join(d, "out", od)

    d = os.path.join(tmp, "starts")
    os.makedirs(d)
    with open(os.path.join(d, "wafer.yaml"), "w") as f:
        f.write(YAML.format(name="starts", dt=0.035, wavemax=2).replace("save_wavefns: false", "save_wavefns: true"))
    _, starts = driver(os.path.join(d, "wafer.yaml"), d)
    configs, cli = [], []
    for name, dt, wavemax in SWEEP_RUNS:
        d = os.path.join(tmp, name)
        os.makedirs(os.path.join(d, "input"))
        for w in range(1, wavemax + 1):
            shutil.copy(os.path.join(starts, f"wavefunction_{w}.csv"), os.path.join(d, "input", f"wavefunction_{w}.csv"))
        text = YAML.format(name=name, dt=dt, wavemax=wavemax)
        with open(os.path.join(d, "wafer.yaml"), "w") as f:
            f.write(text)
        configs += ["-c", os.path.join(d, "wafer.yaml")]
        with open(os.path.join(d, "with_key.yaml"), "w") as f:
            f.write(text + "gpu:\n    moments: true\n")
        cli.append(driver(os.path.join(d, "with_key.yaml"), d)[0])
    out = {}
    for variant, extra in (("plain", []), ("moments", ["--moments"])):
        r = subprocess.run([sys.executable, "-m", "wafer_amd.sweep", *configs, "--output-dir", os.path.join(tmp, "out_" + variant), "--seed", "7",
                            *extra], capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr
        out[variant] = r.stdout
    return out, cli


def test_sweep_without_the_flag_knows_no_moments(swept):
    out, _ = swept
    assert "moments" not in out["plain"].lower()
    for a, b in zip(out["plain"].splitlines()[:2], out["moments"].splitlines()[:2]):
        plain, flagged = json.loads(a), json.loads(b)
        assert "moments" not in plain and sorted(flagged["moments"]) == sorted(mm.NAMES)
        flagged.pop("moments")
        plain.pop("directory")
        flagged.pop("directory")
        assert plain == flagged                                          # the flag adds the key and changes nothing else


def test_sweep_with_the_flag_agrees_with_the_driver(swept):
    """each run's "moments" against the Moments section wafer-hip prints for the same file.  The comparison is the one the sweep's
    excited states are held to against a solve of the file alone (tests/test_gpu_sweep.py: r to rel 1e-7), taken relative to the
    matrix's largest entry: entries that vanish by symmetry have no scale of their own.  (wafer-hip prints 11 digits.)"""
    out, cli = swept
    for i, (name, dt, wavemax) in enumerate(SWEEP_RUNS):
        k = wavemax + 1
        got = json.loads(out["moments"].splitlines()[i])["moments"]
        lines = cli[i].splitlines()
        at = lines.index("Moments")
        rows = [l.split() for l in lines[at + 1:at + 1 + k * (k + 1) // 2]]
        assert lines[at + 1 + k * (k + 1) // 2] == ""
        want = {n: np.zeros((k, k)) for n in mm.NAMES}
        for row in rows:
            a, b = int(row[0]), int(row[1])
            assert a <= b and len(row) == 7
            for q, n in enumerate(mm.NAMES):
                want[n][a, b] = want[n][b, a] = float(row[2 + q])
        for n in mm.NAMES:
            g = np.array(got[n])
            assert g.shape == (k, k) and np.array_equal(g, g.T)
            print(name, n, float(np.max(np.abs(g - want[n]))), float(np.max(np.abs(want[n]))))
            assert np.all(np.abs(g - want[n]) <= 1e-7 * np.max(np.abs(want[n]))), (name, n, g, want[n])
        assert np.all(np.diag(want["r2"]) > np.diag(want["s"]))            # states some cells wide
