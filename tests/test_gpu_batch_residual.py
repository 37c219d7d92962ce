"""Residuals on a batch, on the device: wafer_k_batch_residual_sums and wafer_k_batch_residual_reduce through Batch.residuals, held
bit for bit (==, uint64 views) to a Context of each member's own Params with the same potential, states and phi -- both theta
modes, both sources, one shape, several shapes with state stores, and several shapes without (the phi source only) -- then launch
counts, masks, a member without a Rayleigh quotient, refusals, and the sweep's --residuals flag.

Member sets are those of tests/test_gpu_batch_ritz.py: members differ in dn, mass and built-in potential, so each has its own
denominator and short-form flag."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import ritz_model as rm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.004
DTYPES = ["f64", "f32", "f32fast"]
SMALL = [(3, 2, 5), (12, 10, 9), (17, 17, 17)]
POTS = ["Harmonic", "Cube", "Periodic", "NoPotential", "Harmonic"]
KM = 8   # WAFER_RITZ_MAX
COMBOS = [(dtype, ext) for dtype in DTYPES for ext in (1, 2, 3)]
NAMES = ("theta", "r2", "norm2")


def big_of(dtype):
    return (130, 20, 40) if dtype == "f64" else (258, 20, 40)


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


def member(wa, shape, ext, dtype, m, max_states=10):
    """member m's Params: its own dn and mass (dt <= dn^2 / 3 for every one of them)"""
    return wa.Params(*shape, dn=0.2 + 0.03 * m, dt=DT, mass=1.3 - 0.1 * m, central_difference=ext, dtype=dtype, max_states=max_states)


def make_batch(wa, members, pots, states, phis, stores=True):
    """a Batch (mixed where the shapes differ, with state stores unless stores is False) with potentials, states[m][j] and phi"""
    mixed = len({p.work_shape for p in members}) > 1
    b = wa.Batch(members, mixed_shapes=mixed, state_stores=mixed and stores)
    b.set_potentials(pots)
    if stores:
        for m, ls in enumerate(states):
            for j, l in enumerate(ls):
                b.load_state(m, j, l)
    for m, phi in enumerate(phis):
        b.upload_phi(m, phi)
    return b


def make_context(wa, p, pot, states, phi):
    ctx = wa.Context(p)
    ctx.set_potential(pot)
    for j, l in enumerate(states):
        ctx.load_state(j, l)
    ctx.upload_phi(phi)
    return ctx


def arrays_for(members, dtype, ext, counts, frame=True):
    """per member counts[m] states and one more array for phi"""
    out = [rm.random_states(p.work_shape, ext, n + 1, 100000 * DTYPES.index(dtype) + 1000 * ext + 10 * sum(p.work_shape) + m + 5, frame=frame,
                            storage=storage_of(dtype)) for m, (p, n) in enumerate(zip(members, counts))]
    return [a[:-1] for a in out], [a[-1] for a in out]


def thetas_for(ks):
    return [[-3.5 + m + 0.75 * j for j in range(k)] for m, k in enumerate(ks)]


def against_contexts(wa, dtype, ext, shapes, ks, stores=True):
    members = [member(wa, shape, ext, dtype, m) for m, shape in enumerate(shapes)]
    states, phis = arrays_for(members, dtype, ext, ks)
    pots = POTS[:len(members)]
    th = thetas_for(ks)
    got = {}
    with make_batch(wa, members, pots, states, phis, stores) as b:
        assert b.num_shapes() == len(set(shapes))
        if stores:
            got["s_ray"] = b.residuals(list(ks))
            got["s_given"] = b.residuals(list(ks), theta=th)
        got["p_ray"] = b.residuals(source="phi")
        got["p_given"] = b.residuals(1, theta=[t[:1] for t in th], source="phi")
    for m, p in enumerate(members):
        with make_context(wa, p, pots[m], states[m] if stores else [], phis[m]) as ctx:
            want = dict(p_ray=ctx.residuals(source="phi"), p_given=ctx.residuals(1, theta=th[m][:1], source="phi"))
            if stores:
                want.update(s_ray=ctx.residuals(ks[m]), s_given=ctx.residuals(ks[m], theta=th[m]))
        for key, w in want.items():
            assert got[key][m]["status"] == 0
            for name in NAMES + ("rho",):
                assert got[key][m][name].shape == w[name].shape
                assert same(got[key][m][name], w[name]), (key, m, name, got[key][m][name], w[name])


# ---- 1. every member's numbers are its context's ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,ext", COMBOS)
def test_one_shape_against_contexts(wa, dtype, ext):
    against_contexts(wa, dtype, ext, [(12, 10, 9)] * 3, (1, 4, 8))


@pytest.mark.parametrize("dtype,ext", COMBOS)
def test_one_shape_of_several_tiles_against_contexts(wa, dtype, ext):
    against_contexts(wa, dtype, ext, [big_of(dtype)] * 2, (2, 5))


@pytest.mark.parametrize("dtype,ext", COMBOS)
def test_mixed_shapes_with_stores_against_contexts(wa, dtype, ext):
    against_contexts(wa, dtype, ext, SMALL + [big_of(dtype)], (2, 8, 1, 4))


@pytest.mark.parametrize("dtype,ext", COMBOS)
def test_mixed_shapes_without_stores_take_the_phi_source(wa, dtype, ext):
    against_contexts(wa, dtype, ext, SMALL + [big_of(dtype)], (1, 1, 1, 1), stores=False)


# ---- 2. launch counts -----------------------------------------------------------------------------------------------------------------------
def test_launch_counts_do_not_depend_on_members_or_shapes(wa):
    dtype, ext = "f64", 1
    seen = []
    for shapes in ([(12, 10, 9)], [(12, 10, 9)] * 5, [(3, 2, 5), (12, 10, 9), (17, 17, 17), (9, 12, 14), (12, 10, 9)]):
        B = len(shapes)
        members = [member(wa, shape, ext, dtype, m) for m, shape in enumerate(shapes)]
        states, phis = arrays_for(members, dtype, ext, [3] * B)
        with make_batch(wa, members, ["Harmonic"] * B, states, phis) as b:
            counts = [b.residual_counts()]
            b.residuals(2, theta=[[1.0, 2.0]] * B)
            counts.append(b.residual_counts())
            b.residuals()
            counts.append(b.residual_counts())
            b.residuals(1, theta=[[0.5]] * B, source="phi")
            counts.append(b.residual_counts())
            b.residuals(source="phi", active=[1] + [0] * (B - 1))
            counts.append(b.residual_counts())
            b.residuals(1, active=[0] * B)                       # an empty list launches nothing
            b.residuals(source="phi", active=[0] * B)
            counts.append(b.residual_counts())
            assert b.ritz_counts() == (0, 0)
        seen.append(counts)
    assert seen[0] == [(0, 0), (2, 1), (6, 3), (8, 4), (12, 6), (12, 6)]
    assert seen[1] == seen[0] and seen[2] == seen[0]


# ---- 3. masks: what a call leaves of its arrays, and of the members -------------------------------------------------------------------------
def raw(b, source, active, ks, theta_in, sentinel=-7.25):
    """the C call itself on sentinel-filled outputs -> (rc, theta, r2, s, status)"""
    B = len(b.members)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    a = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
    th, r2, s = (np.full((B, KM), sentinel) for _ in range(3))
    st = (C.c_int * B)(*([55] * B))
    rc = b._L.wafer_batch_residuals(b._h, source, None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8)), (C.c_uint32 * B)(*ks),
                                    None if theta_in is None else dp(theta_in), dp(th), dp(r2), dp(s), st)
    return rc, th, r2, s, list(st)


@pytest.mark.parametrize("mixed", [False, True], ids=["one_shape", "mixed"])
@pytest.mark.parametrize("dtype,ext", [("f64", 1), ("f32", 2), ("f64", 3)])
def test_masks_and_members_that_are_not_listed(wa, dtype, ext, mixed):
    shapes = [(12, 10, 9), (3, 2, 5), (17, 17, 17), (12, 10, 9), big_of(dtype)] if mixed else [(17, 17, 17)] * 5
    counts = [2, 1, 4, 3, 2]
    members = [member(wa, shape, ext, dtype, m) for m, shape in enumerate(shapes)]
    states, phis = arrays_for(members, dtype, ext, counts)
    tin = np.full((5, KM), np.nan)                               # entries of members not listed, and beyond k, are not read
    for m, k in enumerate(counts):
        tin[m, :k] = thetas_for(counts)[m]
    with make_batch(wa, members, POTS, states, phis) as b:
        rc, th0, r20, s0, _ = raw(b, 0, None, counts, None)
        assert rc == 0
        for active in ([1, 1, 1, 1, 1], [0, 0, 0, 1, 0], [1, 0, 0, 1, 1], [0, 1, 1, 1, 0]):
            for theta_in in (None, tin):
                t = tin.copy()
                for m in range(5):
                    if not active[m]:
                        t[m] = np.nan
                ks = [k if a else 99 for k, a in zip(counts, active)]      # (a k that would be refused, were it read)
                rc, th, r2, s, st = raw(b, 0, active, ks, None if theta_in is None else t)
                assert rc == 0, b._L.wafer_last_error().decode()
                for m in range(5):
                    n = counts[m] if active[m] else 0
                    assert np.all(th[m, n:] == -7.25) and np.all(r2[m, n:] == -7.25) and np.all(s[m, n:] == -7.25), (active, m)
                    assert st[m] == (0 if active[m] else 55)
                    assert same(s[m, :n], s0[m, :n])
                    if theta_in is None:
                        assert same(th[m, :n], th0[m, :n]) and same(r2[m, :n], r20[m, :n]), (active, m)
                    else:
                        assert same(th[m, :n], tin[m, :n]) and not np.any(r2[m, :n] == -7.25)
        for m in range(5):                                       # read-only: every member's arrays keep every bit
            assert same(b.download_phi(m), phis[m]), m
            for j in range(counts[m]):
                assert same(b.download_state(m, j), states[m][j]), (m, j)


# ---- 4. a member without a Rayleigh quotient -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True], ids=["one_shape", "mixed"])
def test_a_zero_state_is_that_members_status(wa, mixed):
    from wafer_amd.engine import WAFER_ERR_STATE, WAFER_OK
    dtype, ext = "f64", 1
    shapes = [(12, 10, 9), (17, 17, 17), (3, 2, 5)] if mixed else [(12, 10, 9)] * 3
    members = [member(wa, shape, ext, dtype, m) for m, shape in enumerate(shapes)]
    states, phis = arrays_for(members, dtype, ext, [3, 3, 2])
    states[1][0] = np.zeros_like(states[1][0])
    with make_batch(wa, members, POTS[:3], states, phis) as b:
        rc, th, r2, s, st = raw(b, 0, None, [3, 3, 2], None)
        assert rc == WAFER_OK and st == [WAFER_OK, WAFER_ERR_STATE, WAFER_OK]
        assert "member 1" in b._L.wafer_last_error().decode()
        assert np.all(th[1] == -7.25) and np.all(r2[1] == -7.25) and np.all(s[1] == -7.25)
        res = b.residuals([3, 3, 2])
        assert res[1] == dict(theta=None, r2=None, norm2=None, rho=None, status=WAFER_ERR_STATE)
        # with theta given there is nothing to divide: the zero state has r2 = s = 0
        rc, th1, r21, s1, st1 = raw(b, 0, None, [3, 3, 2], np.ones((3, KM)))
        assert rc == WAFER_OK and st1 == [WAFER_OK] * 3 and r21[1, 0] == 0.0 and s1[1, 0] == 0.0
    for m in (0, 2):
        with make_context(wa, members[m], POTS[m], states[m], phis[m]) as ctx:
            want = ctx.residuals()
        k = len(states[m])
        assert same(th[m, :k], want["theta"]) and same(r2[m, :k], want["r2"]) and same(s[m, :k], want["norm2"]), m
        for name in NAMES:
            assert same(res[m][name], want[name]), (m, name)


# ---- 5. refusals change nothing ----------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(wa):
    from wafer_amd.engine import WAFER_ERR_INVALID, WAFER_ERR_STATE
    dtype, ext, B = "f64", 1, 3
    shapes = [(12, 10, 9), (17, 17, 17), (3, 2, 5)]
    members = [member(wa, shape, ext, dtype, m) for m, shape in enumerate(shapes)]
    states, phis = arrays_for(members, dtype, ext, [3, 3, 3])

    def refused(b, source, ks, theta_in, code, *words):
        before = b.residual_counts()
        rc, th, r2, s, st = raw(b, source, None, ks, theta_in)
        msg = b._L.wafer_last_error().decode()
        assert rc == code and all(w in msg for w in words), (rc, msg)
        assert np.all(th == -7.25) and np.all(r2 == -7.25) and np.all(s == -7.25) and st == [55] * B
        assert b.residual_counts() == before

    mixed = len(set(shapes)) > 1
    b = wa.Batch(members, mixed_shapes=mixed, state_stores=mixed)
    with b:
        b.set_potential(0, "Harmonic")
        b.set_potential(2, "Cube")
        for m in range(B):
            for j in range(3):
                b.load_state(m, j, states[m][j])
        refused(b, 1, [1, 1, 1], None, WAFER_ERR_STATE, "member 0", "phi")           # no phi yet
        for m in range(B):
            b.upload_phi(m, phis[m])
        refused(b, 0, [2, 2, 2], None, WAFER_ERR_STATE, "member 1", "potential")
        refused(b, 1, [1, 1, 1], None, WAFER_ERR_STATE, "member 1", "potential")
        b.set_potential(1, "Periodic")
        refused(b, 0, [2, 0, 2], None, WAFER_ERR_INVALID, "member 1")
        refused(b, 0, [2, 2, 9], None, WAFER_ERR_INVALID, "member 2")
        refused(b, 0, [4, 2, 2], None, WAFER_ERR_STATE, "member 0")
        refused(b, 1, [1, 2, 1], None, WAFER_ERR_INVALID, "member 1")
        refused(b, 2, [1, 1, 1], None, WAFER_ERR_INVALID, "source")
        bad = np.ones((B, KM))
        bad[2, 1] = np.inf
        refused(b, 0, [2, 2, 2], bad, WAFER_ERR_INVALID, "member 2", "finite")
        for m in range(B):
            assert same(b.download_phi(m), phis[m]), m
            for j in range(3):
                assert same(b.download_state(m, j), states[m][j]), (m, j)
    with wa.Batch(members, mixed_shapes=True) as b:                                  # several shapes, no state stores
        b.set_potentials(["Harmonic"] * 3)
        for m in range(B):
            b.upload_phi(m, phis[m])
        refused(b, 0, [1, 1, 1], None, WAFER_ERR_INVALID, "mixed-shape", "wafer_batch_residuals")
        with pytest.raises(wa.WaferError, match="mixed-shape"):
            b.residuals(1)
        assert all(r["status"] == 0 for r in b.residuals(source="phi"))


# ---- 6. the sweep's --residuals flag -----------------------------------------------------------------------------------------------------------
YAML = """project_name: {name}
grid:
    size:
        x: {nx}
        y: 20
        z: {nz}
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
    save_wavefns: true
    save_potential: false
"""
SWEEP_RUNS = [("two", 20, 20, 0.03, 1), ("ground", 20, 20, 0.04, 0), ("small", 16, 12, 0.04, 0)]


@pytest.fixture(scope="module")
def swept(tmp_path_factory):
    """the three runs as one sweep, without and with --residuals, the same seed -> per variant (stdout, the runs' directories)"""
    tmp = str(tmp_path_factory.mktemp("sweep"))
    configs = []
    for name, nx, nz, dt, wavemax in SWEEP_RUNS:
        d = os.path.join(tmp, name)
        os.makedirs(d)
        with open(os.path.join(d, "wafer.yaml"), "w") as f:
            f.write(YAML.format(name=name, nx=nx, nz=nz, dt=dt, wavemax=wavemax))
        configs += ["-c", os.path.join(d, "wafer.yaml")]
    out = {}
    for variant, extra in (("plain", []), ("residuals", ["--residuals"])):
        od = os.path.join(tmp, "out_" + variant)
        r = subprocess.run([sys.executable, "-m", "wafer_amd.sweep", *configs, "--output-dir", od, "--seed", "7", *extra],
                           capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr
        out[variant] = (r.stdout, [os.path.join(od, d) for d in sorted(os.listdir(od))])
    return out


def files_of(d):
    return {name: open(os.path.join(d, name), "rb").read() for name in sorted(os.listdir(d))}


def strip(line):
    """a JSON line without what differs between two sweeps of the same files: the time-stamped directory"""
    d = json.loads(line)
    d.pop("directory")
    return d


def test_sweep_without_the_flag_knows_no_residuals(swept):
    plain, flagged = swept["plain"][0].splitlines(), swept["residuals"][0].splitlines()
    assert "residual" not in swept["plain"][0].lower()
    for a, b in zip(plain[:3], flagged[:3]):                     # the flag adds the key and changes nothing else
        want = strip(b)
        assert "residuals" in want
        want.pop("residuals")
        assert strip(a) == want
    for d0, d1 in zip(swept["plain"][1], swept["residuals"][1]):
        assert files_of(d0) == files_of(d1)


def test_sweep_with_the_flag(wa, swept):
    """each line's residuals are Context.residuals() of a context that solved the same file.  The ground-state runs are solved here
    (Context.solve_state, the sweep's seed); the run with an excited state takes the states its sweep saved, as
    tests/test_gpu_batch_ritz.py does: its second start is a clone that Gram-Schmidt empties, and the reseeded start is the sweep's own"""
    lines = [json.loads(l) for l in swept["residuals"][0].splitlines()[:3]]
    dirs = swept["residuals"][1]
    for i, (name, nx, nz, dt, wavemax) in enumerate(SWEEP_RUNS):
        par = wa.Params(nx, 20, nz, dn=0.5, dt=dt, mass=1.0, sig=1.0, central_difference=1, max_states=wavemax + 1)
        with wa.Context(par) as ctx:
            ctx.set_potential("Harmonic")
            if wavemax == 0:
                ctx.set_initial_condition("Boolean", seed=7)
                _, _, conv = ctx.solve_state(0, 1e-7, 100, 200000)
                assert conv and ctx.num_states() == 1
                want = ctx.residuals(source="phi")
                assert same(want["theta"], ctx.residuals()["theta"])
            else:
                for a in range(wavemax + 1):
                    full = np.zeros((nx + 2, 22, nz + 2))
                    full[1:-1, 1:-1, 1:-1] = np.load(os.path.join(dirs[i], f"wavefunction_{a}.npy"))
                    ctx.load_state(a, full)
                want = ctx.residuals()
        got = lines[i]["residuals"]
        print(name, got, want)
        assert got == dict(theta=[float(x) for x in want["theta"]], rho=[float(x) for x in want["rho"]]), (name, got, want)
        assert len(got["theta"]) == wavemax + 1
