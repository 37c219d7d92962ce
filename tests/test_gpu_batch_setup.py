"""Set-up of many batch members at once on the MI355X: Batch.set_potentials / set_initial_conditions against the per-member calls
(bit for bit, on integer views), the one range check for all listed members against the numpy model of tests/batch_setup_model.py and
against the per-member check, the launch accounting, the refusals, and wafer_amd.sweep with and without --batched-setup.

Shapes (tiles are 64 x 4): (70, 9, 5) two tiles in x, ny odd and no multiple of 4 -- the mirror has a middle row; (12, 10, 7) ny even;
(33, 6, 12).  One-shape batch: 4 x (70, 9, 5) and a fifth member that is not listed; mixed: the three shapes, (12, 10, 7) again, and
the unlisted fifth."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import batch_setup_model as model  # noqa: E402

SHAPES = {"one": [(70, 9, 5)] * 5, "mixed": [(70, 9, 5), (12, 10, 7), (33, 6, 12), (12, 10, 7), (33, 6, 12)]}
KINDS = {"one": {}, "mixed": dict(mixed_shapes=True), "mixed_states": dict(mixed_shapes=True, state_stores=True)}
# dn, dt, mass, sig differ from member to member (dt <= dn^2 / 3)
SPECS = [dict(dn=0.2, dt=0.004, mass=1.0, sig=1.0), dict(dn=0.25, dt=0.01, mass=0.5, sig=0.223), dict(dn=0.2, dt=0.003, mass=1.5, sig=0.6),
         dict(dn=0.3, dt=0.02, mass=2.0, sig=1.4), dict(dn=0.22, dt=0.005, mass=0.8, sig=0.9)]
MASK = [1, 1, 1, 1, 0]
LISTED = range(4)
EXTS = [1, 3]          # ThreePoint and SevenPoint: the frames differ
DTYPES = ["f64", "f32", "f32fast"]
BUILTIN = ["NoPotential", "Cube", "QuadWell", "Periodic", "Coulomb", "ComplexCoulomb", "ElipticalCoulomb", "SimpleCornell", "FullCornell",
           "Harmonic", "ComplexHarmonic", "Dodecahedron"]
GENERATED = ["Gaussian", "Coulomb", "Constant", "Boolean"]
WAFER_ERR_INVALID, WAFER_ERR_NOT_AVAILABLE = -1, -3


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


def params(wa, kind, ext, dtype):
    shapes = SHAPES["one" if kind == "one" else "mixed"]
    return [wa.Params(*s, central_difference=ext, dtype=dtype, max_states=2, **SPECS[k]) for k, s in enumerate(shapes)]


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(u64(a), u64(b))


def snapshot(b, m):
    """everything the issue compares of one member, on integer views"""
    info = b.member_info(m)
    out = dict(info=info, potsub=b.potsub(m), v=u64(b.download_array(m, "v")))
    if info["have_phi"]:
        out["phi"] = u64(b.download_phi(m))
    if info["potsub_kind"] == 2:
        out["potsub_array"] = u64(b.download_array(m, "potsub"))
    return out


def assert_same_member(a, b, where):
    assert a.keys() == b.keys(), where
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (where, k)
        else:
            assert a[k] == b[k], (where, k, a[k], b[k])


# ---- 1. the setters against the per-member calls ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ext", EXTS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_setters_give_the_bits_of_the_per_member_calls(wa, kind, ext, dtype):
    pars = params(wa, kind, ext, dtype)
    with wa.Batch(pars, **KINDS[kind]) as A, wa.Batch(pars, **KINDS[kind]) as B:
        for b in (A, B):   # the member that is never listed: another potential and start, beforehand
            b.set_potential(4, "Harmonic")
            b.set_initial_condition(4, "Constant")
        bystander = snapshot(A, 4)
        assert_same_member(bystander, snapshot(B, 4), "bystander")
        for rnd in range(3):   # all twelve built-in potentials over the four listed members
            names = [BUILTIN[(4 * rnd + m) % 12] for m in LISTED] + ["FromFile"]   # (the unlisted entry is not read)
            A.set_potentials(names, active=MASK)
            for m in LISTED:
                B.set_potential(m, names[m])
            for m in LISTED:
                a = snapshot(A, m)
                assert_same_member(a, snapshot(B, m), (rnd, m, names[m]))
                assert a["info"]["have_pot"] == 1 and a["info"]["member"] == m
                assert a["potsub"][0] == {"FullCornell": 2, "ElipticalCoulomb": 1, "SimpleCornell": 1}.get(names[m], 0), names[m]
                v = u64(A.download_array(m, "v")).view(np.float64)
                assert a["info"]["v_in_range"] == int(model.in_range(v, pars[m].dt)) and a["info"]["v_ysym"] == int(model.y_symmetric(v, ext))
            assert_same_member(bystander, snapshot(A, 4), ("bystander", rnd))
        for rot in (0, 2):     # the four generated starts, Gaussian with its own seed per member
            names = [GENERATED[(m + rot) % 4] for m in LISTED] + [99]
            seeds = [11 + rot, 12 + rot, 13 + rot, 14 + rot, 0]
            A.set_initial_conditions(names, seeds=seeds, active=MASK)
            for m in LISTED:
                B.set_initial_condition(m, names[m], seed=seeds[m])
            for m in LISTED:
                a = snapshot(A, m)
                assert_same_member(a, snapshot(B, m), (rot, m, names[m]))
                assert a["info"]["have_phi"] == 1
            assert_same_member(bystander, snapshot(A, 4), ("bystander", rot))
        # one member per shape against a Context of its Params (the last potentials and starts)
        for m in sorted({s: k for k, s in reversed(list(enumerate(SHAPES["one" if kind == "one" else "mixed"][:4])))}.values()):
            with wa.Context(pars[m]) as c:
                c.set_potential(BUILTIN[(8 + m) % 12])
                c.set_initial_condition(GENERATED[(m + 2) % 4], seed=13 + m)
                assert same(A.download_array(m, "v"), c.download_array("v")), m
                assert same(A.download_phi(m), c.download_phi()), m
                assert A.potsub(m) == c.potsub()
        # a member's a, b arrays, once asked for, are kept in step by the batched writer as by the per-member one
        assert same(A.download_array(1, "a"), B.download_array(1, "a")) and same(A.download_array(1, "b"), B.download_array(1, "b"))
        names = ["SimpleCornell", "Coulomb", "Harmonic", "Cube", 0]
        A.set_potentials(names, active=MASK)
        for m in LISTED:
            B.set_potential(m, names[m])
        for which in ("v", "a", "b"):
            assert same(A.download_array(1, which), B.download_array(1, which)), which
        assert_same_member(bystander, snapshot(A, 4), "bystander, a and b")
        A.evolve(4)
        B.evolve(4)
        oa, ob = A.observables(), B.observables()
        assert oa == ob and all(np.isfinite(list(o.values())).all() for o in oa)
        for m in range(5):
            assert same(A.download_phi(m), B.download_phi(m)), m


# ---- 2. the check against the model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ext", EXTS)
@pytest.mark.parametrize("kind", ["one", "mixed"])
def test_range_check_of_all_members_against_the_model_and_the_per_member_check(wa, kind, ext, dtype):
    pars = params(wa, kind, ext, dtype)
    outcomes = set()
    with wa.Batch(pars, **KINDS[kind]) as A, wa.Batch(pars, **KINDS[kind]) as B:
        for name, src in model.sources().items():
            before = A.setup_counts()
            A.resample_potential(np.array(src))
            assert A.setup_counts() == (before[0] + 1, before[1] + 1)   # one check launch, one read-back, for five members
            for m in range(5):
                v = A.download_array(m, "v")
                want = dict(v_in_range=int(model.in_range(v, pars[m].dt)), v_ysym=int(model.y_symmetric(v, ext)))
                info = A.member_info(m)
                assert {k: info[k] for k in want} == want, (name, m)
                B.set_potential_host(m, v)                               # today's per-member check on the same array
                binfo = B.member_info(m)
                assert same(B.download_array(m, "v"), v)
                assert {k: binfo[k] for k in want} == want, (name, m)
                assert info["short_forms"] == binfo["short_forms"] and info["have_pot"] == 1
                outcomes.add((name, info["v_in_range"], info["v_ysym"]))
    assert {o for o in outcomes if o[0] == "flat"} == {("flat", 1, 1)}
    assert {o[:2] for o in outcomes if o[0] in ("nan", "huge")} == {("nan", 0), ("huge", 0)}
    assert {o for o in outcomes if o[0] == "skew"} == {("skew", 1, 0)}


# ---- 3. launch accounting -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["one", "mixed"])
def test_launches_and_read_backs_do_not_grow_with_the_members(wa, kind):
    pars = params(wa, kind, 1, "f64")
    with wa.Batch(pars, **KINDS[kind]) as b:
        assert b.setup_counts() == (0, 0)
        b.set_potentials(["Harmonic", "Coulomb", "Cube", "SimpleCornell", "Periodic"])
        assert b.setup_counts() == (2, 1)                     # generate + check, one read-back
        b.set_potentials(["Harmonic", "Coulomb", "FullCornell", "SimpleCornell", "Periodic"])
        assert b.setup_counts() == (5, 2)                     # + pot_sub: a listed member is FullCornell
        b.set_potentials(["Harmonic", "Coulomb", "FullCornell", "SimpleCornell", "Periodic"], active=[1, 1, 0, 1, 1])
        assert b.setup_counts() == (7, 3)                     # the FullCornell entry is not listed: no pot_sub launch
        b.set_initial_conditions(["Boolean", "Gaussian", "Constant", "Coulomb", "Boolean"], seeds=[1, 2, 3, 4, 5])
        assert b.setup_counts() == (8, 3)                     # one launch, no read-back
        b.resample_potential(model.sources()["skew"])
        assert b.setup_counts() == (9, 4)                     # exactly one check launch and one read-back
        b.set_potentials(["Harmonic"] * 5, active=[0] * 5)
        b.set_initial_conditions(["Boolean"] * 5, active=[0] * 5)
        b.resample_potential(model.sources()["skew"], active=[0] * 5)
        assert b.setup_counts() == (9, 4)                     # nobody listed: nothing
        b.set_potential(0, "Harmonic")                        # the per-member calls are not counted: they are not batched
        b.set_initial_condition(0, "Boolean")
        assert b.setup_counts() == (9, 4)
        with pytest.raises(ValueError):
            b.set_potentials(["Harmonic"] * 4)                # a length mismatch never reaches the library
        with pytest.raises(ValueError):
            b.set_potentials(["Harmonic"] * 5, active=[1] * 4)
        assert b.setup_counts() == (9, 4)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["one", "mixed"])
def test_a_refused_call_changes_nothing(wa, kind):
    pars = params(wa, kind, 1, "f32")
    with wa.Batch(pars, **KINDS[kind]) as b:
        b.set_potentials(["Harmonic", "Coulomb", "FullCornell", "SimpleCornell", "Periodic"])
        b.set_initial_conditions(["Boolean", "Gaussian", "Constant", "Coulomb", "Boolean"], seeds=[1, 2, 3, 4, 5])
        before, counts = [snapshot(b, m) for m in range(5)], b.setup_counts()
        good_p, good_i = ["Cube"] * 5, ["Constant"] * 5
        cases = [(lambda: b.set_potentials(good_p[:2] + [14] + good_p[3:], active=MASK), WAFER_ERR_INVALID, "unknown potential 14"),
                 (lambda: b.set_potentials(good_p[:2] + [-1] + good_p[3:], active=MASK), WAFER_ERR_INVALID, "unknown potential -1"),
                 (lambda: b.set_potentials(good_p[:2] + ["FromFile"] + good_p[3:], active=MASK), WAFER_ERR_NOT_AVAILABLE, "PotentialNotAvailable"),
                 (lambda: b.set_potentials(good_p[:2] + ["FromScript"] + good_p[3:], active=MASK), WAFER_ERR_NOT_AVAILABLE, "PotentialNotAvailable"),
                 (lambda: b.set_initial_conditions(good_i[:2] + [5] + good_i[3:], active=MASK), WAFER_ERR_INVALID, "unknown initial condition 5"),
                 (lambda: b.set_initial_conditions(good_i[:2] + ["FromFile"] + good_i[3:], active=MASK), WAFER_ERR_NOT_AVAILABLE, "wafer_upload_phi")]
        for call, code, needle in cases:
            with pytest.raises(wa.WaferError) as e:
                call()
            assert e.value.code == code and "member 2" in str(e.value) and needle in str(e.value), str(e.value)
            assert b.setup_counts() == counts
            for m in range(5):   # the members before the bad one were not written either: every check runs first
                assert_same_member(before[m], snapshot(b, m), (needle, m))
        # the same bad entries on the member that is not listed are not read
        b.set_potentials(good_p[:4] + [14], active=MASK)
        b.set_potentials(good_p[:4] + ["FromFile"], active=MASK)
        b.set_initial_conditions(good_i[:4] + [5], active=MASK)
        assert b.setup_counts() == (counts[0] + 5, counts[1] + 2)
        assert_same_member(before[4], snapshot(b, 4), "bystander")
        with pytest.raises(ValueError):
            b.set_initial_conditions(good_i, seeds=[1, 2])
        with pytest.raises(ValueError):
            b.download_array(5, "v")
        with pytest.raises(wa.WaferError) as e:   # Harmonic has no pot_sub array
            b.download_array(0, "potsub")
        assert e.value.code == -4


# ---- 5. the sweep -----------------------------------------------------------------------------------------------------------------------
def test_sweep_with_batched_setup_writes_the_same_files(tmp_path, capsys):
    from wafer_amd import sweep
    from tests.test_gpu_sweep import run_sweep, write_run
    runs = [dict(size=(20, 20, 20), potential="Harmonic", dn=0.5, dt=0.04, mass=1.0, init_condition="Boolean", screen_update=10, tolerance="1e-7"),
            dict(size=(16, 20, 12), potential="Coulomb", dn=0.6, dt=0.05, mass=1.0, init_condition="Gaussian", screen_update=25, tolerance="1e-6",
                 max_steps=100)]
    paths = [write_run(tmp_path, f"run{k}", **r) for k, r in enumerate(runs)]
    _, lines_a, dirs_a = run_sweep(sweep, capsys, paths, tmp_path / "per_member", "--progress")
    _, lines_b, dirs_b = run_sweep(sweep, capsys, paths, tmp_path / "batched", "--progress", "--batched-setup")
    for k in range(2):
        assert lines_a[k]["batch_members"] == lines_b[k]["batch_members"] == [0, 1] and lines_b[k]["mixed_shapes"]
        assert lines_a[k]["states"] == lines_b[k]["states"]
        assert open(os.path.join(dirs_a[k], "table.txt")).read() == open(os.path.join(dirs_b[k], "table.txt")).read()
        name = "wavefunction_0.npy" if lines_a[k]["converged"] else "wavefunction_0_partial.npy"
        assert same(np.load(os.path.join(dirs_a[k], name)), np.load(os.path.join(dirs_b[k], name))), k
    assert lines_a[0]["converged"] and os.path.exists(os.path.join(dirs_b[0], "wavefunction_0.npy"))


# ---- 6. not vacuous -----------------------------------------------------------------------------------------------------------------------
def test_each_flag_takes_both_values(wa):
    """By the index arithmetic of the built-in potentials (their centre is (n + 1) / 2 in PADDED indices) they are their own mirror
    image in y on the ThreePoint frame and not on the SevenPoint frame; a source with 1e200 leaves the range.  The model decides, the
    engine must agree, and both values of both flags must occur."""
    seen = dict(v_in_range=set(), v_ysym=set())
    for ext in EXTS:
        pars = params(wa, "mixed", ext, "f64")
        with wa.Batch(pars, mixed_shapes=True) as b:
            b.set_potentials(["Harmonic", "Coulomb", "Harmonic", "SimpleCornell", "Harmonic"])   # functions of wafer_r2 alone
            b.resample_potential(model.sources()["huge"], active=[0, 0, 0, 0, 1])
            for m in range(5):
                info, v = b.member_info(m), b.download_array(m, "v")
                assert info["v_in_range"] == int(model.in_range(v, pars[m].dt)) and info["v_ysym"] == int(model.y_symmetric(v, ext)), (ext, m)
                for k in seen:
                    seen[k].add(info[k])
                if m < 4:
                    assert info["v_ysym"] == int(ext == 1), (ext, m)
    assert seen == dict(v_in_range={0, 1}, v_ysym={0, 1}), seen
