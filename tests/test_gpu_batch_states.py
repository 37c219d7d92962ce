"""Batched excited states (wafer_amd.Batch: state stores, evolve(..., wnum=k), orthogonalise, norm2, solve_state) on the MI355X.
Every member must compute what the reference computes for it -- the oracle's wo.evolve / wo.solve with the member's own store --
to the project's excited-state tolerances (tests/test_gpu_parity.py: test_excited_state_evolve,
test_excited_state_evolve_nonorthogonal_store, test_norm_normalise_orthogonalise, test_solve_matches_oracle), and a member's
bits must not depend on the batch around it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.gpu_common import make_pair, random_phi  # noqa: E402
from tests.test_gpu_batch import MEMBERS, host_v  # noqa: E402

SHAPES = [(50, 50, 50), (64, 64, 64), (37, 50, 23)]
STEPS = 25


@pytest.fixture(scope="module")
def wo():
    from oracle import wafer_oracle
    wafer_oracle.build()
    return wafer_oracle


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


def orthonormal_store(wo, cfg, wnum, seed):
    """an orthonormal set, as converged states would be"""
    lowers = []
    for i in range(wnum):
        l = random_phi(cfg, seed=seed + i)
        wo.orthogonalise(i, l, lowers)
        wo.normalise(l, wo.norm2(cfg, l))
        lowers.append(l)
    return lowers


def correlated_store(wo, cfg, wnum, seed):
    """normalised states that are NOT orthogonal to each other"""
    lowers = []
    for i in range(wnum):
        l = random_phi(cfg, seed=seed + i) + (0.4 * lowers[0] if lowers else 0.0)
        wo.normalise(l, wo.norm2(cfg, l))
        lowers.append(np.ascontiguousarray(l))
    return lowers


def member_problem(wo, k, spec, shape, ext, max_states=4):
    """-> [cfg, par, v, potsub, phi] of tests/test_gpu_batch.py's member `spec`, seeded by k; every phi is uploaded"""
    host = spec["potential"].startswith("host")
    cfg, par = make_pair(shape, ext=ext, potential="Harmonic" if host else spec["potential"], dn=spec["dn"], dt=spec["dt"],
                         mass=spec["mass"], max_states=max_states, unplanned_div=spec.get("unplanned_div", False))
    if spec["potential"] == "host":
        v, potsub = host_v(cfg), (0, 0.0, None)
    elif spec["potential"] == "host_potsub":
        v, potsub = host_v(cfg), (2, 0.0, np.random.default_rng(7).standard_normal(cfg.work_shape))
    else:
        v, potsub = wo.potential_generate(cfg), wo.potential_sub(cfg)
    return [cfg, par, v, potsub, random_phi(cfg, seed=40 + k)]


def make_batch(wa, ms, stores, order=None):
    """the members ms[k] (with stores[k] loaded) as a batch, in the given order of k"""
    order = list(range(len(ms))) if order is None else order
    b = wa.Batch([ms[k][1] for k in order])
    for slot, k in enumerate(order):
        cfg, par, v, potsub, phi = ms[k]
        b.set_potential_host(slot, v, potsub[0], potsub[1], potsub[2])
        b.upload_phi(slot, phi)
        for i, l in enumerate(stores[k]):
            b.load_state(slot, i, l)
    return b


def make_context(wa, m, store, phi=None):
    cfg, par, v, potsub, phi0 = m
    ctx = wa.Context(par)
    ctx.set_potential_host(v, potsub[0], potsub[1], potsub[2])
    ctx.upload_phi(phi0 if phi is None else phi)
    for i, l in enumerate(store):
        ctx.load_state(i, l)
    return ctx


def problems(wo, shape, ext, wnum, max_states=4, store=orthonormal_store, specs=MEMBERS):
    ms = [member_problem(wo, k, s, shape, ext, max_states) for k, s in enumerate(specs)]
    stores = [store(wo, m[0], wnum, seed=100 + 10 * k) for k, m in enumerate(ms)]   # a store of its own per member
    return ms, stores


def check_against_oracle(wo, b, slot, m, store, wnum, steps, atol=1e-13, rel=1e-12, n2=None):
    cfg, par, v, potsub, phi = m
    a_, b_ = wo.ab(cfg, v)
    want = phi.copy()
    wo.evolve(cfg, wnum, a_, b_, want, store, steps)
    got = b.download_phi(slot)
    err = float(np.max(np.abs(got - want)))
    n2 = b.norm2()[slot] if n2 is None else n2
    ref_n2 = wo.norm2(cfg, want)
    overlaps = [abs(float(np.sum(l * got))) for l in store[:wnum]]
    print("member", slot, "max|dphi|", err, "norm2", n2, "ref", ref_n2, "overlaps", overlaps)
    assert err <= atol, (slot, err)
    assert n2 == pytest.approx(ref_n2, rel=rel), slot
    return overlaps


# ---- 1. evolve against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wnum", [1, 2, 3])
@pytest.mark.parametrize("ext", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_batch_excited_evolve_matches_oracle(wa, wo, shape, ext, wnum):
    ms, stores = problems(wo, shape, ext, wnum)
    with make_batch(wa, ms, stores) as b:
        b.evolve(STEPS, wnum=wnum)
        n2 = b.norm2()
        for k, m in enumerate(ms):
            overlaps = check_against_oracle(wo, b, k, m, stores[k], wnum, STEPS, n2=n2[k])
            assert all(s < 1e-13 for s in overlaps), (k, overlaps)
            for i, l in enumerate(stores[k]):   # the store is read, never written
                assert np.array_equal(b.download_state(k, i), l), (k, i)


# ---- 2. a store that is not orthonormal ------------------------------------------------------------------------------------
@pytest.mark.parametrize("wnum", [2, 4, 5])
def test_batch_excited_evolve_nonorthogonal_store(wa, wo, wnum):
    ms, stores = problems(wo, (26, 19, 23), 2, wnum, max_states=5, store=correlated_store)
    with make_batch(wa, ms, stores) as b:
        b.evolve(6, wnum=wnum)
        for k, m in enumerate(ms):
            check_against_oracle(wo, b, k, m, stores[k], wnum, 6, atol=2e-13, rel=1e-11)


# ---- 3. against Context ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wnum", [1, 2, 3])
@pytest.mark.parametrize("ext", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_batch_excited_evolve_matches_contexts(wa, wo, shape, ext, wnum):
    """not bit for bit: the context's two-steps-per-pass kernels regroup the sums (test_two_excited_steps_per_pass_vs_oracle)"""
    ms, stores = problems(wo, shape, ext, wnum)
    with make_batch(wa, ms, stores) as b:
        b.evolve(STEPS, wnum=wnum)
        n2 = b.norm2()
        for k, m in enumerate(ms):
            with make_context(wa, m, stores[k]) as ctx:
                ctx.evolve(wnum, STEPS)
                want, want_n2 = ctx.download_phi(), ctx.norm2()
            got = b.download_phi(k)
            err = float(np.max(np.abs(got - want)))
            print("member", k, "max|dphi|", err, "norm2", n2[k], "context", want_n2)
            assert err <= 1e-13, (k, err)
            assert n2[k] == pytest.approx(want_n2, rel=1e-12), k
            for l in stores[k]:
                assert abs(float(np.sum(l * got))) < 1e-13, k


@pytest.mark.parametrize("shape,ext,wnum", [((50, 50, 50), 1, 3), ((64, 64, 64), 2, 2), ((37, 50, 23), 3, 1)])
def test_batch_orthogonalise_and_norm2_match_contexts(wa, wo, shape, ext, wnum):
    ms, stores = problems(wo, shape, ext, wnum)
    with make_batch(wa, ms, stores) as b:
        n2 = b.norm2()
        b.orthogonalise(wnum)
        n2_after = b.norm2()
        for k, m in enumerate(ms):
            with make_context(wa, m, stores[k]) as ctx:
                assert n2[k] == pytest.approx(ctx.norm2(), rel=1e-12), k
                ctx.orthogonalise(wnum)
                want = ctx.download_phi()
                assert n2_after[k] == pytest.approx(ctx.norm2(), rel=1e-12), k
            ref = m[4].copy()
            wo.orthogonalise(wnum, ref, stores[k])
            got = b.download_phi(k)
            print("member", k, "vs context", float(np.max(np.abs(got - want))), "vs oracle", float(np.max(np.abs(got - ref))))
            assert np.allclose(got, want, rtol=0, atol=1e-14), k
            assert np.allclose(got, ref, rtol=0, atol=1e-14), k
            assert n2[k] == pytest.approx(wo.norm2(m[0], m[4]), rel=1e-12), k
        with pytest.raises(wa.WaferError) as e:
            b.orthogonalise(wnum + 1)   # every store is too short
        assert e.value.code == wa.engine.WAFER_ERR_STATE and "member 0" in str(e.value)


# ---- 4. independence and determinism, exact --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ext,wnum", [((50, 50, 50), 1, 2), ((64, 64, 64), 1, 3), ((37, 50, 23), 2, 1), ((64, 64, 64), 3, 2)])
def test_batch_excited_member_bits_do_not_depend_on_the_batch(wa, wo, shape, ext, wnum):
    ms, stores = problems(wo, shape, ext, wnum)
    B = len(ms)
    with make_batch(wa, ms, stores) as b:
        b.evolve(STEPS, wnum=wnum)
        full = [b.download_phi(k) for k in range(B)]
        full_n2 = b.norm2()
    with make_batch(wa, ms, stores) as b:   # the same call from the same start: the same bits
        b.evolve(STEPS, wnum=wnum)
        for k in range(B):
            assert np.array_equal(b.download_phi(k), full[k]), k
        assert b.norm2() == full_n2
    for k in range(B):                      # alone in a batch of one
        with make_batch(wa, ms, stores, order=[k]) as b:
            b.evolve(STEPS, wnum=wnum)
            assert np.array_equal(b.download_phi(0), full[k]), k
            assert b.norm2()[0] == full_n2[k], k
    order = [3, 4, 0, 1, 2]                 # at another index
    with make_batch(wa, ms, stores, order=order) as b:
        b.evolve(STEPS, wnum=wnum)
        for slot, k in enumerate(order):
            assert np.array_equal(b.download_phi(slot), full[k]), k
    for mask in ([1, 0, 0, 1, 0], [0, 1, 1, 0, 1], [0, 0, 1, 0, 0]):   # with the others frozen
        with make_batch(wa, ms, stores) as b:
            b.evolve(STEPS, active=mask, wnum=wnum)
            for k in range(B):
                got = b.download_phi(k)
                if mask[k]:
                    assert np.array_equal(got, full[k]), (mask, k)
                else:
                    assert got.tobytes() == ms[k][4].tobytes(), (mask, k)
                for i, l in enumerate(stores[k]):
                    assert b.download_state(k, i).tobytes() == l.tobytes(), (mask, k, i)
            # the frozen members continue from where they stood
            b.evolve(STEPS, active=[1 - x for x in mask], wnum=wnum)
            for k in range(B):
                assert np.array_equal(b.download_phi(k), full[k]), (mask, k)


def test_batch_orthogonalise_mask_and_determinism(wa, wo):
    ms, stores = problems(wo, (40, 36, 44), 1, 3)
    with make_batch(wa, ms, stores) as b:
        b.orthogonalise(3)
        full = [b.download_phi(k) for k in range(len(ms))]
    mask = [0, 1, 0, 1, 1]
    with make_batch(wa, ms, stores) as b:
        b.orthogonalise(3, active=mask)
        for k in range(len(ms)):
            want = full[k] if mask[k] else ms[k][4]
            assert b.download_phi(k).tobytes() == want.tobytes(), k


# ---- 5. wnum = 0 ---------------------------------------------------------------------------------------------------------------
def test_batch_wnum_zero_paths(wa, wo):
    ms, stores = problems(wo, (40, 36, 44), 1, 0)
    with make_batch(wa, ms, stores) as b, make_batch(wa, ms, stores) as b0:
        b.evolve(7)
        b0.evolve(7, wnum=0)
        for k in range(len(ms)):
            assert b.download_phi(k).tobytes() == b0.download_phi(k).tobytes(), k
        assert b0.num_states() == [0] * len(ms)
    shape, tol, su = (32, 32, 32), 1e-7, 50
    dts = [0.0015, 0.004, 0.006, 0.008, 0.012]   # tests/test_gpu_batch.py::test_batch_solve_matches_contexts: member 0 ends in MaxStep
    pars = [wa.Params(*shape, dn=0.2, dt=dt, mass=1.0) for dt in dts]
    cfg0, _ = make_pair(shape, dn=0.2, dt=dts[0])
    phi0 = wo.initial_condition(cfg0, "Gaussian")
    with wa.Batch(pars) as b, wa.Batch(pars) as b0:
        for k in range(len(pars)):
            for x in (b, b0):
                x.set_potential(k, "Harmonic")
                x.upload_phi(k, phi0)
        free = b.solve(tol, su)
        last = [r[0][-1]["step"] for r in free]
        max_steps = max(last[1:])
        assert last[0] > max_steps + su, last
        for k in range(len(pars)):
            b.upload_phi(k, phi0)
        want = b.solve(tol, su, max_steps)
        got = b0.solve_state(0, tol, su, max_steps)
        assert got == want
        assert [r[2] for r in got] == [False, True, True, True, True]
        for k in range(len(pars)):
            assert b.download_phi(k).tobytes() == b0.download_phi(k).tobytes(), k
        assert b.num_states() == [0] * 5          # solve pushes nothing
        assert b0.num_states() == [0, 1, 1, 1, 1]  # solve_state pushes what converged
        for k in range(1, 5):
            assert b0.download_state(k, 0).tobytes() == b0.download_phi(k).tobytes(), k


# ---- 6. / 7. solve ---------------------------------------------------------------------------------------------------------
SOLVE_DTS = [0.032, 0.02, 0.012]
SOLVE_ARGS = dict(tolerance=1e-9, screen_update=100, max_steps=100000)


def solve_setup(wa, wo):
    ms = []
    for dt in SOLVE_DTS:
        cfg, par = make_pair((32, 32, 32), ext=1, potential="Harmonic", dn=0.4, dt=dt, mass=1.0)
        v = wo.potential_generate(cfg)
        ms.append((cfg, par, v, wo.ab(cfg, v)))
    b = wa.Batch([m[1] for m in ms])
    for k in range(len(ms)):
        b.set_potential(k, "Harmonic")
    return b, ms


def upload_guess(wo, b, ms, wnum):
    """a fresh O(1) guess per state on both sides (test_solve_matches_oracle's docstring says why not the clone)"""
    phis = [wo.initial_condition(m[0], "Gaussian", seed=3 + wnum) for m in ms]
    for k, phi in enumerate(phis):
        b.upload_phi(k, phi)
    return phis


def test_batch_solve_states_match_oracle(wa, wo):
    b, ms = solve_setup(wa, wo)
    with b:
        stores = [[] for _ in ms]
        energies = [[] for _ in ms]
        stops = []
        for wnum in range(3):
            phis = upload_guess(wo, b, ms, wnum)
            got = b.solve_state(wnum, **SOLVE_ARGS)
            for k, (cfg, par, v, (a_, b_)) in enumerate(ms):
                want, conv = wo.solve(cfg, wnum, v, a_, b_, phis[k], stores[k], 1e-9, 100, max_steps=100000)
                rows, final, gconv, status = got[k]
                print("state", wnum, "member", k, "rows", len(rows), len(want), "E", final["energy"], want[-1]["energy"] / want[-1]["norm2"])
                assert conv and gconv and status == wa.engine.WAFER_OK, (wnum, k, conv, gconv, status)
                assert abs(len(rows) - len(want)) <= 1, (wnum, k)
                for g, w in zip(rows, want):
                    assert g["step"] == w["step"] and g["tau"] == w["tau"]
                    assert g["energy"] / g["norm2"] == pytest.approx(w["energy"] / w["norm2"], abs=2e-9)
                    assert np.sqrt(g["r2"] / g["norm2"]) == pytest.approx(np.sqrt(w["r2"] / w["norm2"]), rel=1e-7)
                assert final["state"] == wnum
                stores[k].append(phis[k].copy())
                energies[k].append(final["energy"])
            assert b.num_states() == [wnum + 1] * len(ms)
            stops.append([r[0][-1]["step"] for r in got])
        for k in range(len(ms)):
            assert energies[k][0] == pytest.approx(1.5, abs=0.02), k
            assert energies[k][1] == pytest.approx(2.5, abs=0.04) and energies[k][2] == pytest.approx(2.5, abs=0.04), k
        assert all(len(set(s)) == 3 for s in stops), stops   # members freeze one by one while the rest go on


def test_batch_solve_state_with_a_short_store(wa, wo):
    b, ms = solve_setup(wa, wo)
    b2, _ = solve_setup(wa, wo)
    with b, b2:
        for x in (b, b2):
            upload_guess(wo, x, ms, 0)
            assert all(r[2] for r in x.solve_state(0, **SOLVE_ARGS))
        b.clear_states([0, 1, 0])
        assert b.num_states() == [1, 0, 1]
        for x in (b, b2):
            upload_guess(wo, x, ms, 1)
        before = b.download_phi(1)
        got = b.solve_state(1, **SOLVE_ARGS)   # returns: the short store is member 1's error, not the call's
        want = b2.solve_state(1, **SOLVE_ARGS)
        assert got[1][3] == wa.engine.WAFER_ERR_STATE and not got[1][2] and got[1][0] == []
        assert b.download_phi(1).tobytes() == before.tobytes()
        assert b.num_states() == [2, 0, 2]
        for k in (0, 2):
            assert got[k] == want[k], k
            assert got[k][2] and got[k][3] == wa.engine.WAFER_OK
            assert b.download_phi(k).tobytes() == b2.download_phi(k).tobytes(), k
            assert b.download_state(k, 1).tobytes() == b2.download_state(k, 1).tobytes(), k
        with pytest.raises(wa.WaferError) as e:   # the calls without a status per member name the member instead
            b.evolve(3, wnum=1)
        assert e.value.code == wa.engine.WAFER_ERR_STATE and "member 1" in str(e.value)
        assert b.download_phi(1).tobytes() == before.tobytes()


# ---- 8. capacity, and a large batch ----------------------------------------------------------------------------------------
def test_batch_store_capacity_is_per_member(wa, wo):
    shape = (24, 20, 28)
    pars = [wa.Params(*shape, dn=0.3, dt=0.01, max_states=n) for n in (3, 1, 2)]
    cfg, _ = make_pair(shape, dn=0.3, dt=0.01)
    states = orthonormal_store(wo, cfg, 3, seed=5)
    with wa.Batch(pars) as b:
        for k in range(3):
            b.set_potential(k, "Harmonic")
            b.upload_phi(k, states[0])
        b.push_state()
        assert b.num_states() == [1, 1, 1]
        with pytest.raises(wa.WaferError) as e:
            b.push_state()                      # member 1 is full: nothing is pushed anywhere
        assert e.value.code == wa.engine.WAFER_ERR_STATE and "member 1" in str(e.value)
        assert b.num_states() == [1, 1, 1]
        b.push_state([1, 0, 1])
        assert b.num_states() == [2, 1, 2]
        with pytest.raises(wa.WaferError) as e:
            b.load_state(2, 2, states[2])       # past member 2's max_states
        assert e.value.code == wa.engine.WAFER_ERR_STATE and "member 2" in str(e.value)
        b.load_state(2, 1, states[1])           # an existing slot can be overwritten
        b.load_state(0, 2, states[2])
        assert b.num_states() == [3, 1, 2]
        assert np.array_equal(b.download_state(0, 2), states[2]) and np.array_equal(b.download_state(2, 1), states[1])
        assert np.array_equal(b.download_state(1, 0), states[0])
        with pytest.raises(wa.WaferError) as e:
            b.load_state(1, 3, states[1])
        assert "member 1" in str(e.value)
        with pytest.raises(wa.WaferError) as e:
            b.download_state(1, 1)
        assert "member 1" in str(e.value)
        b.clone_state_to_phi(1, active=[1, 0, 1])
        assert np.array_equal(b.download_phi(2), states[1]) and np.array_equal(b.download_phi(1), states[0])
        with pytest.raises(wa.WaferError) as e:
            b.clone_state_to_phi(1)
        assert "member 1" in str(e.value)
        b.clear_states()
        assert b.num_states() == [0, 0, 0]


def test_batch_of_64_at_32_excited(wa, wo):
    shape, wnum = (32, 32, 32), 2
    ms = []
    for k in range(64):
        cfg, par = make_pair(shape, potential="Harmonic" if k % 2 else "Coulomb", dn=0.2, dt=0.002 + 0.00015 * k, mass=1.0 + 0.01 * k)
        ms.append([cfg, par, wo.potential_generate(cfg), wo.potential_sub(cfg), random_phi(cfg, seed=40 + k)])
    stores = [orthonormal_store(wo, m[0], wnum, seed=100 + 10 * k) for k, m in enumerate(ms)]
    with make_batch(wa, ms, stores) as b:
        b.evolve(10, wnum=wnum)
        n2 = b.norm2()
        for k in (0, 27, 63):
            overlaps = check_against_oracle(wo, b, k, ms[k], stores[k], wnum, 10, n2=n2[k])
            assert all(s < 1e-13 for s in overlaps), (k, overlaps)
