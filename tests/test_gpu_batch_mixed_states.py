"""Excited states on mixed-shape batches (wafer_amd.Batch(members, mixed_shapes=True, state_stores=True), wafer_batch_create_mixed_states)
on the MI355X.  The contract is bit equality: a member's phi, stored states and norm2 after any state-store or excited-state call are
what the same member gets in a batch of ITS shape made by wafer_batch_create, under the same gs variant -- in the sequential and in
the one-pass form, on the three dtypes, whatever the other members' shapes, the member's index or the active set -- in the same
number of launches per step for all shapes together.  Through that equality fp64 keeps the oracle tolerances of
tests/test_gpu_batch_states.py (1e-13 per cell, norm2 rel 1e-12), asserted here on the three shapes that file holds to the oracle."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.gpu_common import make_pair, random_phi  # noqa: E402

# tests/test_gpu_batch_mixed.py's shapes: one and two 64-wide x tiles, ragged 4-row y tiles, nz below one 4-plane chunk, a member of
# 4 workgroups beside one of 256 (so the workgroups beyond a member's partition run and leave), each with its own dn, dt, mass, potential
S = [(50, 50, 50), (64, 64, 64), (37, 50, 23), (130, 6, 5), (8, 8, 8), (65, 13, 3)]
SPECS = [
    dict(potential="Harmonic", dn=0.2, dt=0.004, mass=1.0),
    dict(potential="Coulomb", dn=0.25, dt=0.01, mass=0.5),
    dict(potential="host_potsub", dn=0.2, dt=0.003, mass=1.5),   # host V with a pot_sub array
    dict(potential="Harmonic", dn=0.3, dt=0.02, mass=1.0),
    dict(potential="Coulomb", dn=0.2, dt=0.005, mass=2.0),
    dict(potential="host_potsub", dn=0.25, dt=0.006, mass=1.0),
]
ORACLE_SHAPES = (0, 1, 2)   # the members whose shapes tests/test_gpu_batch_states.py holds to the oracle
ALL = tuple(range(len(S)))
STEPS = 25


@pytest.fixture(scope="module")
def wo():
    from oracle import wafer_oracle
    wafer_oracle.build()
    wafer_oracle.set_threads(8)
    return wafer_oracle


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


# ---- helpers (tests/test_gpu_batch_states.py's and tests/test_gpu_batch_mixed.py's, restated) ----------------------------------------
def host_v(cfg):
    """a smooth, non-builtin potential on the padded grid"""
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in cfg.padded_shape], indexing="ij")
    c = [(n - 1) / 2.0 for n in cfg.padded_shape]
    return 0.05 * ((x - c[0]) ** 2 + 0.5 * (y - c[1]) ** 2) * cfg.dn + 0.3 * np.cos(0.4 * z)


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


@functools.lru_cache(maxsize=None)
def member(wo, k, ext, dtype="f64", max_states=4):
    """member k of S: (cfg, par, v, potsub, phi) -- computed once, shared, never written to"""
    s = SPECS[k]
    host = s["potential"] == "host_potsub"
    cfg, par = make_pair(S[k], ext=ext, potential="Harmonic" if host else s["potential"], dn=s["dn"], dt=s["dt"], mass=s["mass"], dtype=dtype,
                         max_states=max_states)
    if host:
        v, potsub = host_v(cfg), (2, 0.0, np.random.default_rng(7 + k).standard_normal(cfg.work_shape))
    else:
        v, potsub = wo.potential_generate(cfg), wo.potential_sub(cfg)
    phi = random_phi(cfg, seed=40 + k)
    for a in (v, phi, potsub[2]):
        if a is not None:
            a.setflags(write=False)
    return cfg, par, v, potsub, phi


@functools.lru_cache(maxsize=None)
def store(wo, k, ext, kind="orthonormal"):
    """member k's store: four orthonormal states (any prefix is orthonormal), or five correlated ones; shared, read-only"""
    cfg = member(wo, k, ext)[0]
    out = orthonormal_store(wo, cfg, 4, seed=100 + 10 * k) if kind == "orthonormal" else correlated_store(wo, cfg, 5, seed=100 + 10 * k)
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def make_batch(wa, wo, ks, ext, nload, dtype="f64", variant=None, mixed=True, max_states=4, kind="orthonormal"):
    """the members ks of S, each with the first `nload` states of its store: a mixed-shape batch with state stores, or (mixed=False:
    all of one shape) a batch made by wafer_batch_create"""
    pars = [member(wo, k, ext, dtype, max_states)[1] for k in ks]
    b = wa.Batch(pars, mixed_shapes=True, state_stores=True) if mixed else wa.Batch(pars)
    if variant is not None:
        b.set_gs_variant(variant)
    for slot, k in enumerate(ks):
        cfg, par, v, potsub, phi = member(wo, k, ext, dtype, max_states)
        b.set_potential_host(slot, np.array(v), potsub[0], potsub[1], None if potsub[2] is None else np.array(potsub[2]))
        b.upload_phi(slot, np.array(phi))
        for i, l in enumerate(store(wo, k, ext, kind)[:nload]):
            b.load_state(slot, i, np.array(l))
    return b


def snapshot(b, nstates, n2=None):
    """-> per member (phi, [its first nstates stored states], norm2)"""
    n2 = b.norm2() if n2 is None else n2
    return [(b.download_phi(s), [b.download_state(s, i) for i in range(nstates)], n2[s]) for s in range(len(b.members))]


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "phi", float(np.max(np.abs(got[0] - want[0]))))
    assert len(got[1]) == len(want[1])
    for i, (g, w) in enumerate(zip(got[1], want[1])):
        assert g.tobytes() == w.tobytes(), (what, "state", i)
    assert got[2] == want[2], (what, "norm2", got[2], want[2])


@functools.lru_cache(maxsize=None)
def one_shape_after(wa, wo, k, ext, wnum, steps, dtype="f64", variant=None, max_states=4, kind="orthonormal", call="evolve"):
    """THE REFERENCE: member k after the call in a batch of its own shape made by wafer_batch_create (computed once per case, shared)"""
    with make_batch(wa, wo, [k], ext, wnum, dtype, variant, mixed=False, max_states=max_states, kind=kind) as b:
        if call == "evolve":
            b.evolve(steps, wnum=wnum)
        elif call == "orthogonalise":
            b.orthogonalise(wnum)
        return snapshot(b, wnum)[0]


def check_oracle(wo, k, ext, wnum, steps, got, kind="orthonormal"):
    """tests/test_gpu_batch_states.py's numbers: 1e-13 per cell, norm2 rel 1e-12"""
    cfg, par, v, potsub, phi = member(wo, k, ext)
    lowers = [np.array(l) for l in store(wo, k, ext, kind)[:wnum]]
    a_, b_ = wo.ab(cfg, np.array(v))
    want = np.array(phi)
    wo.evolve(cfg, wnum, a_, b_, want, lowers, steps)
    err = float(np.max(np.abs(got[0] - want)))
    ref_n2 = wo.norm2(cfg, want)
    print("member", k, "ext", ext, "wnum", wnum, "max|dphi| vs oracle", err, "norm2", got[2], "oracle", ref_n2)
    assert err <= 1e-13, (k, err)
    assert got[2] == pytest.approx(ref_n2, rel=1e-12), k
    for i, l in enumerate(lowers):
        assert got[1][i].tobytes() == l.tobytes(), (k, i)   # the store is read, never written


# ---- 1. evolve, the sequential form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wnum", [1, 2, 3])
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_evolve_sequential_is_the_one_shape_batch_bit_for_bit(wa, wo, ext, wnum):
    with make_batch(wa, wo, ALL, ext, wnum) as b:
        assert b.num_shapes() == len(S) and b.num_states() == [wnum] * len(S)
        b.evolve(STEPS, wnum=wnum)
        assert b.gs_steps() == (0, STEPS)
        got = snapshot(b, wnum)
    for k in ALL:
        same(got[k], one_shape_after(wa, wo, k, ext, wnum, STEPS), (k, S[k]))
    for k in ORACLE_SHAPES:
        check_oracle(wo, k, ext, wnum, STEPS, got[k])


# ---- 2. the one-pass form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wnum", [1, 2, 3, 4])
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_evolve_onepass_is_the_one_shape_batch_bit_for_bit(wa, wo, ext, wnum):
    with make_batch(wa, wo, ALL, ext, wnum, variant=1) as b:
        b.evolve(STEPS, wnum=wnum)
        assert b.gs_steps() == (STEPS, 0)
        got = snapshot(b, wnum)
    for k in ALL:
        same(got[k], one_shape_after(wa, wo, k, ext, wnum, STEPS, variant=1), (k, S[k]))
    for k in ORACLE_SHAPES:
        check_oracle(wo, k, ext, wnum, STEPS, got[k])


def test_wnum_five_falls_back_to_the_sequential_forms_bits(wa, wo):
    kw = dict(max_states=5, kind="correlated")
    with make_batch(wa, wo, ALL, 2, 5, variant=1, **kw) as b:
        d = b.gs_dispatch(5)
        assert d["form"] == "sequential" and d["launches_per_step"] == 1 + 2 * 6 + 1 and d["variant"] == 1, d
        assert b.gs_dispatch(4)["form"] == "onepass"
        b.evolve(6, wnum=5)
        assert b.gs_steps() == (0, 6)
        got = snapshot(b, 5)
    for k in ALL:
        same(got[k], one_shape_after(wa, wo, k, 2, 5, 6, variant=0, **kw), (k, S[k]))


# ---- 3. float storage ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dtype,ext,wnum", [("f32", 1, 2), ("f32fast", 3, 3)])
def test_float_dtypes_are_the_one_shape_batch_bit_for_bit(wa, wo, dtype, ext, wnum, variant):
    with make_batch(wa, wo, ALL, ext, wnum, dtype=dtype, variant=variant) as b:
        assert b.gs_dispatch(wnum)["dtype"] == dtype
        b.evolve(STEPS, wnum=wnum)
        assert b.gs_steps() == ((STEPS, 0) if variant else (0, STEPS))
        got = snapshot(b, wnum)
    for k in ALL:
        same(got[k], one_shape_after(wa, wo, k, ext, wnum, STEPS, dtype=dtype, variant=variant), (dtype, k, S[k]))
        for i, l in enumerate(store(wo, k, ext)[:wnum]):   # what was loaded, rounded to float once
            assert np.array_equal(got[k][1][i], l.astype(np.float32).astype(np.float64)), (k, i)


# ---- 4. independence ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [None, 1])
def test_member_bits_do_not_depend_on_the_batch(wa, wo, variant):
    ext, wnum = 1, 2
    want = [one_shape_after(wa, wo, k, ext, wnum, STEPS, variant=variant) for k in ALL]   # test 1's / test 2's results
    for _ in range(2):                                  # the same call twice
        with make_batch(wa, wo, ALL, ext, wnum, variant=variant) as b:
            b.evolve(STEPS, wnum=wnum)
            for k, g in enumerate(snapshot(b, wnum)):
                same(g, want[k], ("again", k))
    order = [3, 4, 0, 5, 1, 2]                          # members in another order
    with make_batch(wa, wo, order, ext, wnum, variant=variant) as b:
        b.evolve(STEPS, wnum=wnum)
        for slot, g in enumerate(snapshot(b, wnum)):
            same(g, want[order[slot]], ("order", slot))
    for mask in ([1, 0, 0, 1, 0, 0], [0, 1, 0, 0, 1, 1], [0, 0, 0, 0, 1, 0]):   # the others frozen, then the complement
        with make_batch(wa, wo, ALL, ext, wnum, variant=variant) as b:
            b.evolve(STEPS, active=mask, wnum=wnum)
            for k in ALL:
                got = b.download_phi(k)
                if mask[k]:
                    assert np.array_equal(got, want[k][0]), (mask, k)
                else:
                    assert got.tobytes() == member(wo, k, ext)[4].tobytes(), (mask, k)
                for i, l in enumerate(store(wo, k, ext)[:wnum]):
                    assert b.download_state(k, i).tobytes() == l.tobytes(), (mask, k, i)
            b.evolve(STEPS, active=[1 - x for x in mask], wnum=wnum)
            for k, g in enumerate(snapshot(b, wnum)):
                same(g, want[k], (mask, "complement", k))
    shared = [0, 5, 4, 0, 5]                            # members that share shapes pairwise: two of 50^3, two of (65, 13, 3), one 8^3
    with make_batch(wa, wo, shared, ext, wnum, variant=variant) as b:
        assert b.num_shapes() == 3
        b.evolve(STEPS, wnum=wnum)
        for slot, g in enumerate(snapshot(b, wnum)):
            same(g, want[shared[slot]], ("shared", slot))


# ---- 5. orthogonalise and norm2 alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("ext,wnum", [(1, 3), (3, 2)])
def test_orthogonalise_and_norm2_alone(wa, wo, ext, wnum, variant):
    with make_batch(wa, wo, ALL, ext, wnum, variant=variant) as b:
        before = b.norm2()
        for k in ALL:
            with make_batch(wa, wo, [k], ext, wnum, variant=variant, mixed=False) as u:
                assert before[k] == u.norm2()[0], k
        with pytest.raises(wa.WaferError) as e:
            b.orthogonalise(wnum + 1)   # every store is too short
        assert e.value.code == wa.engine.WAFER_ERR_STATE and "member 0" in str(e.value)
        for k in ALL:                   # ... and nothing has changed
            assert b.download_phi(k).tobytes() == member(wo, k, ext)[4].tobytes(), k
        assert b.norm2() == before and b.gs_steps() == (0, 0)
        b.orthogonalise(wnum)
        assert b.gs_steps() == ((1, 0) if variant else (0, 1))
        got = snapshot(b, wnum)
    for k in ALL:
        same(got[k], one_shape_after(wa, wo, k, ext, wnum, 0, variant=variant, call="orthogonalise"), (k, S[k]))


# ---- 6. the store calls --------------------------------------------------------------------------------------------------------------------
def test_store_calls_and_capacity_per_member(wa, wo):
    ext = 1
    caps = [3, 1, 2, 3, 2, 3]
    pars = [make_pair(S[k], ext=ext, dn=SPECS[k]["dn"], dt=SPECS[k]["dt"], max_states=caps[k])[1] for k in ALL]
    with wa.Batch(pars, mixed_shapes=True, state_stores=True) as b:
        for k in ALL:
            b.set_potential(k, "Harmonic")
            b.upload_phi(k, np.array(store(wo, k, ext)[0]))
        assert b.num_states() == [0] * 6
        b.push_state()
        assert b.num_states() == [1] * 6
        for k in ALL:
            assert b.download_state(k, 0).tobytes() == store(wo, k, ext)[0].tobytes(), k
        with pytest.raises(wa.WaferError) as e:
            b.push_state()                              # member 1 is full: nothing is pushed anywhere
        assert e.value.code == wa.engine.WAFER_ERR_STATE and "member 1" in str(e.value)
        assert b.num_states() == [1] * 6
        b.push_state([1, 0, 1, 0, 0, 1])                # with a mask
        assert b.num_states() == [2, 1, 2, 1, 1, 2]
        with pytest.raises(wa.WaferError) as e:
            b.load_state(2, 2, np.array(store(wo, 2, ext)[2]))   # past member 2's max_states
        assert e.value.code == wa.engine.WAFER_ERR_STATE and "member 2" in str(e.value)
        b.load_state(2, 1, np.array(store(wo, 2, ext)[1]))       # an existing slot can be overwritten
        b.load_state(0, 2, np.array(store(wo, 0, ext)[2]))
        b.load_state(3, 1, np.array(store(wo, 3, ext)[1]))
        assert b.num_states() == [3, 1, 2, 2, 1, 2]
        for k, i in ((0, 2), (2, 1), (3, 1), (1, 0), (5, 1)):
            want = store(wo, k, ext)[i if (k, i) != (5, 1) else 0]   # (member 5's state 1 is its pushed phi: its state 0)
            assert b.download_state(k, i).tobytes() == want.tobytes(), (k, i)
        with pytest.raises(wa.WaferError) as e:
            b.download_state(4, 1)
        assert "member 4" in str(e.value)
        b.clone_state_to_phi(1, active=[0, 0, 1, 1, 0, 0])
        assert b.download_phi(2).tobytes() == store(wo, 2, ext)[1].tobytes() and b.download_phi(3).tobytes() == store(wo, 3, ext)[1].tobytes()
        assert b.download_phi(0).tobytes() == store(wo, 0, ext)[0].tobytes()
        with pytest.raises(wa.WaferError) as e:
            b.clone_state_to_phi(1)
        assert "member 1" in str(e.value)
        b.clear_states([0, 0, 1, 0, 1, 0])              # with a mask
        assert b.num_states() == [3, 1, 0, 2, 0, 2]
        assert b.download_state(0, 2).tobytes() == store(wo, 0, ext)[2].tobytes()
        b.clear_states()
        assert b.num_states() == [0] * 6


def test_gram_matrix_is_fresh_after_load_push_clear(wa, wo):
    """a step under the one-pass form after each edit of the stores is the one-shape batch's after the same edits"""
    ext = 2
    ks = [0, 3, 4, 5]

    def edits(b, members):
        """-> the snapshots after a one-pass step that follows each edit; members: the member of S in each slot of b"""
        out = []

        def step(wnum):
            b.evolve(1, wnum=wnum)
            out.append(snapshot(b, wnum))
        step(2)                                                           # the matrices of the loaded stores
        for slot, k in enumerate(members):                                # load: state 1 replaced by another correlated one
            b.load_state(slot, 1, np.array(store(wo, k, ext, "correlated")[3]))
        step(2)
        b.push_state()                                                    # push: phi becomes state 2
        step(3)
        b.clear_states()                                                  # clear, then a store of one state: no pair
        for slot, k in enumerate(members):
            b.load_state(slot, 0, np.array(store(wo, k, ext, "correlated")[2]))
        step(1)
        return out

    with make_batch(wa, wo, ks, ext, 2, variant=1, kind="correlated") as b:
        got = edits(b, ks)
        assert b.gs_steps() == (4, 0)
    for s, k in enumerate(ks):
        with make_batch(wa, wo, [k], ext, 2, variant=1, mixed=False, kind="correlated") as u:
            want = edits(u, [k])
        for n, (g, w) in enumerate(zip(got, want)):
            same(g[s], w[0], ("edit", n, k))


# ---- 7. solve_state ------------------------------------------------------------------------------------------------------------------------
# Small cubic Harmonic members of three sizes (cubes keep the first excited level exactly degenerate, so no phase crawls between two
# nearly degenerate states), tolerance and screen_update of tests/test_gpu_batch_states.py::test_batch_solve_states_match_oracle.
# Member 3 (a second member of the first shape) has a time step so small that it is at tau = 2 when max_steps runs out, where the
# energy still falls by ~1e-4 per block: it ends phase 0 in MaxStep, is not pushed, and so has a short store in phases 1 and 2.
SOLVE_SHAPES = [(20, 20, 20), (24, 24, 24), (16, 16, 16), (20, 20, 20)]
SOLVE_DTS = [0.032, 0.02, 0.026, 0.0001]
SOLVE_ARGS = dict(tolerance=1e-9, screen_update=100, max_steps=20000)


def test_solve_state_phases_match_the_one_shape_batches(wa, wo):
    pairs = [make_pair(s, ext=1, potential="Harmonic", dn=0.4, dt=dt, mass=1.0) for s, dt in zip(SOLVE_SHAPES, SOLVE_DTS)]
    groups = [[0, 3], [1], [2]]   # the members of each shape: the one-shape batches
    batches = [wa.Batch([p[1] for p in pairs], mixed_shapes=True, state_stores=True)] + [wa.Batch([pairs[k][1] for k in g]) for g in groups]
    try:
        mixed, uniform = batches[0], batches[1:]
        assert mixed.num_shapes() == 3
        where = {k: (u, g.index(k)) for u, g in zip(uniform, groups) for k in g}
        for k in range(4):
            mixed.set_potential(k, "Harmonic")
            where[k][0].set_potential(where[k][1], "Harmonic")
        for wnum in range(3):
            for k, (cfg, par) in enumerate(pairs):
                phi = wo.initial_condition(cfg, "Gaussian", seed=3 + wnum)
                mixed.upload_phi(k, phi)
                where[k][0].upload_phi(where[k][1], phi)
            got = mixed.solve_state(wnum, **SOLVE_ARGS)
            want = [u.solve_state(wnum, **SOLVE_ARGS) for u in uniform]
            for k in range(4):
                u, slot = where[k]
                w = want[uniform.index(u)][slot]
                print("state", wnum, "member", k, "rows", len(got[k][0]), "converged", got[k][2], "status", got[k][3])
                assert got[k] == w, (wnum, k)                      # records, final, converged, status
                assert mixed.download_phi(k).tobytes() == u.download_phi(slot).tobytes(), (wnum, k)
                assert mixed.num_states()[k] == u.num_states()[slot], (wnum, k)
            status = [r[3] for r in got]
            if wnum == 0:
                assert status == [wa.engine.WAFER_OK] * 3 + [wa.engine.WAFER_ERR_MAX_STEP], status
            else:   # the short store is member 3's status, not the call's; it is left as it stands
                assert status == [wa.engine.WAFER_OK] * 3 + [wa.engine.WAFER_ERR_STATE] and got[3][0] == [], status
            assert [r[2] for r in got] == [True, True, True, False]
            assert mixed.num_states() == [wnum + 1] * 3 + [0]
        for k in range(3):
            for i in range(3):
                u, slot = where[k]
                assert mixed.download_state(k, i).tobytes() == u.download_state(slot, i).tobytes(), (k, i)
    finally:
        for b in batches:
            b.close()


# ---- 8. unchanged contracts ----------------------------------------------------------------------------------------------------------------
def test_unchanged_contracts_and_dispatch(wa, wo):
    ext, wnum = 1, 2
    pars = [member(wo, k, ext)[1] for k in ALL]
    with wa.Batch(pars, mixed_shapes=True) as b:        # wafer_batch_create_mixed still refuses
        with pytest.raises(wa.WaferError) as e:
            b.load_state(0, 0, np.array(store(wo, 0, ext)[0]))
        assert e.value.code == wa.engine.WAFER_ERR_INVALID and "mixed-shape" in str(e.value) and "wafer_batch_load_state" in str(e.value)
        assert "shapes" not in b.gs_dispatch(wnum)
    with pytest.raises(ValueError):
        wa.Batch(pars, state_stores=True)
    # one distinct shape: wafer_batch_create's dispatch lines and bits
    one = [make_pair(S[2], ext=ext, dn=0.2, dt=0.003 + 0.001 * i, max_states=4)[1] for i in range(3)]
    with wa.Batch(one, mixed_shapes=True, state_stores=True) as b, wa.Batch(one) as u:
        assert b.num_shapes() == 1
        for x in (b, u):
            x.set_gs_variant(1)
            for i in range(3):
                x.set_potential(i, "Harmonic")
                x.upload_phi(i, np.array(member(wo, 2, ext)[4]))
                for j, l in enumerate(store(wo, 2, ext)[:wnum]):
                    x.load_state(i, j, np.array(l))
        assert b.dispatch() == u.dispatch() and "shapes" not in b.dispatch()
        for w in (0, 1, 2, 5):
            assert b.gs_dispatch(w) == u.gs_dispatch(w) and "shapes" not in b.gs_dispatch(w)
        for x in (b, u):
            x.evolve(5, wnum=wnum)
        assert b.gs_dispatch(wnum) == u.gs_dispatch(wnum)   # (onepass_bytes too: the same allocations)
        for g, w in zip(snapshot(b, wnum), snapshot(u, wnum)):
            same(g, w, "one shape")
        one_kernels = {}   # the one-shape kernels= fields, (gs variant, wnum): what the several-shape lines below must differ from
        for variant in (0, 1):
            u.set_gs_variant(variant)
            for w in (1, 2, 3, 4):
                one_kernels[variant, w] = u.gs_dispatch(w)["kernels"]
                assert "WaferBatchGeomTable" not in one_kernels[variant, w]
    # several shapes: the table-reading instantiations, the launch counts, shapes=6
    with make_batch(wa, wo, ALL, ext, wnum) as b:
        for w in (1, 2, 3):
            d = b.gs_dispatch(w)
            assert d["form"] == "sequential" and d["launches_per_step"] == 1 + 2 * (1 + w) + 1 and d["shapes"] == 6, d
            assert "wafer_k_batch_gs<NORM2|SCALE|AXPY,double,WaferBatchGeomTable>" in d["kernels"], d
            assert d["kernels"].endswith("+wafer_k_batch_gs_reduce") and d["kernels"] != one_kernels[0, w], d
        assert b.gs_dispatch(0)["launches_per_step"] == 1 and b.gs_dispatch(0)["shapes"] == 6
        b.set_gs_variant(1)
        for w in (1, 2, 3, 4):
            d = b.gs_dispatch(w)
            assert d["form"] == "onepass" and d["launches_per_step"] == 4 and d["shapes"] == 6 and d["onepass_bytes"] == 0, d
            assert "wafer_k_batch_gs_sums<%d,double,WaferBatchGeomTable>" % w in d["kernels"], d
            assert "wafer_k_batch_gs_apply<%d,double,true,WaferBatchGeomTable>" % w in d["kernels"], d
            assert "+wafer_k_batch_gs_reduce_sums+" in d["kernels"] and d["kernels"] != one_kernels[1, w], d
        b.evolve(1, wnum=wnum)
        assert b.gs_dispatch(wnum)["onepass_bytes"] > 0
        b.set_gs_variant(-1)
        assert b.gs_dispatch(wnum)["form"] == "sequential"
        assert int(b.dispatch()["shapes"]) == 6
