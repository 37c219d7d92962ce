"""The one-pass form of the batched excited step (Batch.set_gs_variant(1): step, raw sums, reduce, one apply pass with the member's
Gram matrix) on the MI355X.  fp64: every member against the oracle's excited-state evolve and a Context to the bars of
tests/test_gpu_batch_states.py; float dtypes: the model of tests/batch_onepass_model.py within the bar of
tests/test_gpu_batch_fp32.py's `_within`; a member's bits independent of the batch around it; the Gram matrix fresh after every
change of a store; and nothing changed under the default variant.  Every case asserts through gs_steps() that the form it means
to test is the one that ran."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import batch_fp32_model as chain  # noqa: E402
from tests import batch_onepass_model as onepass  # noqa: E402
from tests import test_gpu_batch_fp32 as f32t  # noqa: E402
from tests import test_gpu_batch_states as st  # noqa: E402

SHAPES = [(65, 33, 20), (37, 50, 23), (64, 64, 64)]   # two x-tiles and ragged y; sub-tile x, ragged y, nz % 4 != 0; exact tiles
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


def sid(shape):
    return "x".join(map(str, shape))


def onepass_batch(wa, ms, stores, order=None):
    b = st.make_batch(wa, ms, stores, order)
    b.set_gs_variant(1)
    return b


def correlated_store(wo, cfg, wnum, seed):
    """normalised states with pairwise overlaps of about 0.4: each random state normalised, 0.4 x the first added, normalised
    again (tests/test_gpu_batch_states.py's store of that name adds 0.4 x the first to an un-normalised state: overlaps ~0.01)"""
    lowers = []
    for i in range(wnum):
        l = st.random_phi(cfg, seed=seed + i)
        wo.normalise(l, wo.norm2(cfg, l))
        if lowers:
            l = l + 0.4 * lowers[0]
            wo.normalise(l, wo.norm2(cfg, l))
        lowers.append(np.ascontiguousarray(l))
    return lowers


def ran_onepass(b, n):
    """n excited steps / orthogonalise calls since creation, all in the one-pass form"""
    assert b.gs_steps() == (n, 0), b.gs_steps()


# ---- 1. against the oracle and contexts -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wnum", [1, 2, 3, 4])
@pytest.mark.parametrize("ext", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_onepass_evolve_matches_oracle_and_contexts(wa, wo, shape, ext, wnum):
    ms, stores = st.problems(wo, shape, ext, wnum)
    with onepass_batch(wa, ms, stores) as b:
        d = b.gs_dispatch(wnum)
        assert d["form"] == "onepass" and d["launches_per_step"] == 4 and d["wnum"] == wnum and d["variant"] == 1, d
        assert d["onepass_bytes"] == 0, d   # allocated by the first one-pass call, not by selecting the form
        b.evolve(STEPS, wnum=wnum)
        ran_onepass(b, STEPS)
        assert b.gs_dispatch(wnum)["onepass_bytes"] > 0
        n2 = b.norm2()
        for k, m in enumerate(ms):
            overlaps = st.check_against_oracle(wo, b, k, m, stores[k], wnum, STEPS, atol=1e-13, rel=1e-12, n2=n2[k])
            assert all(s < 1e-13 for s in overlaps), (k, overlaps)
            for i, l in enumerate(stores[k]):   # the store is read, never written
                assert np.array_equal(b.download_state(k, i), l), (k, i)
            with st.make_context(wa, m, stores[k]) as ctx:
                ctx.evolve(wnum, STEPS)
                want, want_n2 = ctx.download_phi(), ctx.norm2()
            err = float(np.max(np.abs(b.download_phi(k) - want)))
            print("member", k, "vs context max|dphi|", err, "norm2", n2[k], "context", want_n2)
            assert err <= 1e-13, (k, err)
            assert n2[k] == pytest.approx(want_n2, rel=1e-12), k


# ---- 2. a correlated store, and the fallback ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wnum", [2, 4])
def test_onepass_evolve_correlated_store(wa, wo, wnum):
    ms, stores = st.problems(wo, (26, 19, 23), 2, wnum, max_states=5, store=correlated_store)
    assert abs(float(np.sum(stores[0][1] * stores[0][0]))) > 0.3   # the Gram matrix matters
    with onepass_batch(wa, ms, stores) as b:
        b.evolve(6, wnum=wnum)
        ran_onepass(b, 6)
        for k, m in enumerate(ms):
            st.check_against_oracle(wo, b, k, m, stores[k], wnum, 6, atol=2e-13, rel=1e-11)


def test_wnum_above_four_falls_back_to_the_sequential_form(wa, wo):
    ms, stores = st.problems(wo, (26, 19, 23), 2, 5, max_states=5, store=correlated_store)
    with onepass_batch(wa, ms, stores) as b1, st.make_batch(wa, ms, stores) as b0:
        b0.set_gs_variant(0)
        d = b1.gs_dispatch(5)
        assert d["form"] == "sequential" and d["launches_per_step"] == 1 + 2 * 6 + 1 and d["variant"] == 1, d
        assert b1.gs_dispatch(4)["form"] == "onepass"
        for b in (b0, b1):
            b.evolve(6, wnum=5)
        assert b1.gs_steps() == (0, 6) and b0.gs_steps() == (0, 6)
        for k in range(len(ms)):
            assert b1.download_phi(k).tobytes() == b0.download_phi(k).tobytes(), k


# ---- 3. orthogonalise alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ext,wnum", [((65, 33, 20), 1, 3), ((64, 64, 64), 2, 4), ((37, 50, 23), 3, 1)])
def test_onepass_orthogonalise_matches_oracle_and_contexts(wa, wo, shape, ext, wnum):
    ms, stores = st.problems(wo, shape, ext, wnum)
    mask = [0, 1, 0, 1, 1]
    with onepass_batch(wa, ms, stores) as b, onepass_batch(wa, ms, stores) as bm:
        b.orthogonalise(wnum)
        bm.orthogonalise(wnum, active=mask)
        ran_onepass(b, 1)
        ran_onepass(bm, 1)
        for k, m in enumerate(ms):
            with st.make_context(wa, m, stores[k]) as ctx:
                ctx.orthogonalise(wnum)
                want = ctx.download_phi()
            want_o = m[4].copy()
            wo.orthogonalise(wnum, want_o, stores[k])
            got = b.download_phi(k)
            print("member", k, "vs context", float(np.max(np.abs(got - want))), "vs oracle", float(np.max(np.abs(got - want_o))))
            assert np.allclose(got, want, rtol=0, atol=1e-14), k
            assert np.allclose(got, want_o, rtol=0, atol=1e-14), k
            assert bm.download_phi(k).tobytes() == (got if mask[k] else m[4]).tobytes(), k
            for i, l in enumerate(stores[k]):
                assert bm.download_state(k, i).tobytes() == l.tobytes(), (k, i)


# ---- 4. independence and determinism, exact ----------------------------------------------------------------------------------------------
def independence(make, B, starts, nstates, steps, wnum, order, masks):
    """make(order) -> a one-pass batch of the members order[slot]; starts[k]: member k's uploaded phi (as the batch holds it)"""
    with make(range(B)) as b:
        b.evolve(steps, wnum=wnum)
        ran_onepass(b, steps)
        full = [b.download_phi(k) for k in range(B)]
        full_n2 = b.norm2()
        states = [[b.download_state(k, i) for i in range(nstates)] for k in range(B)]
    with make(range(B)) as b:               # the same call from the same start: the same bits
        b.evolve(steps, wnum=wnum)
        for k in range(B):
            assert np.array_equal(b.download_phi(k), full[k]), k
        assert b.norm2() == full_n2
    for k in range(B):                      # alone in a batch of one
        with make([k]) as b:
            b.evolve(steps, wnum=wnum)
            ran_onepass(b, steps)
            assert np.array_equal(b.download_phi(0), full[k]), k
            assert b.norm2()[0] == full_n2[k], k
    with make(order) as b:                  # at another index
        b.evolve(steps, wnum=wnum)
        for slot, k in enumerate(order):
            assert np.array_equal(b.download_phi(slot), full[k]), k
    for mask in masks:                      # with the others frozen
        with make(range(B)) as b:
            b.evolve(steps, active=mask, wnum=wnum)
            for k in range(B):
                got = b.download_phi(k)
                if mask[k]:
                    assert np.array_equal(got, full[k]), (mask, k)
                else:
                    assert got.tobytes() == starts[k].tobytes(), (mask, k)
                for i in range(nstates):
                    assert b.download_state(k, i).tobytes() == states[k][i].tobytes(), (mask, k, i)
            b.evolve(steps, active=[1 - x for x in mask], wnum=wnum)   # the frozen members continue from where they stood
            ran_onepass(b, 2 * steps)
            for k in range(B):
                assert np.array_equal(b.download_phi(k), full[k]), (mask, k)


@pytest.mark.parametrize("shape,ext,wnum", [((65, 33, 20), 1, 2), ((64, 64, 64), 1, 3), ((37, 50, 23), 2, 1), ((64, 64, 64), 3, 4)],
                         ids=lambda v: sid(v) if isinstance(v, tuple) else None)
def test_onepass_member_bits_do_not_depend_on_the_batch(wa, wo, shape, ext, wnum):
    ms, stores = st.problems(wo, shape, ext, wnum)
    independence(lambda order: onepass_batch(wa, ms, stores, list(order)), len(ms), [m[4] for m in ms], wnum, STEPS, wnum,
                 [3, 4, 0, 1, 2], ([1, 0, 0, 1, 0], [0, 1, 1, 0, 1], [0, 0, 1, 0, 0]))


def float_batch(wa, wo, dtype, shape, ext, wnum, order=None, variant=1):
    """tests/test_gpu_batch_fp32.py's batch of batch_fp32_model.MEMBERS with their float stores loaded"""
    order = list(range(f32t.NM)) if order is None else list(order)
    b = f32t.make_batch(wa, wo, dtype, shape, ext, order=order)
    if variant is not None:
        b.set_gs_variant(variant)
    for slot, k in enumerate(order):
        for i, l in enumerate(chain.stored_states(f32t.inputs(wo, k, shape, ext)[0], k, wnum)):
            b.load_state(slot, i, l)
    return b


@pytest.mark.parametrize("shape,ext,wnum", [((65, 33, 20), 1, 2), ((33, 20, 11), 3, 4)], ids=lambda v: sid(v) if isinstance(v, tuple) else None)
def test_onepass_member_bits_do_not_depend_on_the_batch_f32(wa, wo, shape, ext, wnum):
    starts = [f32t.inputs(wo, k, shape, ext)[2] for k in range(f32t.NM)]
    independence(lambda order: float_batch(wa, wo, "f32", shape, ext, wnum, order), f32t.NM, starts, wnum, 8, wnum,
                 [2, 0, 1], ([1, 0, 0], [0, 1, 1], [0, 0, 1]))


# ---- 5. the Gram matrix follows the store -------------------------------------------------------------------------------------------------
def test_gram_matrix_is_fresh_after_every_change_of_a_store(wa, wo):
    shape, ext = (37, 50, 23), 1
    ms, stores = st.problems(wo, shape, ext, 3, store=correlated_store)
    other = correlated_store(wo, ms[2][0], 3, seed=900)   # what member 2's slots get later

    def fresh(phis, stores_now, wnum, steps):
        """a new batch holding these wavefunctions and stores, evolved: the bits a current Gram matrix gives"""
        with onepass_batch(wa, [m[:4] + [phi] for m, phi in zip(ms, phis)], stores_now) as f:
            f.evolve(steps, wnum=wnum)
            ran_onepass(f, steps)
            return [f.download_phi(k) for k in range(len(ms))]

    def same(b, want, what):
        for k in range(len(ms)):
            assert b.download_phi(k).tobytes() == want[k].tobytes(), (what, k)

    with onepass_batch(wa, ms, [s[:2] for s in stores]) as b:
        now = [s[:2] for s in stores]
        b.evolve(5, wnum=2)                                   # forms every member's Gram matrix
        # load_state over slot 1 of one member
        b.load_state(2, 1, other[1])
        now[2] = [now[2][0], other[1]]
        phis = [b.download_phi(k) for k in range(len(ms))]
        b.evolve(5, wnum=2)
        same(b, fresh(phis, now, 2, 5), "after load_state")
        # push_state: phi becomes state 2 of every member
        phis = [b.download_phi(k) for k in range(len(ms))]
        b.push_state()
        now = [s + [phi] for s, phi in zip(now, phis)]
        b.evolve(5, wnum=3)
        same(b, fresh(phis, now, 3, 5), "after push_state")
        # clear_states of two members and a reload with other states
        b.clear_states([0, 1, 1, 0, 0])
        for k in (1, 2):
            now[k] = [other[2], stores[k][2], other[0]] if k == 2 else [stores[k][1], stores[k][2], stores[k][0]]
            for i, l in enumerate(now[k]):
                b.load_state(k, i, l)
        phis = [b.download_phi(k) for k in range(len(ms))]
        b.evolve(5, wnum=3)
        same(b, fresh(phis, now, 3, 5), "after clear_states and a reload")
        ran_onepass(b, 20)


def test_onepass_solve_states_match_oracle(wa, wo):
    """tests/test_gpu_batch_states.py::test_batch_solve_states_match_oracle under variant 1, with its bars: solve_state pushes
    what converged, and the next state's steps must see the Gram matrix of the grown store"""
    b, ms = st.solve_setup(wa, wo)
    with b:
        b.set_gs_variant(1)
        stores = [[] for _ in ms]
        energies = [[] for _ in ms]
        for wnum in range(3):
            phis = st.upload_guess(wo, b, ms, wnum)
            got = b.solve_state(wnum, **st.SOLVE_ARGS)
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
        for k in range(len(ms)):
            assert energies[k][0] == pytest.approx(1.5, abs=0.02), k
            assert energies[k][1] == pytest.approx(2.5, abs=0.04) and energies[k][2] == pytest.approx(2.5, abs=0.04), k
        one, seq = b.gs_steps()
        assert one > 0 and seq == 0, (one, seq)


# ---- 6. float dtypes against the one-pass model --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", onepass.FLOAT_SHAPES, ids=sid)
@pytest.mark.parametrize("ext", [1, 2, 3])
@pytest.mark.parametrize("wnum", [1, 2, 3])
def test_float_dtypes_follow_the_onepass_model(wa, wo, wnum, ext, shape):
    """orthogonalise(wnum) alone, then evolve(steps, wnum) for 1 and 4 steps from the uploaded start, every member, f32 and f32fast:
    within max(1, 4 D_ref) float spacings of the exact-scalar model and at most 1 % of the work cells differing from it
    (tests/test_gpu_batch_fp32.py's `_within`; tests/test_batch_onepass_host.py holds D_ref <= 1 and the model's own flips to
    1 %: measured there over this table's shapes, exts, wnums and members, D_ref <= 0.75 and at most 0.12 % of the cells), every value a float, and f32fast equal to f32 bit for bit"""
    models = [onepass.float_models(wo, k, shape, ext, wnum) for k in range(f32t.NM)]
    got = {}
    for dtype in f32t.DTYPES:
        with float_batch(wa, wo, dtype, shape, ext, wnum) as b:
            assert b.gs_dispatch(wnum)["form"] == "onepass" and b.gs_dispatch(wnum)["dtype"] == dtype
            b.orthogonalise(wnum)
            got[dtype, "orthogonalise"] = [b.download_phi(k) for k in range(f32t.NM)]
            for k, (cfg, lowers, _) in enumerate(models):
                for i, l in enumerate(lowers):   # the store is read, never written
                    assert np.array_equal(b.download_state(k, i), l), (k, i)
            for steps in onepass.FLOAT_STEPS:
                for k in range(f32t.NM):
                    b.upload_phi(k, f32t.inputs(wo, k, shape, ext)[2])
                b.evolve(steps, wnum=wnum)
                got[dtype, steps] = [b.download_phi(k) for k in range(f32t.NM)]
            ran_onepass(b, 1 + sum(onepass.FLOAT_STEPS))
    for what in ("orthogonalise",) + tuple(onepass.FLOAT_STEPS):
        for k, (cfg, _, out) in enumerate(models):
            f32t._within(got["f32", what][k], cfg, *out[what], f"f32 {what} member {k}")
            f32t.equal(got["f32fast", what][k], got["f32", what][k], ext, f"f32fast against f32, {what}, member {k}")


# ---- 7. the default is unchanged ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32", "f32fast"])
def test_default_variant_is_the_sequential_form(wa, wo, dtype):
    shape, ext, wnum = (65, 33, 20), 1, 2
    out = {}
    for variant in (None, -1, 0):
        for op in ("evolve", "orthogonalise"):
            with float_batch(wa, wo, dtype, shape, ext, wnum, variant=None) as b:   # (on f64 the float inputs are held as doubles)
                if variant is not None:
                    b.set_gs_variant(variant)
                d = b.gs_dispatch(wnum)
                assert d["form"] == "sequential" and d["launches_per_step"] == 1 + 2 * (1 + wnum) + 1 and d["onepass_bytes"] == 0, d
                if op == "evolve":
                    b.evolve(6, wnum=wnum)
                else:
                    b.orthogonalise(wnum)
                assert b.gs_steps() == (0, 6 if op == "evolve" else 1)
                assert b.gs_dispatch(wnum)["onepass_bytes"] == 0
                out[variant, op] = [b.download_phi(k).tobytes() for k in range(f32t.NM)]
    for op in ("evolve", "orthogonalise"):
        assert out[None, op] == out[-1, op] == out[0, op], op


def test_gs_variant_outside_the_range_is_invalid(wa, wo):
    with f32t.make_batch(wa, wo, "f64", (17, 17, 17), 1) as b:
        for v in (2, -2):
            with pytest.raises(wa.WaferError) as e:
                b.set_gs_variant(v)
            assert e.value.code == wa.engine.WAFER_ERR_INVALID
        b.set_gs_variant(1)
        assert b.gs_dispatch(1)["variant"] == 1


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ground_state_batch_is_untouched_by_the_variant(wa, wo, dtype):
    shape, ext, out = (65, 33, 20), 1, {}
    for variant in (-1, 0, 1):
        with f32t.make_batch(wa, wo, dtype, shape, ext) as b:
            b.set_gs_variant(variant)
            b.evolve(7)
            b.evolve(3, wnum=0)
            assert b.gs_steps() == (0, 0)
            d = b.gs_dispatch(0)
            assert d["form"] == "sequential" and d["launches_per_step"] == 1 and d["onepass_bytes"] == 0, d
            out[variant] = [b.download_phi(k).tobytes() for k in range(f32t.NM)]
    assert out[-1] == out[0] == out[1]
