"""Float-storage batches (wafer_amd.Batch with dtype "f32" / "f32fast") on the MI355X.

Ground state: every member's bits are those of tests/fp32_reference.py (a, b formed from the stored V in the arithmetic type,
every step rounded to float) and of a Context of that dtype under default dispatch -- one step per launch and fused passes alike;
observables and normalise to the bit as well.  Excited states: the chain model of tests/batch_fp32_model.py on float storage,
within a bar taken from the model alone.  tests/test_batch_fp32_host.py holds the inputs to the f32fast reference's domain and
the chain model to the oracle."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import batch_fp32_model as model  # noqa: E402
from tests import fp32_reference as ref  # noqa: E402

DTYPES = ["f32", "f32fast"]
NM = len(model.MEMBERS)


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


def params(wa, cfg, dtype, **kw):
    return wa.Params(cfg.nx, cfg.ny, cfg.nz, dn=cfg.dn, dt=cfg.dt, mass=cfg.mass, sig=cfg.sig, central_difference=cfg.ext, dtype=dtype, **kw)


@functools.lru_cache(maxsize=None)
def inputs(wo, k, shape, ext):
    cfg, v, phi = model.member_inputs(wo, k, shape, ext)
    return cfg, v, phi, wo.potential_sub(cfg)


@functools.lru_cache(maxsize=None)
def reference(wo, dtype, k, shape, ext):
    cfg, v, phi, _ = inputs(wo, k, shape, ext)
    want, _ = ref.evolve(wo, cfg, v, phi, model.STEP_COUNTS, dtype, ab="registers")
    return want


def make_batch(wa, wo, dtype, shape, ext, order=None, variant=None, phi=True, **kw):
    """members order[slot] of the table (default: 0, 1, 2) with their potentials and starts"""
    order = list(range(NM)) if order is None else list(order)
    ms = [inputs(wo, k, shape, ext) for k in order]
    b = wa.Batch([params(wa, m[0], dtype, **kw) for m in ms])
    if variant is not None:
        b.set_step_variant(variant)
    for slot, (cfg, v, start, potsub) in enumerate(ms):
        b.set_potential_host(slot, v, potsub[0], potsub[1], potsub[2])
        if phi:
            b.upload_phi(slot, start)
    return b


def make_context(wa, wo, dtype, k, shape, ext, **kw):
    cfg, v, start, potsub = inputs(wo, k, shape, ext)
    ctx = wa.Context(params(wa, cfg, dtype, **kw))
    ctx.set_potential_host(v, potsub[0], potsub[1], potsub[2])
    ctx.upload_phi(start)
    return ctx


def equal(got, want, ext, what):
    msg = ref.describe_mismatch(got, want, ext)
    assert msg is None, f"{what}: {msg}"


def sid(shape):
    return "x".join(map(str, shape))


# ---- 1. ground-state evolve against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1, -1])
@pytest.mark.parametrize("shape", model.SHAPES, ids=sid)
@pytest.mark.parametrize("ext", [1, 2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ground_state_evolve_equals_the_reference(wa, wo, dtype, ext, shape, variant):
    """after 1, 2, 3, 7, 8 and 12 steps from the uploaded start, every member, np.array_equal on the whole array (so the frame is
    zero), one step per launch (0), fused passes (1) and the default (-1).  That the instantiation of the batch's own dtype ran
    is shown by the bits, not by the dispatch line (which is built from the dtype): on every shape of more than a few cells the
    two dtypes' references differ after one step already, so the other dtype's kernel could not pass."""
    if np.prod(shape) > 1:
        for k in range(NM):
            assert not np.array_equal(reference(wo, "f32", k, shape, ext)[1], reference(wo, "f32fast", k, shape, ext)[1]), k
    with make_batch(wa, wo, dtype, shape, ext, variant=variant) as b:
        d = b.dispatch()
        assert d["dtype"] == dtype and ("float,double" if dtype == "f32" else "float,float") in d["kernel"], d
        for steps in model.STEP_COUNTS:
            for k in range(NM):
                b.upload_phi(k, inputs(wo, k, shape, ext)[2])
            b.evolve(steps)
            for k in range(NM):
                equal(b.download_phi(k), reference(wo, dtype, k, shape, ext)[steps], ext, f"member {k} after {steps} steps ({d['kernel']})")
        fused, single = b.passes()
        if variant == 1 and ext <= 2:
            assert d["steps_per_pass"] == (3 if ext == 1 else 2) and fused > 0, (d, fused, single)
        if variant == 0 or ext == 3:
            assert d["steps_per_pass"] == 1 and fused == 0, (d, fused, single)


# ---- 2. against single contexts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", model.SHAPES, ids=sid)
@pytest.mark.parametrize("ext", [1, 2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_members_equal_single_contexts(wa, wo, dtype, ext, shape):
    """12 steps: phi equal; the four observables doubles equal with ==; Batch.norm2() equal to Context.norm2() with =="""
    with make_batch(wa, wo, dtype, shape, ext) as b:
        b.evolve(12)
        obs, n2 = b.observables(), b.norm2()
        for k in range(NM):
            with make_context(wa, wo, dtype, k, shape, ext) as ctx:
                ctx.evolve(0, 12)
                equal(b.download_phi(k), ctx.download_phi(), ext, f"member {k}")
                want, want_n2 = ctx.observables(), ctx.norm2()
            print(dtype, ext, shape, "member", k, obs[k], want, n2[k], want_n2)
            for key in ("energy", "norm2", "v_infinity", "r2"):
                assert obs[k][key] == want[key], (k, key, obs[k][key], want[key])
            assert n2[k] == want_n2, (k, n2[k], want_n2)


@pytest.mark.parametrize("shape,ext", [((300, 5, 4), 1), ((521, 3, 2), 2)])
@pytest.mark.parametrize("dtype", ["f64"] + DTYPES)
def test_sums_on_rows_wider_than_a_tile(wa, wo, dtype, shape, ext):
    """nx beyond the observables' tile width (128 cells on doubles, 256 on floats) and beyond one 1 KiB row segment of the row
    walk: several x tiles per row and the workgroup swizzle over them.  Observables == a context's on every dtype; norm2() ==
    on float storage, rel 1e-12 on fp64 (the batch's own partition there)."""
    with make_batch(wa, wo, dtype, shape, ext) as b:
        b.evolve(3)
        obs, n2 = b.observables(), b.norm2()
        for k in range(NM):
            with make_context(wa, wo, dtype, k, shape, ext) as ctx:
                ctx.evolve(0, 3)
                equal(b.download_phi(k), ctx.download_phi(), ext, f"member {k}")
                want, want_n2 = ctx.observables(), ctx.norm2()
            print(dtype, shape, "member", k, obs[k], want, n2[k], want_n2)
            for key in ("energy", "norm2", "v_infinity", "r2"):
                assert obs[k][key] == want[key], (k, key, obs[k][key], want[key])
            if dtype == "f64":
                assert n2[k] == pytest.approx(want_n2, rel=model.REL_SUM, abs=0.0), k
            else:
                assert n2[k] == want_n2, (k, n2[k], want_n2)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_unplanned_division_is_honoured(wa, wo, dtype, variant):
    """WAFER_FLAG_UNPLANNED_DIV on every member: the planned divisions (fp64 and fp32) are off, the bits stay the reference's
    (the plan is the IEEE quotient) and a context's with the same flag"""
    shape, ext = (65, 33, 20), 1
    with make_batch(wa, wo, dtype, shape, ext, variant=variant, unplanned_div=True) as b:
        b.evolve(7)
        for k in range(NM):
            got = b.download_phi(k)
            equal(got, reference(wo, dtype, k, shape, ext)[7], ext, f"member {k}")
            with make_context(wa, wo, dtype, k, shape, ext, unplanned_div=True) as ctx:
                ctx.evolve(0, 7)
                equal(got, ctx.download_phi(), ext, f"member {k} against its context")


# ---- 3. one step per launch against fused passes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", model.VARIANT_SHAPES, ids=sid)
@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_passes_equal_single_steps(wa, wo, dtype, ext, shape):
    with make_batch(wa, wo, dtype, shape, ext, variant=0) as b0, make_batch(wa, wo, dtype, shape, ext, variant=1) as b1:
        assert b0.steps_per_launch() == 1 and b1.steps_per_launch() == (3 if ext == 1 else 2)
        for steps in model.VARIANT_STEPS:
            for b in (b0, b1):
                for k in range(NM):
                    b.upload_phi(k, inputs(wo, k, shape, ext)[2])
                b.evolve(steps)
            for k in range(NM):
                equal(b1.download_phi(k), b0.download_phi(k), ext, f"member {k} after {steps} steps")
        assert b1.passes()[0] > 0 and b0.passes()[0] == 0


# ---- 4. round trips -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ext", [((65, 33, 20), 1), ((3, 2, 5), 2), ((17, 17, 17), 3)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_uploads_and_states_round_to_float(wa, wo, dtype, shape, ext):
    """upload_phi / download_phi, load_state / download_state, push_state / clone_state_to_phi: what comes back is r32 of what
    went in (values over 60 binades, so the rounding is not the identity), per member, and the other members' are untouched"""
    rng = np.random.default_rng(11)
    with make_batch(wa, wo, dtype, shape, ext, phi=False) as b:
        pshape = b.members[0].padded_shape
        xs = [np.ascontiguousarray(rng.standard_normal(pshape) * 2.0 ** rng.integers(-30, 30, pshape)) for _ in range(2 * NM)]
        assert not np.array_equal(xs[0], ref.r32(xs[0]))
        for k in range(NM):
            b.upload_phi(k, xs[k])
            b.load_state(k, 0, xs[NM + k])
        for k in range(NM):
            equal(b.download_phi(k), ref.r32(xs[k]), ext, f"phi {k}")
            equal(b.download_state(k, 0), ref.r32(xs[NM + k]), ext, f"state {k}")
        b.push_state()                      # phi -> slot 1
        assert b.num_states() == [2] * NM
        for k in range(NM):
            equal(b.download_state(k, 1), ref.r32(xs[k]), ext, f"pushed {k}")
        b.clone_state_to_phi(0, active=[1, 0, 1])
        for k in range(NM):
            equal(b.download_phi(k), ref.r32(xs[NM + k] if k != 1 else xs[k]), ext, f"cloned {k}")


# ---- 5. normalise and norm2 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ext", [((65, 33, 20), 1), ((17, 17, 17), 2), ((3, 2, 5), 3), ((1, 1, 1), 1)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_normalise_and_norm2(wa, wo, dtype, shape, ext):
    """normalise(n2) with host-given norms: r32(x / sqrt(n2)) per cell; norm2(): the fp64 sum over the float values, rel 1e-12
    against numpy (another order of summation), and the double a context returns for the same values"""
    with make_batch(wa, wo, dtype, shape, ext) as b:
        starts = [inputs(wo, k, shape, ext)[2] for k in range(NM)]
        got_n2 = b.norm2()
        for k in range(NM):
            assert got_n2[k] == pytest.approx(float(np.sum(starts[k] * starts[k])), rel=model.REL_SUM, abs=0.0), k
            with make_context(wa, wo, dtype, k, shape, ext) as ctx:
                assert got_n2[k] == ctx.norm2(), k
        n2 = [(1.75 + k) * float(np.sum(x * x)) for k, x in enumerate(starts)]
        b.normalise(n2, active=[1, 1, 0])
        for k in range(NM):
            want = ref.r32(starts[k] / np.sqrt(n2[k])) if k < 2 else starts[k]
            equal(b.download_phi(k), want, ext, f"member {k}")


# ---- 6. independence --------------------------------------------------------------------------------------------------------------------
def _run(b, wnum, steps=5):
    if wnum:
        b.evolve(steps, wnum=wnum)
    else:
        b.set_step_variant(1)
        b.evolve(steps)


def _load_stores(b, wo, order, shape, ext, wnum):
    for slot, k in enumerate(order):
        for i, l in enumerate(model.stored_states(inputs(wo, k, shape, ext)[0], k, wnum)):
            b.load_state(slot, i, l)


@pytest.mark.parametrize("wnum", [0, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_member_bits_do_not_depend_on_the_batch(wa, wo, dtype, wnum):
    """member 1's bits at (B, slot) = (1, 0), (6, 4), (40, 37); under an active mask the active members equal the all-active
    run and the frozen ones are untouched"""
    shape, ext, k = (65, 33, 20), 1, 1
    runs = []
    for B, slot in ((1, 0), (6, 4), (40, 37)):
        order = [(s + 1 + k) % NM if s != slot else k for s in range(B)]   # the others differ from slot to slot
        with make_batch(wa, wo, dtype, shape, ext, order=order) as b:
            _load_stores(b, wo, order, shape, ext, wnum)
            _run(b, wnum)
            runs.append((b.download_phi(slot), b.norm2()[slot]))
    for got, n2 in runs[1:]:
        equal(got, runs[0][0], ext, "member 1 in another batch")
        assert n2 == runs[0][1]
    order = [0, 1, 2, 1, 0]
    with make_batch(wa, wo, dtype, shape, ext, order=order) as b:
        _load_stores(b, wo, order, shape, ext, wnum)
        _run(b, wnum)
        full = [b.download_phi(s) for s in range(len(order))]
    equal(full[1], runs[0][0], ext, "member 1 among five")
    for mask in ([1, 0, 0, 1, 0], [0, 1, 1, 0, 1]):
        with make_batch(wa, wo, dtype, shape, ext, order=order) as b:
            _load_stores(b, wo, order, shape, ext, wnum)
            if wnum:
                b.evolve(5, active=mask, wnum=wnum)
            else:
                b.set_step_variant(1)
                b.evolve(5, active=mask)
            for s, kk in enumerate(order):
                equal(b.download_phi(s), full[s] if mask[s] else inputs(wo, kk, shape, ext)[2], ext, f"slot {s} under {mask}")


# ---- 7. solve ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_solve_equals_context_solve(wa, wo, dtype):
    """(17, 17, 17) Harmonic, three dt: rows and finals of Batch.solve equal Context.solve_state(0, ...) of that dtype field by
    field, the wavefunctions too; max_steps is set so that the member with the smallest dt runs out of steps and the others
    converge"""
    shape, tol, su = (17, 17, 17), 1e-5, 20
    dts = [0.002, 0.008, 0.012]
    pars = [wa.Params(*shape, dn=0.2, dt=dt, mass=1.0, dtype=dtype) for dt in dts]
    cfg0 = wo.Config(*shape, ext=1, potential="Harmonic", dn=0.2, dt=dts[0], mass=1.0)
    phi0 = wo.initial_condition(cfg0, "Gaussian")

    def context_solve(par, max_steps):
        with wa.Context(par) as ctx:
            ctx.set_potential("Harmonic")
            ctx.upload_phi(phi0)
            rows, final, converged = ctx.solve_state(0, tol, su, max_steps)
            return rows, final, converged, ctx.download_phi()

    free = [context_solve(p, 4000) for p in pars[1:]]
    assert all(r[2] for r in free), [r[0][-1] for r in free]
    max_steps = max(r[0][-1]["step"] for r in free)
    refs = [context_solve(p, max_steps) for p in pars]
    assert [r[2] for r in refs] == [False, True, True], [(r[2], r[0][-1]["step"]) for r in refs]
    with wa.Batch(pars) as b:
        for k in range(len(pars)):
            b.set_potential(k, "Harmonic")
            b.upload_phi(k, phi0)
        got = b.solve(tol, su, max_steps)
        for k, (rows, final, converged, status) in enumerate(got):
            rrows, rfinal, rconv, rphi = refs[k]
            print(dtype, "member", k, "rows", len(rows), "final", final, "status", status)
            assert rows == rrows, k
            assert final == rfinal, k
            assert converged == rconv, k
            assert status == (wa.engine.WAFER_OK if rconv else wa.engine.WAFER_ERR_MAX_STEP), k
            equal(b.download_phi(k), rphi, 1, f"member {k}")


# ---- 8. excited states against the chain model ------------------------------------------------------------------------------------------
EXCITED_STEPS = (1, 4)


@functools.lru_cache(maxsize=None)
def chain(wo, k, shape, ext, wnum):
    """member k's stored states and, per operation ("orthogonalise", 1, 4: steps), the chain model on float storage with exact
    scalars and with every scalar moved by +-1e-12 relative"""
    cfg, v, phi, _ = inputs(wo, k, shape, ext)
    lowers = model.stored_states(cfg, k, wnum)
    out = {"orthogonalise": (model.orthogonalise(phi, lowers, np.float32),
                             model.orthogonalise(phi, lowers, np.float32, model.Perturbed(k)))}
    for steps in EXCITED_STEPS:
        out[steps] = (model.excited_steps(cfg, v, phi, lowers, steps, np.float32),
                      model.excited_steps(cfg, v, phi, lowers, steps, np.float32, model.Perturbed(k)))
    return lowers, out


def bar(cfg, exact, perturbed):
    """(u, D_ref, work cells in which the two model runs differ)"""
    u = model.spacing_u(exact)
    return u, float(np.max(np.abs(exact - perturbed))) / u, int(np.count_nonzero(model.work(cfg, exact) != model.work(cfg, perturbed)))


def _within(got, cfg, exact, perturbed, what):
    u, d_ref, flips = bar(cfg, exact, perturbed)
    ncell = cfg.nx * cfg.ny * cfg.nz
    err = float(np.max(np.abs(got - exact))) / u
    differ = int(np.count_nonzero(model.work(cfg, got) != model.work(cfg, exact)))
    print(what, "D_ref", d_ref, "model flips", flips, "u", u, "gpu max err / u", err, "gpu cells differing", differ, "of", ncell)
    assert np.array_equal(got, ref.r32(got)), what
    assert err <= max(1.0, 4.0 * d_ref), (what, err, d_ref)
    assert differ <= 0.01 * ncell, (what, differ, ncell)


@pytest.mark.parametrize("shape", model.EXCITED_SHAPES, ids=sid)
@pytest.mark.parametrize("ext", [1, 2, 3])
@pytest.mark.parametrize("wnum", [1, 2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_excited_states_follow_the_chain_model(wa, wo, dtype, wnum, ext, shape):
    """orthogonalise(wnum) alone, then evolve(steps, wnum) for 1 and 4 steps, every member, against the chain model with float
    storage.  The batch's sums are partitioned differently from numpy's, so a scalar can differ in its last bits and flip a
    float rounding in a rare cell; the bar comes from the model alone: D_ref = the largest cell difference, in units of u (the
    float spacing at max |phi|), between the model with exact scalars and the model with every scalar moved by +-1e-12
    relative (the project's bar for sums).  The GPU result lies within max(1, 4 D_ref) u of the exact-scalar model (4: the
    perturbation's sign pattern is one sample), and at most 1 % of the work cells differ from it at all.

    Observed on the CPU, the model against its perturbed self over the 18 cases x 3 members x {orthogonalise, 1 step, 4 steps}
    of this table: D_ref <= 1.0 at (33, 20, 11) and <= 0.75 at (65, 33, 20), 0 in most cases; cells that differ at all: at most
    42 of 7 260 (0.58 %) at (33, 20, 11) and 129 of 42 900 (0.30 %) at (65, 33, 20), both after 4 steps (a flipped cell moves
    its neighbours' next step by a fraction of an ulp, so flips breed).  The batch's scalars differ from numpy's by fp64
    rounding (~1e-16), four orders below the perturbation."""
    with make_batch(wa, wo, dtype, shape, ext) as b:
        models = [chain(wo, k, shape, ext, wnum) for k in range(NM)]
        for k, (lowers, _) in enumerate(models):
            for i, l in enumerate(lowers):
                b.load_state(k, i, l)
        b.orthogonalise(wnum)
        for k, (lowers, out) in enumerate(models):
            _within(b.download_phi(k), inputs(wo, k, shape, ext)[0], *out["orthogonalise"], f"orthogonalise member {k}")
            for i, l in enumerate(lowers):   # the store is read, never written
                assert np.array_equal(b.download_state(k, i), l), (k, i)
        for steps in EXCITED_STEPS:
            for k in range(NM):
                b.upload_phi(k, inputs(wo, k, shape, ext)[2])
            b.evolve(steps, wnum=wnum)
            for k, (lowers, out) in enumerate(models):
                _within(b.download_phi(k), inputs(wo, k, shape, ext)[0], *out[steps], f"{steps} steps member {k}")


# ---- 9. f32fast excited steps are f32's ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_f32fast_excited_steps_equal_f32(wa, wo, ext):
    """excited steps compute in fp64 on both float dtypes"""
    shape, out = (65, 33, 20), {}
    for dtype in DTYPES:
        with make_batch(wa, wo, dtype, shape, ext) as b:
            _load_stores(b, wo, range(NM), shape, ext, 1)
            b.evolve(6, wnum=1)
            out[dtype] = [b.download_phi(k) for k in range(NM)]
    for k in range(NM):
        equal(out["f32fast"][k], out["f32"][k], ext, f"member {k}")


# ---- 10. a sweep over states ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_solve_state_sweep(wa, wo, dtype):
    """solve_state(0) then solve_state(1) on three members: statuses OK, two states in every store, and the rows of a member
    do not depend on the batch around it (B = 1 against B = 5)"""
    shape, tol, su = (17, 17, 17), 1e-4, 20
    dts = [0.006, 0.008, 0.012]
    cfg0 = wo.Config(*shape, ext=1, potential="Harmonic", dn=0.2, dt=dts[0], mass=1.0)
    starts = [wo.initial_condition(cfg0, "Gaussian"), wo.initial_condition(cfg0, "Boolean")]

    def sweep(which):
        pars = [wa.Params(*shape, dn=0.2, dt=dts[k], mass=1.0, dtype=dtype, max_states=2) for k in which]
        with wa.Batch(pars) as b:
            out = []
            for wnum in (0, 1):
                for s in range(len(pars)):
                    if wnum == 0:
                        b.set_potential(s, "Harmonic")
                    b.upload_phi(s, starts[wnum])
                out.append(b.solve_state(wnum, tol, su, 3000))
            return out, b.num_states(), [[b.download_state(s, i) for i in range(2)] for s in range(len(pars))]

    which = [0, 1, 2, 1, 0]
    full, counts, states = sweep(which)
    assert counts == [2] * 5
    for wnum in (0, 1):
        for s in range(5):
            rows, final, converged, status = full[wnum][s]
            assert converged and status == wa.engine.WAFER_OK and final["state"] == wnum, (wnum, s, status, rows[-1])
    for k in range(3):
        alone, counts1, states1 = sweep([k])
        assert counts1 == [2]
        for wnum in (0, 1):
            assert alone[wnum][0][0] == full[wnum][k][0], (k, wnum)
            assert alone[wnum][0][1] == full[wnum][k][1], (k, wnum)
        for i in range(2):
            assert np.array_equal(states1[0][i], states[k][i]), (k, i)
    for i in range(2):   # the same member at two slots of one batch
        assert np.array_equal(states[3][i], states[1][i]) and np.array_equal(states[4][i], states[0][i])
