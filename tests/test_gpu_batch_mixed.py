"""Mixed-shape batches (wafer_amd.Batch(members, mixed_shapes=True)) on the MI355X: members of different nx, ny, nz in one batch,
one launch per step or fused pass for all of them.  Every member must compute bit for bit what a Context of its own Params (and, on
fp64, the oracle) computes: phi after evolve under both step variants and on the three dtypes, the observables, norm2, normalise
and solve -- whatever the batch size, its index, the other members' shapes or the active set."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.gpu_common import make_pair, random_phi, ulp_diff  # noqa: E402

REL_SUM = 1e-12

# The smallest set that still hits every layout difference: the reference's shipped size; BASELINE config #1's size; ragged in every
# axis; a second 128-element pitch tile on doubles with fewer rows than one 12-row fused tile and thinner than a fused chunk; one
# workgroup beside large members; one column past a 64-wide tile with odd rows and nz < 2R+1 for R = 3.
S = [(50, 50, 50), (64, 64, 64), (37, 50, 23), (130, 6, 5), (8, 8, 8), (65, 13, 3)]
SPECS = [
    dict(potential="Harmonic", dn=0.2, dt=0.004, mass=1.0),
    dict(potential="Coulomb", dn=0.25, dt=0.01, mass=0.5),
    dict(potential="host_potsub", dn=0.2, dt=0.003, mass=1.5),   # host V with a pot_sub array
    dict(potential="Harmonic", dn=0.3, dt=0.02, mass=1.0),
    dict(potential="Coulomb", dn=0.2, dt=0.005, mass=2.0),
    dict(potential="host_potsub", dn=0.25, dt=0.006, mass=1.0),
]
CALLS = (1, 2, 3, 7)   # cumulative step counts 1, 3, 6, 13: remainders of the fused passes occur


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


def host_v(cfg):
    """a smooth, non-builtin potential on the padded grid"""
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in cfg.padded_shape], indexing="ij")
    c = [(n - 1) / 2.0 for n in cfg.padded_shape]
    return 0.05 * ((x - c[0]) ** 2 + 0.5 * (y - c[1]) ** 2) * cfg.dn + 0.3 * np.cos(0.4 * z)


@functools.lru_cache(maxsize=None)
def member(wo, k, ext, dtype="f64"):
    """member k of S: (cfg, par, v, potsub, phi) -- computed once, shared, never written to"""
    s = SPECS[k]
    host = s["potential"] == "host_potsub"
    cfg, par = make_pair(S[k], ext=ext, potential="Harmonic" if host else s["potential"], dn=s["dn"], dt=s["dt"], mass=s["mass"], dtype=dtype)
    if host:
        v, potsub = host_v(cfg), (2, 0.0, np.random.default_rng(7 + k).standard_normal(cfg.work_shape))
    else:
        v, potsub = wo.potential_generate(cfg), wo.potential_sub(cfg)
    phi = random_phi(cfg, seed=k + 1)
    for a in (v, phi, potsub[2]):
        if a is not None:
            a.setflags(write=False)
    return cfg, par, v, potsub, phi


def set_up(obj, wo, k, ext, dtype="f64", slot=None, host_arrays=False):
    """member k's potential and start into a Batch (slot given) or a Context, by the same calls"""
    cfg, par, v, potsub, phi = member(wo, k, ext, dtype)
    at = () if slot is None else (slot,)
    if host_arrays or SPECS[k]["potential"] == "host_potsub":
        obj.set_potential_host(*at, np.array(v), potsub[0], potsub[1], None if potsub[2] is None else np.array(potsub[2]))
    else:
        obj.set_potential(*at, SPECS[k]["potential"])
    obj.upload_phi(*at, np.array(phi))


def make_batch(wa, wo, ext, dtype="f64", order=None, variant=None, mixed=True, host_arrays=False):
    order = list(range(len(S))) if order is None else list(order)
    b = wa.Batch([member(wo, k, ext, dtype)[1] for k in order], mixed_shapes=mixed)
    if variant is not None:
        b.set_step_variant(variant)
    for slot, k in enumerate(order):
        set_up(b, wo, k, ext, dtype, slot=slot, host_arrays=host_arrays)
    return b


def make_context(wa, wo, k, ext, dtype="f64", host_arrays=False):
    ctx = wa.Context(member(wo, k, ext, dtype)[1])
    set_up(ctx, wo, k, ext, dtype, host_arrays=host_arrays)
    return ctx


@functools.lru_cache(maxsize=None)
def oracle_after(wo, k, ext, steps):
    """member k's fp64 phi after `steps` steps from its start (the oracle; shared by the tests)"""
    cfg, par, v, potsub, phi = member(wo, k, ext)
    a_, b_ = wo.ab(cfg, v)
    out = np.array(phi)
    wo.evolve(cfg, 0, a_, b_, out, [], steps)
    out.setflags(write=False)
    return out


def pass_sequence(steps, K, have2):
    """wafer_batch_plan.h's rule: passes of K while at least K remain, one two-step pass if there is one, then single steps"""
    left, seq = max(steps, 1), []
    while K > 1 and left >= K:
        seq.append(K)
        left -= K
    while have2 and left >= 2:
        seq.append(2)
        left -= 2
    return seq + [1] * left


def expected_passes(ext, variant, calls):
    K = {1: 3, 2: 2, 3: 1}[ext] if variant == 1 else 1
    seq = [k for n in calls for k in pass_sequence(n, K, have2=(K == 3))]
    return sum(1 for k in seq if k > 1), sum(1 for k in seq if k == 1)


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---- 1. fp64 evolve against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_mixed_evolve_matches_oracle(wa, wo, ext, variant):
    with make_batch(wa, wo, ext, variant=variant) as b:
        assert b.num_shapes() == len(S)
        total = 0
        for n in CALLS:
            b.evolve(n)
            total += n
            for k in range(len(S)):
                got = b.download_phi(k)
                assert ulp_diff(got, oracle_after(wo, k, ext, total)) == 0, (ext, variant, total, k, S[k])
                e = ext   # the Dirichlet frame stays zero
                assert not np.any(got[:e]) and not np.any(got[-e:]) and not np.any(got[:, :e]) and not np.any(got[:, :, -e:])
        # launches of ONE batch: every launch covers all six shapes
        assert b.passes() == expected_passes(ext, variant, CALLS), (b.passes(), b.dispatch())


# ---- 2. independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext,variant", [(1, 0), (1, 1), (2, 1), (3, 0)])
def test_member_bits_do_not_depend_on_the_batch(wa, wo, ext, variant):
    n = len(S)
    with make_batch(wa, wo, ext, variant=variant) as b:
        b.evolve(7)
        in_s = [b.download_phi(k) for k in range(n)]
    with make_batch(wa, wo, ext, variant=variant, order=range(n - 1, -1, -1)) as b:   # other index, other neighbours
        b.evolve(7)
        for slot in range(n):
            assert same_bits(b.download_phi(slot), in_s[n - 1 - slot]), ("reversed", n - 1 - slot)
    for k in range(n):   # alone, in a batch of one shape
        with make_batch(wa, wo, ext, variant=variant, order=[k], mixed=False) as b:
            b.evolve(7)
            assert same_bits(b.download_phi(0), in_s[k]), ("alone", k)
    with make_batch(wa, wo, ext, variant=variant) as b:   # in S with only it active; the frozen members bit for bit unchanged
        for k in range(n):
            for j in range(n):
                b.upload_phi(j, np.array(member(wo, j, ext)[4]))
            before = [b.download_phi(j) for j in range(n)]
            b.evolve(7, active=[int(j == k) for j in range(n)])
            for j in range(n):
                assert same_bits(b.download_phi(j), in_s[k] if j == k else before[j]), ("only", k, j)


@pytest.mark.parametrize("variant", [0, 1])
def test_member_left_out_of_a_call_continues_from_where_it_stood(wa, wo, variant):
    ext, n = 1, len(S)
    calls = [(2, [1, 0, 1, 0, 1, 0]), (3, [0, 1, 1, 0, 0, 1]), (2, [1, 1, 1, 1, 1, 1])]   # the members' buffers flip apart
    with make_batch(wa, wo, ext, variant=variant) as b:
        done = [0] * n
        for steps, mask in calls:
            before = [b.download_phi(k) for k in range(n)]
            b.evolve(steps, active=mask)
            for k in range(n):
                got = b.download_phi(k)
                if not mask[k]:
                    assert same_bits(got, before[k]), (steps, k)
                    continue
                done[k] += steps
                assert ulp_diff(got, oracle_after(wo, k, ext, done[k])) == 0, (steps, k, done[k])


# ---- 3. float dtypes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("dtype", ["f32", "f32fast"])
def test_mixed_float_members_equal_contexts(wa, wo, dtype, ext, variant):
    with make_batch(wa, wo, ext, dtype=dtype, variant=variant) as b:
        d = b.dispatch()
        assert d["dtype"] == dtype and ("float,double" if dtype == "f32" else "float,float") in d["kernel"], d
        b.evolve(7)
        for k in range(len(S)):
            with make_context(wa, wo, k, ext, dtype) as ctx:
                ctx.evolve(0, 7)
                assert same_bits(b.download_phi(k), ctx.download_phi()), (dtype, ext, variant, k, S[k])


# ---- 4. observables, norm2, normalise ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [1, 2, 3])
@pytest.mark.parametrize("dtype", ["f64", "f32", "f32fast"])
def test_mixed_observables_norm2_and_normalise(wa, wo, dtype, ext):
    """V and pot_sub go up as host arrays here, so that on float storage the oracle can be given what the device holds: the
    arrays rounded to float (uploads round to nearest even)."""
    held = (lambda a: a) if dtype == "f64" else (lambda a: a.astype(np.float32).astype(np.float64))
    with make_batch(wa, wo, ext, dtype=dtype, host_arrays=True) as b:
        b.evolve(5)
        obs, n2 = b.observables(), b.norm2()
        phis = [b.download_phi(k) for k in range(len(S))]
        b.normalise([o["norm2"] for o in obs])
        for k in range(len(S)):
            cfg, par, v, potsub, _ = member(wo, k, ext, dtype)
            with make_context(wa, wo, k, ext, dtype, host_arrays=True) as ctx:
                ctx.upload_phi(phis[k])
                want, want_n2 = ctx.observables(), ctx.norm2()
                print(dtype, ext, S[k], obs[k], want, n2[k], want_n2)
                assert obs[k] == want, (k, obs[k], want)   # all four doubles: the context's partition and tree for this shape
                if dtype == "f64":
                    assert abs(n2[k] - want_n2) <= REL_SUM * want_n2, (k, n2[k], want_n2)
                else:
                    assert n2[k] == want_n2, (k, n2[k], want_n2)
                ctx.normalise(obs[k]["norm2"])
                assert same_bits(b.download_phi(k), ctx.download_phi()), ("normalise", k)
            sub = potsub if potsub[2] is None else (potsub[0], potsub[1], held(potsub[2]))
            ref = wo.observables(cfg, held(v), phis[k], sub)
            for q in ref:
                assert abs(obs[k][q] - ref[q]) <= REL_SUM * abs(ref[q]), (k, q, obs[k][q], ref[q])


# ---- 5. solve -------------------------------------------------------------------------------------------------------------------
def test_mixed_solve_matches_contexts(wa, wo):
    shapes = [(24, 24, 24), (16, 16, 16), (20, 24, 18), (32, 32, 32)]
    dts = [0.004, 0.008, 0.006, 0.0015]   # the last needs the most steps: it is the one that hits max_steps
    tol, su = 1e-6, 50
    pars = [wa.Params(*s, dn=0.2, dt=dt, mass=1.0) for s, dt in zip(shapes, dts)]
    phis = [wo.initial_condition(make_pair(s, dn=0.2, dt=dt)[0], "Gaussian") for s, dt in zip(shapes, dts)]

    def ref(k, max_steps):
        with wa.Context(pars[k]) as ctx:
            ctx.set_potential("Harmonic")
            ctx.upload_phi(phis[k])
            rows, final, converged = ctx.solve_state(0, tol, su, max_steps)
            return rows, final, converged, ctx.download_phi()
    last = [ref(k, None)[0][-1]["step"] for k in range(4)]
    max_steps = max(last[:3])
    assert last[3] > max_steps + su, last
    assert len(set(last)) > 2, last   # members finish at different blocks
    refs = [ref(k, max_steps) for k in range(4)]
    with wa.Batch(pars, mixed_shapes=True) as b:
        assert b.num_shapes() == 4
        for k in range(4):
            b.set_potential(k, "Harmonic")
            b.upload_phi(k, phis[k])
        got = b.solve(tol, su, max_steps)
        for k, (rows, final, converged, status) in enumerate(got):
            rrows, rfinal, rconv, rphi = refs[k]
            assert rows == rrows, k
            assert final == rfinal, k
            assert converged == rconv == (k != 3), k
            assert status == (wa.engine.WAFER_ERR_MAX_STEP if k == 3 else wa.engine.WAFER_OK), (k, status)
            assert same_bits(b.download_phi(k), rphi), k


# ---- 6. refusals, and the one-shape case ------------------------------------------------------------------------------------------
def test_state_store_calls_are_refused_on_several_shapes(wa, wo):
    ext = 1
    with make_batch(wa, wo, ext) as b:
        before = [b.download_phi(k) for k in range(len(S))]
        state = np.array(member(wo, 2, ext)[4])
        calls = {
            "wafer_batch_load_state": lambda: b.load_state(2, 0, state),
            "wafer_batch_download_state": lambda: b.download_state(2, 0),
            "wafer_batch_push_state": lambda: b.push_state(),
            "wafer_batch_clear_states": lambda: b.clear_states(),
            "wafer_batch_clone_state_to_phi": lambda: b.clone_state_to_phi(0),
            "wafer_batch_orthogonalise": lambda: b.orthogonalise(1),
            "wafer_batch_evolve_state": lambda: b.evolve(1, wnum=1),
            "wafer_batch_solve_state": lambda: b.solve_state(0, 1e-6, 50, 100),
            "wafer_batch_solve_state ": lambda: b.solve_state(1, 1e-6, 50, 100),
            "wafer_batch_set_gs_variant": lambda: b.set_gs_variant(1),
        }
        for name, call in calls.items():
            with pytest.raises(wa.WaferError) as e:
                call()
            assert e.value.code == -1, (name, str(e.value))
            assert "mixed-shape" in str(e.value) and name.strip() in str(e.value), (name, str(e.value))
        for k in range(len(S)):
            assert same_bits(b.download_phi(k), before[k]), k
        # what still works: evolve_state with wnum = 0 is evolve; the counts are zeros; the excited-state diagnostic answers
        assert b.num_states() == [0] * len(S)
        assert b.gs_dispatch(0)["form"] == "sequential"
        b.set_gs_variant(0)
        b.set_gs_variant(-1)
        assert b._L.wafer_batch_evolve_state(b._h, None, 0, 1) == 0
        for k in range(len(S)):
            assert ulp_diff(b.download_phi(k), oracle_after(wo, k, ext, 1)) == 0, k


def test_one_distinct_shape_is_a_plain_batch(wa, wo):
    shape = (32, 32, 32)
    pars = [wa.Params(*shape, dn=0.2, dt=0.002 + 0.0005 * k, mass=1.0 + 0.1 * k) for k in range(4)]
    phis = [random_phi(make_pair(shape)[0], seed=20 + k) for k in range(4)]
    out = []
    for mixed in (False, True):
        with wa.Batch(pars, mixed_shapes=mixed) as b:
            assert b.num_shapes() == 1
            for k in range(4):
                b.set_potential(k, "Harmonic")
                b.upload_phi(k, phis[k])
            b.evolve(3)
            b.push_state()
            for k in range(4):
                b.upload_phi(k, phis[(k + 1) % 4])
            b.evolve(5, wnum=1)
            out.append((b.dispatch(), b.kernel_name(), b.num_states(), [b.download_phi(k) for k in range(4)],
                        [b.download_state(k, 0) for k in range(4)]))
    plain, mixed = out
    assert mixed[0] == plain[0] and "shapes" not in mixed[0]
    assert mixed[1] == plain[1] == "wafer_k_batch_step"
    assert mixed[2] == plain[2] == [1] * 4
    for k in range(4):
        assert same_bits(mixed[3][k], plain[3][k]) and same_bits(mixed[4][k], plain[4][k]), k


# ---- 7. dispatch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_mixed_dispatch_names_what_it_launches(wa, wo, variant):
    ext = 1
    with make_batch(wa, wo, ext, variant=variant) as b, make_batch(wa, wo, ext, variant=variant, order=[0, 0], mixed=False) as u:
        d, du = b.dispatch(), u.dispatch()
        assert b.num_shapes() == 6 and d["shapes"] == "6" and "shapes" not in du
        assert d["kernel"] != du["kernel"] and "WaferBatchGeomTable" in d["kernel"], (d, du)
        assert d["kernel"].startswith("wafer_k_batch_stepk<1,3," if variant == 1 else "wafer_k_batch_step<1,"), d
        assert {k: v for k, v in d.items() if k not in ("kernel", "shapes")} == {k: v for k, v in du.items() if k != "kernel"}
        assert b.kernel_name() != u.kernel_name() and b.kernel_name().startswith("wafer_k_batch_step<1,"), b.kernel_name()
