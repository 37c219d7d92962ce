"""The fused K-step pass of batched ground-state evolves (wafer_k_batch_stepk, Batch.set_step_variant(1)) on the MI355X: every
member's bits are those of the one-step kernel -- the single context's and the oracle's -- whatever the pass sequence, the
active set, the batch size and the calls in between; passes() shows that the kernel meant is the one that ran."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.gpu_common import make_pair, random_phi, ulp_diff  # noqa: E402
from tests.test_gpu_batch import MEMBERS, setup_members, context_of  # noqa: E402

SHAPES = [(50, 50, 50), (64, 64, 64), (37, 50, 23), (130, 70, 40), (64, 64, 2)]   # (130, 70, 40): tile seams in x and y;
FUSED_EXTS = [1, 2]                                                                # (64, 64, 2): thinner than K R
STEP_COUNTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 1000)


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


def predicted(b, steps):
    """(fused passes, one-step launches) of a ground-state call: the sequence tests/test_batch_plan.py checks on the CPU"""
    d = b.dispatch()
    K, have2 = b.steps_per_launch(), d["remainder"] == "stepk2+step"
    left, fused, single = max(steps, 1), 0, 0
    while K > 1 and left >= K:
        fused, left = fused + 1, left - K
    while have2 and left >= 2:
        fused, left = fused + 1, left - 2
    return fused, single + left


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def frame_is_zero(got, e):
    return not (np.any(got[:e]) or np.any(got[-e:]) or np.any(got[:, :e]) or np.any(got[:, -e:]) or np.any(got[:, :, :e])
                or np.any(got[:, :, -e:]))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ext", FUSED_EXTS)
def test_fused_evolve_matches_oracle(wa, wo, shape, ext):
    b, ms = setup_members(wa, wo, shape, ext, MEMBERS)
    with b:
        b.set_step_variant(1)
        assert b.steps_per_launch() == (3 if ext == 1 else 2)
        abs_ = [wo.ab(m[0], m[2]) for m in ms]
        want_f, want_s = 0, 0
        for steps in STEP_COUNTS:
            f, s = predicted(b, steps)
            want_f, want_s = want_f + f, want_s + s
            b.evolve(steps)
            assert b.passes() == (want_f, want_s), (shape, ext, steps)
            for k, m in enumerate(ms):
                cfg, phi = m[0], m[4]
                wo.evolve(cfg, 0, abs_[k][0], abs_[k][1], phi, [], steps)
                got = b.download_phi(k)
                d = ulp_diff(got, phi)
                print(shape, ext, steps, "member", k, "ulp", d)
                assert d == 0, (shape, ext, steps, k)
                assert frame_is_zero(got, cfg.ext), (shape, ext, steps, k)
        assert want_f > 0


@pytest.mark.parametrize("shape", [(50, 50, 50), (130, 70, 40), (64, 64, 2)])
@pytest.mark.parametrize("ext", FUSED_EXTS)
def test_fused_equals_one_step(wa, wo, shape, ext):
    """from the same start, variants 0 and 1 give the same int64 views"""
    res = {}
    for variant in (0, 1):
        b, ms = setup_members(wa, wo, shape, ext, MEMBERS)
        with b:
            b.set_step_variant(variant)
            out = []
            for steps in (1, 2, 3, 5, 8, 64):
                b.evolve(steps)
                out.append([bits(b.download_phi(k)) for k in range(len(ms))])
            res[variant] = out
            f, s = b.passes()
            if variant == 0:
                assert f == 0 and s == 83
            else:
                assert f > 0
    for a, c in zip(res[0], res[1]):
        for k in range(len(a)):
            assert np.array_equal(a[k], c[k]), (shape, ext, k)


@pytest.mark.parametrize("ext", FUSED_EXTS)
def test_fused_active_mask(wa, wo, ext):
    shape = (40, 36, 44)
    b, ms = setup_members(wa, wo, shape, ext, MEMBERS)
    ref, _ = setup_members(wa, wo, shape, ext, MEMBERS)
    with b, ref:
        b.set_step_variant(1)
        ref.set_step_variant(1)
        before = [bits(b.download_phi(k)) for k in range(len(ms))]
        mask = [1, 0, 1, 0, 1]
        b.evolve(7, active=mask)
        ref.evolve(7)
        assert b.passes()[0] > 0
        for k in range(len(ms)):
            got = bits(b.download_phi(k))
            if mask[k]:   # an active member's bits are those of an all-active run
                assert np.array_equal(got, bits(ref.download_phi(k))), k
            else:         # a frozen member is not touched
                assert np.array_equal(got, before[k]), k
        # a member left out of one call continues from where it stood, whatever its `cur`
        b.evolve(4, active=[0, 1, 0, 1, 0])
        b.evolve(3, active=[0, 1, 0, 1, 0])
        for k in (1, 3):
            assert np.array_equal(bits(b.download_phi(k)), bits(ref.download_phi(k))), k


def test_fused_bits_do_not_depend_on_batch_size_or_index(wa, wo):
    shape = (32, 32, 32)
    cfg, par = make_pair(shape, potential="Coulomb", dn=0.2, dt=0.0031, mass=1.3)
    phi = random_phi(cfg, seed=11)
    got = []
    for B, slot in ((1, 0), (6, 4), (64, 37)):
        pars = [wa.Params(*shape, dn=0.2, dt=0.002 + 0.0001 * k, mass=1.0 + 0.01 * k) for k in range(B)]
        pars[slot] = par
        with wa.Batch(pars) as b:
            b.set_step_variant(1)
            for k in range(B):
                b.set_potential(k, "Coulomb" if k == slot else "Harmonic")
                b.upload_phi(k, phi if k == slot else random_phi(cfg, seed=100 + k))
            b.evolve(7)
            assert b.passes() == (2, 1)   # 7 steps at K = 3: two passes of three, then one single step
            got.append(bits(b.download_phi(slot)))
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    a_, b_ = wo.ab(cfg, wo.potential_generate(cfg))
    wo.evolve(cfg, 0, a_, b_, phi, [], 7)
    assert np.array_equal(got[0], bits(phi))


@pytest.mark.parametrize("shape,ext", [((50, 50, 50), 1), ((64, 64, 64), 2)])
def test_fused_mixed_calls_match_contexts(wa, wo, shape, ext):
    """evolve(3), observables, normalise, evolve(4), push_state, evolve(2, wnum=1): the `cur` bookkeeping across odd and even
    launch counts (K = 3: 1, then 1 + 1 launches; K = 2: 1 + 1, then 2), against a Context per member"""
    b, ms = setup_members(wa, wo, shape, ext, MEMBERS)
    with b:
        b.set_step_variant(1)
        b.evolve(3)
        obs = b.observables()
        b.normalise([o["norm2"] for o in obs])
        b.evolve(4)
        assert b.passes()[0] > 0
        ground = [b.download_phi(k) for k in range(len(ms))]
        obs2 = b.observables()
        b.push_state()
        fresh = [random_phi(m[0], seed=70 + k) for k, m in enumerate(ms)]
        for k in range(len(ms)):
            b.upload_phi(k, fresh[k])
        b.evolve(2, wnum=1)
        for k, m in enumerate(ms):
            with context_of(wa, m, m[4]) as ctx:
                ctx.evolve(0, 3)
                o = ctx.observables()
                assert o == obs[k], (k, o, obs[k])
                ctx.normalise(o["norm2"])
                ctx.evolve(0, 4)
                assert np.array_equal(bits(ctx.download_phi()), bits(ground[k])), k
                assert ctx.observables() == obs2[k], k
                ctx.push_state()
                assert np.array_equal(bits(b.download_state(k, 0)), bits(ground[k])), k
                ctx.upload_phi(fresh[k])
                ctx.evolve(1, 2)
                err = float(np.max(np.abs(b.download_phi(k) - ctx.download_phi())))
                print("member", k, "excited max|dphi|", err)
                assert err <= 1e-13, (k, err)


def test_fused_solve_equals_one_step_solve(wa, wo):
    shape, tol, su = (32, 32, 32), 1e-7, 50          # 50 steps: 16 passes of 3 and one of 2 -- an odd number of launches
    dts = [0.0015, 0.004, 0.006, 0.008, 0.012]
    cfg0, _ = make_pair(shape, dn=0.2, dt=dts[0])
    phi0 = wo.initial_condition(cfg0, "Gaussian")
    res = {}
    for variant in (0, 1):
        pars = [wa.Params(*shape, dn=0.2, dt=dt, mass=1.0) for dt in dts]
        with wa.Batch(pars) as b:
            b.set_step_variant(variant)
            for k in range(len(pars)):
                b.set_potential(k, "Harmonic")
                b.upload_phi(k, phi0)
            got = b.solve(tol, su, 1500)
            res[variant] = (got, [bits(b.download_phi(k)) for k in range(len(pars))], b.passes())
    assert res[0][2][0] == 0 and res[1][2][0] > 0
    assert res[0][0] == res[1][0]                      # rows, finals, converged, statuses: exact equality
    for a, c in zip(res[0][1], res[1][1]):
        assert np.array_equal(a, c)


@pytest.mark.parametrize("ext", [1, 2, 3])
def test_dispatch_reports_what_runs(wa, wo, ext):
    b, ms = setup_members(wa, wo, (20, 18, 16), ext, MEMBERS[:2])
    with b:
        assert b.kernel_name() == "wafer_k_batch_step"
        for variant in (0, 1, -1):
            b.set_step_variant(variant)
            d = b.dispatch()
            K = b.steps_per_launch()
            assert d["steps_per_pass"] == K and d["variant"] == variant
            assert d["stencil"] == ["ThreePoint", "FivePoint", "SevenPoint"][ext - 1]
            if variant == 0 or ext == 3:
                assert K == 1
            if variant == 1 and ext < 3:
                assert K == (3, 2)[ext - 1]
            if K > 1:
                assert d["kernel"] == "wafer_k_batch_stepk<%d,%d>" % (ext, K) and d["lds_bytes"] > 0
                assert d["tile"] == "64x12" and d["remainder"] in ("step", "stepk2+step")
            else:
                assert d["kernel"] == "wafer_k_batch_step<%d>" % ext and d["lds_bytes"] == 0 and d["remainder"] == "none"
            f0, s0 = b.passes()
            b.evolve(5 * K + 1)
            assert b.passes() == ((f0 + 5, s0 + 1) if K > 1 else (f0, s0 + 6)), (variant, d)
        with pytest.raises(wa.WaferError):
            b.set_step_variant(2)
