"""Batched ensembles (wafer_amd.Batch) on the MI355X: every member must compute bit for bit what a single Context with
its Params computes -- phi after evolve (and so the oracle's), the observables, normalisation and solve."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.gpu_common import make_pair, random_phi, ulp_diff  # noqa: E402

REL_SUM = 1e-12


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


# potential: builtin name, "host" (uploaded V) or "host_potsub" (uploaded V and pot_sub array); ic: initial condition name or
# "random".  The oracle starts from the device's initial phi and, for uploads, the same V: the transcendental initial conditions
# and potentials (exp, sin) come from different libms (tests/test_gpu_parity.py), the step arithmetic does not.
MEMBERS = [
    dict(potential="Harmonic", dn=0.2, dt=0.004, mass=1.0, ic="Boolean"),
    dict(potential="Coulomb", dn=0.25, dt=0.01, mass=0.5, ic="Gaussian"),
    dict(potential="SimpleCornell", dn=0.2, dt=0.005, mass=2.0, ic="random", unplanned_div=True),
    dict(potential="host", dn=0.3, dt=0.02, mass=1.0, ic="Gaussian"),
    dict(potential="host_potsub", dn=0.2, dt=0.003, mass=1.5, ic="random"),   # host V with a pot_sub array
]


def setup_members(wa, wo, shape, ext, specs):
    """-> (batch, [(cfg, par, v, potsub, phi_host)]) with every member set up in the batch and in the oracle"""
    out, pars = [], []
    for k, s in enumerate(specs):
        host = s["potential"].startswith("host")
        pot = "Harmonic" if host else s["potential"]
        cfg, par = make_pair(shape, ext=ext, potential=pot, dn=s["dn"], dt=s["dt"], mass=s["mass"],
                             unplanned_div=s.get("unplanned_div", False))
        if s["potential"] == "host":
            v, potsub = host_v(cfg), (0, 0.0, None)
        elif s["potential"] == "host_potsub":
            v, potsub = host_v(cfg), (2, 0.0, np.random.default_rng(7).standard_normal(cfg.work_shape))
        else:
            v, potsub = wo.potential_generate(cfg), wo.potential_sub(cfg)
        phi = random_phi(cfg, seed=k + 1) if s["ic"] == "random" else wo.initial_condition(cfg, s["ic"], seed=k)
        out.append([cfg, par, v, potsub, phi])
        pars.append(par)
    b = wa.Batch(pars)
    for k, (s, m) in enumerate(zip(specs, out)):
        cfg, par, v, potsub, phi = m
        if s["potential"].startswith("host"):
            b.set_potential_host(k, v, potsub[0], potsub[1], potsub[2])
        else:
            b.set_potential(k, s["potential"])
        if s["ic"] == "random":
            b.upload_phi(k, phi)
        else:
            b.set_initial_condition(k, s["ic"], seed=k)
            m[4] = b.download_phi(k)
    return b, out


def context_of(wa, member, phi):
    cfg, par, v, potsub, _ = member
    ctx = wa.Context(par)
    kind, scalar, arr = potsub
    ctx.set_potential_host(v, kind, scalar, arr)
    ctx.upload_phi(phi)
    return ctx


@pytest.mark.parametrize("shape", [(50, 50, 50), (64, 64, 64), (37, 50, 23)])
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_batch_evolve_matches_oracle(wa, wo, shape, ext):
    b, ms = setup_members(wa, wo, shape, ext, MEMBERS)
    with b:
        assert b.kernel_name() == "wafer_k_batch_step"
        abs_ = [wo.ab(m[0], m[2]) for m in ms]
        for steps in (1, 2, 3, 7, 1000):
            b.evolve(steps)
            for k, m in enumerate(ms):
                cfg, phi = m[0], m[4]
                wo.evolve(cfg, 0, abs_[k][0], abs_[k][1], phi, [], steps)
                got = b.download_phi(k)
                assert ulp_diff(got, phi) == 0, (shape, ext, steps, k)
                e = cfg.ext   # the Dirichlet frame stays zero
                assert not np.any(got[:e]) and not np.any(got[-e:]) and not np.any(got[:, :e]) and not np.any(got[:, :, -e:])


@pytest.mark.parametrize("shape,ext", [((50, 50, 50), 1), ((64, 64, 64), 2), ((37, 50, 23), 3)])
def test_batch_observables_match_context_and_oracle(wa, wo, shape, ext):
    b, ms = setup_members(wa, wo, shape, ext, MEMBERS)
    with b:
        b.evolve(5)
        obs = b.observables()
        for k, m in enumerate(ms):
            phi = b.download_phi(k)
            with context_of(wa, m, phi) as ctx:
                want = ctx.observables()
            assert obs[k] == want, (k, obs[k], want)   # bit for bit: the single context's partition and tree
            ref = wo.observables(m[0], m[2], phi, m[3])
            for q in ref:
                assert abs(obs[k][q] - ref[q]) <= REL_SUM * abs(ref[q]), (k, q, obs[k][q], ref[q])
        # normalisation: the same true division as the single context
        before = [b.download_phi(k) for k in range(len(ms))]
        n2 = [o["norm2"] for o in obs]
        b.normalise(n2)
        for k, m in enumerate(ms):
            with context_of(wa, m, before[k]) as ctx:
                ctx.normalise(n2[k])
                assert ulp_diff(b.download_phi(k), ctx.download_phi()) == 0, k


def solve_members(wa, shape, dts, potential="Harmonic"):
    pars = [wa.Params(*shape, dn=0.2, dt=dt, mass=1.0) for dt in dts]
    return pars


def _solve_ref(wa, par, potential, phi, tol, su, max_steps):
    with wa.Context(par) as ctx:
        ctx.set_potential(potential)
        ctx.upload_phi(phi)
        rows, final, converged = ctx.solve_state(0, tol, su, max_steps)
        return rows, final, converged, ctx.download_phi()


def test_batch_solve_matches_contexts(wa, wo):
    shape, tol, su = (32, 32, 32), 1e-7, 50
    dts = [0.0015, 0.004, 0.006, 0.008, 0.012]        # the smallest dt needs the most steps
    pars = solve_members(wa, shape, dts)
    cfg0, _ = make_pair(shape, dn=0.2, dt=dts[0])
    phi0 = wo.initial_condition(cfg0, "Gaussian")
    free = [_solve_ref(wa, p, "Harmonic", phi0, tol, su, None) for p in pars]
    last = [r[0][-1]["step"] for r in free]
    assert all(r[2] for r in free)
    # one max_steps for the batch: every member but the first converges within it, the first does not
    max_steps = max(last[1:])
    assert last[0] > max_steps + su, last
    assert len(set(last)) > 2, last                      # members finish at different blocks
    refs = [_solve_ref(wa, p, "Harmonic", phi0, tol, su, max_steps) for p in pars]
    with wa.Batch(pars) as b:
        for k in range(len(pars)):
            b.set_potential(k, "Harmonic")
            b.upload_phi(k, phi0)
        got = b.solve(tol, su, max_steps)
        for k, (rows, final, converged, status) in enumerate(got):
            rrows, rfinal, rconv, rphi = refs[k]
            assert rows == rrows, k
            assert final == rfinal, k
            assert converged == rconv == (k != 0), k
            assert status == (wa.engine.WAFER_ERR_MAX_STEP if k == 0 else wa.engine.WAFER_OK), (k, status)
            assert ulp_diff(b.download_phi(k), rphi) == 0, k


def test_batch_solve_non_finite_member(wa, wo):
    shape, tol, su = (24, 24, 24), 1e-6, 50
    dts = [0.004, 0.008, 0.006]
    pars = solve_members(wa, shape, dts) + [wa.Params(*shape, dn=0.2, dt=0.005)]
    cfg0, _ = make_pair(shape, dn=0.2, dt=dts[0])
    phi0 = wo.initial_condition(cfg0, "Gaussian")
    bad = phi0.copy()
    bad[5, 6, 7] = np.nan
    refs = [_solve_ref(wa, p, "Harmonic", phi0, tol, su, 20000) for p in pars[:3]]
    with wa.Batch(pars) as b:
        for k in range(4):
            b.set_potential(k, "Harmonic")
            b.upload_phi(k, bad if k == 3 else phi0)
        got = b.solve(tol, su, 20000)
    assert got[3][3] == wa.engine.WAFER_ERR_STATE
    for k in range(3):
        rows, final, converged, status = got[k]
        assert (rows, final, converged) == refs[k][:3], k
        assert status == wa.engine.WAFER_OK


def test_batch_active_mask(wa, wo):
    b, ms = setup_members(wa, wo, (40, 36, 44), 1, MEMBERS)
    with b:
        before = [b.download_phi(k) for k in range(len(ms))]
        mask = [1, 0, 1, 0, 1]
        b.evolve(3, active=mask)
        for k, m in enumerate(ms):
            got = b.download_phi(k)
            if mask[k]:
                a_, b_ = wo.ab(m[0], m[2])
                wo.evolve(m[0], 0, a_, b_, m[4], [], 3)
                assert ulp_diff(got, m[4]) == 0, k
            else:
                assert got.tobytes() == before[k].tobytes(), k
        # a member left out of one call continues from where it stood
        b.evolve(2)
        for k, m in enumerate(ms):
            a_, b_ = wo.ab(m[0], m[2])
            wo.evolve(m[0], 0, a_, b_, m[4], [], 2)
            assert ulp_diff(b.download_phi(k), m[4]) == 0, k


def test_batch_of_one_equals_context(wa, wo):
    b, ms = setup_members(wa, wo, (64, 64, 64), 1, MEMBERS[:1])
    with b:
        m = ms[0]
        with context_of(wa, m, m[4]) as ctx:
            b.evolve(11)
            ctx.evolve(0, 11)
            assert ulp_diff(b.download_phi(0), ctx.download_phi()) == 0
            assert b.observables()[0] == ctx.observables()


def test_batch_of_64_at_32(wa, wo):
    shape = (32, 32, 32)
    pars = [wa.Params(*shape, dn=0.2, dt=0.002 + 0.00015 * k, mass=1.0 + 0.01 * k) for k in range(64)]
    with wa.Batch(pars) as b:
        cfgs = [make_pair(shape, potential="Harmonic" if k % 2 else "Coulomb", dn=0.2, dt=pars[k].dt, mass=pars[k].mass)[0]
                for k in range(64)]
        phis = [wo.initial_condition(c, "Gaussian") for c in cfgs]
        for k in range(64):
            b.set_potential(k, "Harmonic" if k % 2 else "Coulomb")
            b.upload_phi(k, phis[k])
        b.evolve(10)
        obs = b.observables()
        for k in range(0, 64, 9):
            cfg, phi = cfgs[k], phis[k]
            v = wo.potential_generate(cfg)
            a_, b_ = wo.ab(cfg, v)
            wo.evolve(cfg, 0, a_, b_, phi, [], 10)
            assert ulp_diff(b.download_phi(k), phi) == 0, k
            ref = wo.observables(cfg, v, phi, wo.potential_sub(cfg))
            assert abs(obs[k]["energy"] - ref["energy"]) <= REL_SUM * abs(ref["energy"]), k
