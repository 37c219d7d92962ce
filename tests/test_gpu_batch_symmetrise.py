"""Batch.symmetrise and Batch.set_potsub on the MI355X: one launch applies every member's own symmetry constraint
(wafer_k_batch_symmetrise), on batches of one shape and of several, and each member must end bit for bit where the oracle's
symmetrise_wavefunction and a Context of its own Params end -- the destination buffer included, which is scratch between steps."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.gpu_common import make_pair, random_phi  # noqa: E402

# the context test's shapes: two x-blocks with a ragged edge, odd and even lengths along both mirrored axes
ONE_SHAPE = [(70, 9, 12), (12, 16, 7)]
CONS6 = ["AboutZ", "AntisymAboutZ", "AboutY", "AntisymAboutY", "NotConstrained", "AboutY"]
MIXED = [(70, 9, 12), (12, 16, 7), (8, 8, 8), (65, 13, 3), (130, 6, 5), (12, 16, 7)]
MIXED_CONS = ["AntisymAboutY", "AboutZ", "AntisymAboutZ", "AboutY", "AboutZ", "NotConstrained"]
SPECS = [dict(dn=0.2, dt=0.004, mass=1.0), dict(dn=0.25, dt=0.01, mass=0.5), dict(dn=0.2, dt=0.003, mass=1.5),
         dict(dn=0.3, dt=0.02, mass=1.0), dict(dn=0.2, dt=0.005, mass=2.0), dict(dn=0.25, dt=0.006, mass=1.0)]


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


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@functools.lru_cache(maxsize=None)
def member(shape, k, dtype="f64", ext=3):
    """(cfg, par, phi) of member k: SevenPoint Harmonic with its own dn, dt, mass and start -- computed once, never written to"""
    cfg, par = make_pair(shape, ext=ext, potential="Harmonic", dtype=dtype, **SPECS[k % len(SPECS)])
    phi = random_phi(cfg, seed=40 + k)
    if dtype == "f32":
        phi = phi.astype(np.float32).astype(np.float64)
    phi.setflags(write=False)
    return cfg, par, phi


def make_batch(wa, shapes, dtype="f64", mixed=False, order=None, ext=3):
    order = list(range(len(shapes))) if order is None else list(order)
    b = wa.Batch([member(shapes[k], k, dtype, ext)[1] for k in order], mixed_shapes=mixed)
    for slot, k in enumerate(order):
        b.set_potential(slot, "Harmonic")
        b.upload_phi(slot, np.array(member(shapes[k], k, dtype, ext)[2]))
    return b


# ---- 1. one shape ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", ONE_SHAPE)
def test_one_shape_batch_matches_the_oracle(wo, wa, shape, dtype):
    """six members, six constraints, one call: every member is the oracle's symmetrise of its own start"""
    with make_batch(wa, [shape] * 6, dtype) as b:
        b.symmetrise(CONS6)
        for m, kind in enumerate(CONS6):
            cfg, par, phi = member(shape, m, dtype)
            want = np.array(phi)
            wo.symmetrise(cfg, kind, want)
            got = b.download_phi(m)
            assert np.array_equal(got, want), (m, kind)
            if kind == "NotConstrained":
                assert same_bits(got, phi)


# ---- 2. several shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
def test_mixed_shape_batch_matches_contexts(wa, reverse):
    """a constraint per member, member 0 and the largest frozen: the active ones are a Context's bits, the frozen ones their own"""
    order = list(range(len(MIXED)))
    if reverse:
        order.reverse()
    frozen = {0, 4}   # the member with the most planes and the one with the most tiles per plane: the launch's grid is the others'
    cons = [MIXED_CONS[k] for k in order]
    # the frozen members carry a constraint too: the mask alone must keep them
    cons = [c if c != "NotConstrained" or k not in frozen else "AboutY" for c, k in zip(cons, order)]
    active = [0 if k in frozen else 1 for k in order]
    with make_batch(wa, MIXED, mixed=True, order=order) as b:
        assert b.num_shapes() == 5
        b.symmetrise(cons, active=active)
        for slot, k in enumerate(order):
            cfg, par, phi = member(MIXED[k], k)
            got = b.download_phi(slot)
            if k in frozen:
                assert same_bits(got, phi), k
                continue
            with wa.Context(par) as ctx:
                ctx.upload_phi(np.array(phi))
                ctx.symmetrise(cons[slot])
                assert np.array_equal(got, ctx.download_phi()), (k, cons[slot])


# ---- 3. the destination buffer is scratch between steps ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_run(shape, k, kind, kind2):
    """the oracle: evolve 3, symmetrise, evolve 2 -> first array; then symmetrise(kind2), evolve 1 -> second"""
    from oracle import wafer_oracle as wo
    cfg, par, phi = member(shape, k)
    a_, b_ = wo.ab(cfg, wo.potential_generate(cfg))
    out = np.array(phi)
    wo.evolve(cfg, 0, a_, b_, out, [], 3)
    wo.symmetrise(cfg, kind, out)
    wo.evolve(cfg, 0, a_, b_, out, [], 2)
    first = out.copy()
    wo.symmetrise(cfg, kind2, out)
    wo.evolve(cfg, 0, a_, b_, out, [], 1)
    return first, out


@functools.lru_cache(maxsize=None)
def context_obs(shape, k, kind):
    """observables of a Context that did evolve 3, symmetrise, evolve 2"""
    import wafer_amd as wa
    cfg, par, phi = member(shape, k)
    with wa.Context(par) as ctx:
        ctx.set_potential("Harmonic")
        ctx.upload_phi(np.array(phi))
        ctx.evolve(0, 3)
        ctx.symmetrise(kind)
        ctx.evolve(0, 2)
        return ctx.observables()


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("kind", ["one0", "one1", "mixed"])
def test_dirty_scratch_buffer_and_frame(wo, wa, kind, variant):
    """steps dirty the other buffer; symmetrise writes into it; the steps after it read its frame.  The NotConstrained member does
    not flip, so the second symmetrise meets members whose current buffers differ."""
    shapes = MIXED if kind == "mixed" else [ONE_SHAPE[int(kind[-1])]] * 6
    cons = MIXED_CONS if kind == "mixed" else CONS6
    cons2 = cons[1:] + cons[:1]
    with make_batch(wa, shapes, mixed=(kind == "mixed")) as b:
        b.set_step_variant(variant)
        b.evolve(3)
        b.symmetrise(cons)
        b.evolve(2)
        obs = b.observables()
        for m in range(len(shapes)):
            assert np.array_equal(b.download_phi(m), oracle_run(shapes[m], m, cons[m], cons2[m])[0]), m
            assert obs[m] == context_obs(shapes[m], m, cons[m]), m
        b.symmetrise(cons2)
        b.evolve(1)
        for m in range(len(shapes)):
            assert np.array_equal(b.download_phi(m), oracle_run(shapes[m], m, cons[m], cons2[m])[1]), m


# ---- 4. refusals and no-ops -------------------------------------------------------------------------------------------------------
def test_refusals_and_no_ops(wa):
    shape = (12, 16, 7)
    with make_batch(wa, [shape] * 3, ext=1) as b:   # ThreePoint
        before = [b.download_phi(m) for m in range(3)]
        with pytest.raises(wa.WaferError, match="SevenPoint") as e:
            b.symmetrise(["NotConstrained", "AboutY", "NotConstrained"])
        assert e.value.code == -1
        b.symmetrise(["NotConstrained"] * 3)
        b.symmetrise([0, 0, 0], active=[1, 0, 1])
        b.symmetrise(["NotConstrained", "AboutY", "NotConstrained"], active=[1, 0, 1])   # the constrained member is not active
        for m in range(3):
            assert same_bits(b.download_phi(m), before[m])
    with make_batch(wa, [shape] * 3) as b:   # SevenPoint
        before = [b.download_phi(m) for m in range(3)]
        for bad in (5, -1):
            with pytest.raises(wa.WaferError) as e:
                b.symmetrise([1, bad, 0])
            assert e.value.code == -1
        b.symmetrise([1, 5, 0], active=[1, 0, 1])   # out of range on a frozen member: not looked at
        assert not same_bits(b.download_phi(0), before[0])
        assert same_bits(b.download_phi(1), before[1]) and same_bits(b.download_phi(2), before[2])
        with pytest.raises(ValueError):
            b.symmetrise([1, 1])
    par = member(shape, 0)[1]
    with wa.Batch([par, par]) as b:
        b.upload_phi(0, np.array(member(shape, 0)[2]))
        with pytest.raises(wa.WaferError) as e:
            b.symmetrise(["AboutY", "AboutY"])   # member 1 has no phi
        assert e.value.code == -4   # WAFER_ERR_STATE
        assert same_bits(b.download_phi(0), member(shape, 0)[2])   # nothing changed
        b.symmetrise(["AboutY", "AboutY"], active=[1, 0])


# ---- 5. set_potsub ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True])
def test_set_potsub_matches_a_context(wa, mixed):
    shapes = [(20, 17, 22), (12, 16, 7), (8, 8, 8)] if mixed else [(20, 17, 22)] * 3
    pairs = [make_pair(s, ext=2, potential="SimpleCornell", dn=0.15, dt=0.003, mass=1.4, sig=0.223) for s in shapes]
    phis = [random_phi(cfg, seed=4 + k) for k, (cfg, par) in enumerate(pairs)]
    args = [(0, 0.0, None), (1, 0.75, None), (2, 0.0, np.random.default_rng(12).standard_normal(pairs[2][0].work_shape))]
    with wa.Batch([par for cfg, par in pairs], mixed_shapes=mixed) as b:
        with pytest.raises(wa.WaferError):
            b.set_potsub(1, 1, 0.75)   # no potential yet
        with pytest.raises(ValueError):
            b.set_potsub(3, 1, 0.75)   # no such member
        for m in range(3):
            b.set_potential(m, "SimpleCornell")
            b.set_potsub(m, *args[m])
            b.upload_phi(m, phis[m])
        got = b.observables()
    for m, (cfg, par) in enumerate(pairs):
        with wa.Context(par) as ctx:
            ctx.set_potential("SimpleCornell")
            ctx.set_potsub(*args[m])
            ctx.upload_phi(phis[m])
            assert got[m] == ctx.observables(), m
    assert got[0]["v_infinity"] == 0.0 and got[1]["v_infinity"] != 0.0 and got[2]["v_infinity"] != 0.0
