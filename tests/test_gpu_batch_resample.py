"""Batch.resample_* on the MI355X: ONE source trilinearly resampled onto many members in one launch (wafer_k_batch_trilerp).  Every
member must hold, bit for bit, the oracle's trilerp_resize of the source in a zero frame (rounded to float on float storage) and
what a Context of its Params holds after the corresponding *_resampled call, with that call's bookkeeping; members outside the mask
keep their bits.  Every comparison of arrays is np.array_equal."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.gpu_common import make_pair, random_phi  # noqa: E402

# the repository's ragged, over-one-tile and sub-tile shapes, and a repeated shape
MIXED = [(33, 20, 11), (65, 33, 20), (7, 5, 3), (33, 20, 11)]
ONE = [(33, 20, 11)] * 6
SPECS = [dict(dn=0.2, dt=0.004, mass=1.0), dict(dn=0.25, dt=0.01, mass=0.5), dict(dn=0.2, dt=0.003, mass=1.5),
         dict(dn=0.3, dt=0.02, mass=1.0), dict(dn=0.2, dt=0.005, mass=2.0), dict(dn=0.25, dt=0.006, mass=1.0)]
# (2, 2, 2); upsampling; downsampling on every axis; equal to a member (still resampled under "padded", the identity under "work")
SOURCE_SHAPES = [(2, 2, 2), (9, 6, 5), (40, 37, 23), (33, 20, 11)]
EXTS = [1, 2, 3]
DTYPES = ["f64", "f32", "f32fast"]
BASES = ["padded", "work"]
WAFER_ERR_INVALID, WAFER_ERR_STATE = -1, -4


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
def source(shape, wide=False):
    """random normal data; wide: scaled so that the values span 1e-280 .. 1e280"""
    rng = np.random.default_rng(sum(shape) + 7 * shape[0])
    a = rng.standard_normal(shape)
    if wide:
        a = a * 10.0 ** rng.uniform(-280, 280, shape)
    a.setflags(write=False)
    return a


SOURCES = [source(s) for s in SOURCE_SHAPES] + [source((9, 6, 5), wide=True)]


def stored(a, dtype):
    """what an array of the batch's storage type holds of these doubles"""
    if dtype == "f64":
        return a
    with np.errstate(over="ignore", under="ignore"):
        return a.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def member(shape, k, dtype="f64", ext=1, potential="Harmonic"):
    """(cfg, par, phi) of member k -- computed once, never written to"""
    cfg, par = make_pair(shape, ext=ext, potential=potential, dtype=dtype, sig=0.223, **SPECS[k % len(SPECS)])
    phi = stored(random_phi(cfg, seed=60 + k), dtype)
    phi.setflags(write=False)
    return cfg, par, phi


@functools.lru_cache(maxsize=None)
def expected(src_key, shape, ext, basis, dtype):
    """the oracle: trilerp_resize of the source onto the member's work shape, in a zero frame, as the storage type holds it"""
    from oracle import wafer_oracle as wo
    src = SOURCES[src_key]
    out = np.zeros(tuple(n + 2 * ext for n in shape))
    out[ext:-ext, ext:-ext, ext:-ext] = wo.trilerp_resize(src, shape, basis=tuple(n + 2 * ext for n in shape) if basis == "padded" else shape)
    out = stored(out, dtype)
    out.setflags(write=False)
    return out


def ctx_basis(par, basis):
    return None if basis == "padded" else par.work_shape


def make_batch(wa, shapes, dtype="f64", ext=1, potential="Harmonic", phi=True, set_potential=True, **kind):
    b = wa.Batch([member(s, k, dtype, ext, potential)[1] for k, s in enumerate(shapes)], **kind)
    for k, s in enumerate(shapes):
        if set_potential:
            b.set_potential(k, potential)
        if phi:
            b.upload_phi(k, np.array(member(s, k, dtype, ext, potential)[2]))
    return b


def mixed_kind(shapes, states=False):
    if len(set(shapes)) == 1:
        return {}
    return dict(mixed_shapes=True, state_stores=True) if states else dict(mixed_shapes=True)


# ---- 1. phi and V: the oracle and a Context, every stencil and dtype, both bases ---------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ext", EXTS)
def test_phi_and_potential_of_a_mixed_batch(wo, wa, ext, dtype):
    pars = [member(s, k, dtype, ext)[1] for k, s in enumerate(MIXED)]
    ctxs = [wa.Context(p) for p in pars]
    try:
        with wa.Batch(pars, mixed_shapes=True) as b:
            assert b.num_shapes() == 3
            for key, src in enumerate(SOURCES):
                for basis in BASES:
                    b.resample_phi(np.array(src), basis=basis)
                    for m, shape in enumerate(MIXED):
                        got = b.download_phi(m)
                        want = expected(key, shape, ext, basis, dtype)
                        assert np.array_equal(got, want), (key, basis, m)
                        ctxs[m].upload_phi_resampled(np.array(src), basis=ctx_basis(pars[m], basis))
                        assert np.array_equal(got, ctxs[m].download_phi()), (key, basis, m)
                        if basis == "work":   # the corners: the first sample is the source's first point, the last its last (the q >= n bracket)
                            e = ext
                            assert got[e, e, e] == stored(src[:1, :1, :1], dtype)[0, 0, 0]
                            assert got[-e - 1, -e - 1, -e - 1] == stored(src[-1:, -1:, -1:], dtype)[0, 0, 0]
                            if src.shape == shape:
                                assert same_bits(got[e:-e, e:-e, e:-e], stored(src, dtype))
            # V: the batch holds no download of it; one step from a phi that is non-zero on every work cell reads every cell of it,
            # and the observables sum it
            for key, src in enumerate(SOURCES[:4]):
                for basis in BASES:
                    b.resample_potential(np.array(src), basis=basis)
                    b.resample_phi(np.array(SOURCES[1]), basis="work")
                    obs = b.observables()
                    b.evolve(1)
                    for m in range(len(MIXED)):
                        c = ctxs[m]
                        c.set_potential_resampled(np.array(src), basis=ctx_basis(pars[m], basis))
                        assert np.array_equal(c.download_array("v"), expected(key, MIXED[m], ext, basis, dtype)), (key, basis, m)
                        c.upload_phi_resampled(np.array(SOURCES[1]), basis=pars[m].work_shape)
                        assert obs[m] == c.observables(), (key, basis, m)
                        c.evolve(0, 1)
                        assert np.array_equal(b.download_phi(m), c.download_phi()), (key, basis, m)
    finally:
        for c in ctxs:
            c.close()


# ---- 2. pot_sub -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ext", EXTS)
def test_potsub_of_a_mixed_batch(wo, wa, ext, dtype):
    """basis "work" (input.rs:472), through the observables' v_infinity as a Context's potential_sub is checked"""
    with make_batch(wa, MIXED, dtype, ext, "FullCornell", mixed_shapes=True) as b:
        for key in (1, 2, 3):
            src = SOURCES[key]
            b.resample_potsub(np.array(src))
            obs = b.observables()
            for m, shape in enumerate(MIXED):
                cfg, par, phi = member(shape, m, dtype, ext, "FullCornell")
                with wa.Context(par) as c:
                    c.set_potential("FullCornell")
                    c.set_potsub_resampled(np.array(src))
                    assert c.potsub() == (2, 0.0)
                    assert np.array_equal(c.download_array("potsub"), expected(key, shape, ext, "work", dtype)[ext:-ext, ext:-ext, ext:-ext])
                    c.upload_phi(np.array(phi))
                    assert obs[m] == c.observables(), (key, m)
                if dtype == "f64":
                    sub = np.ascontiguousarray(expected(key, shape, ext, "work", dtype)[ext:-ext, ext:-ext, ext:-ext])
                    want = wo.observables(cfg, wo.potential_generate(cfg), np.array(phi), (2, 0.0, sub))
                    assert obs[m]["v_infinity"] == pytest.approx(want["v_infinity"], rel=1e-12), (key, m)
                    assert obs[m]["v_infinity"] != 0.0
        with pytest.raises(wa.WaferError) as e:
            b.resample_potsub(np.array(SOURCES[1]), basis="padded")
        assert e.value.code == WAFER_ERR_INVALID
        assert b.observables() == obs


# ---- 3. masks, independence -------------------------------------------------------------------------------------------------------
MASKS = [[1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 1, 1], None]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mask", MASKS)
def test_one_shape_batch_under_masks(wa, mask, dtype):
    """six members of one shape, listed one, some (the last among them) and all: the listed ones are the oracle's, the others
    keep phi, V (their observables and their next step) and their stored states bit for bit"""
    ext, src = 2, SOURCES[1]
    listed = [True] * 6 if mask is None else [bool(x) for x in mask]
    with make_batch(wa, ONE, dtype, ext) as b, make_batch(wa, ONE, dtype, ext) as twin:
        for x in (b, twin):
            x.push_state()
        obs0 = b.observables()
        b.resample_phi(np.array(src), active=mask)
        b.resample_state(0, np.array(SOURCES[2]), active=mask, basis="work")
        assert b.num_states() == [1] * 6
        for m in range(6):
            phi = member(ONE[m], m, dtype, ext)[2]
            if listed[m]:
                assert np.array_equal(b.download_phi(m), expected(1, ONE[m], ext, "padded", dtype)), m
                assert np.array_equal(b.download_state(m, 0), expected(2, ONE[m], ext, "work", dtype)), m
            else:
                assert same_bits(b.download_phi(m), phi) and same_bits(b.download_state(m, 0), phi), m
        b.resample_potential(np.array(src), active=mask, basis="work")
        for m in range(6):
            if listed[m]:   # the members start again from their own phi, under the new V
                b.upload_phi(m, np.array(member(ONE[m], m, dtype, ext)[2]))
        obs1 = b.observables()
        b.evolve(2)
        twin.evolve(2)
        for m in range(6):
            if listed[m]:
                assert obs1[m] != obs0[m], m
            else:
                assert obs1[m] == obs0[m] and same_bits(b.download_phi(m), twin.download_phi(m)), m


def test_mixed_batch_under_a_mask(wa):
    """members 1 and 3 listed -- one of the two that share a shape; the padded frame of the listed members is zero"""
    ext, dtype, mask = 1, "f64", [0, 1, 0, 1]
    with make_batch(wa, MIXED, dtype, ext, mixed_shapes=True, state_stores=True) as b:
        for m, s in enumerate(MIXED):   # something non-zero on every padded cell of the targets, the frame included
            b.upload_phi(m, np.full(member(s, m, dtype, ext)[1].padded_shape, 3.0))
        b.push_state()
        obs0 = b.observables()
        b.resample_phi(np.array(SOURCES[2]), active=mask)
        b.resample_state(0, np.array(SOURCES[2]), active=mask)
        b.resample_potential(np.array(SOURCES[1]), active=mask)
        obs1 = b.observables()
        for m, s in enumerate(MIXED):
            got, st = b.download_phi(m), b.download_state(m, 0)
            if mask[m]:
                want = expected(2, s, ext, "padded", dtype)
                assert np.array_equal(got, want) and np.array_equal(st, want), m
                inner = np.zeros(got.shape, dtype=bool)
                inner[ext:-ext, ext:-ext, ext:-ext] = True
                assert not got[~inner].any() and not st[~inner].any() and got[inner].all(), m
            else:
                assert (got == 3.0).all() and (st == 3.0).all() and obs1[m] == obs0[m], m


# ---- 4. guard cells and bookkeeping: steps after resample_potential -------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("ext,dtype", [(1, "f64"), (2, "f64"), (3, "f64"), (1, "f32"), (1, "f32fast")])
def test_three_steps_after_resample_potential(wa, ext, dtype, variant):
    src = SOURCES[1]
    pars = [member(s, k, dtype, ext)[1] for k, s in enumerate(MIXED)]
    with wa.Batch(pars, mixed_shapes=True) as b:
        b.resample_potential(np.array(src))
        for m in range(len(MIXED)):
            b.set_initial_condition(m, "Boolean")
        b.set_step_variant(variant)
        b.evolve(3)
        obs = b.observables()
        for m, par in enumerate(pars):
            with wa.Context(par) as c:
                c.set_potential_resampled(np.array(src))
                c.set_initial_condition("Boolean")
                c.evolve(0, 3)
                assert np.array_equal(b.download_phi(m), c.download_phi()), m
                assert obs[m] == c.observables(), m
                assert c.potsub() == (0, 0.0) and obs[m]["v_infinity"] == 0.0


# ---- 5. stored states ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shapes", [ONE[:3], MIXED], ids=["one-shape", "mixed-states"])
def test_resample_state(wa, shapes, dtype):
    ext, n = 1, len(shapes)
    kind = mixed_kind(shapes, states=True)
    with make_batch(wa, shapes, dtype, ext, **kind) as b, make_batch(wa, shapes, dtype, ext, **kind) as twin:
        b.resample_state(0, np.array(SOURCES[1]))
        assert b.num_states() == [1] * n
        for m, s in enumerate(shapes):
            assert np.array_equal(b.download_state(m, 0), expected(1, s, ext, "padded", dtype)), m
        with pytest.raises(wa.WaferError) as e:   # out of order, for every member: nothing changes
            b.resample_state(2, np.array(SOURCES[1]))
        assert e.value.code == WAFER_ERR_STATE and b.num_states() == [1] * n
        first = [1] + [0] * (n - 1)
        b.resample_state(1, np.array(SOURCES[2]), active=first, basis="work")
        assert b.num_states() == [2] + [1] * (n - 1)
        assert np.array_equal(b.download_state(0, 1), expected(2, shapes[0], ext, "work", dtype))
        with pytest.raises(wa.WaferError) as e:   # state 2 is in order for member 0 only: refused for all, member 0 untouched
            b.resample_state(2, np.array(SOURCES[1]))
        assert e.value.code == WAFER_ERR_STATE and b.num_states() == [2] + [1] * (n - 1)
        b.resample_state(0, np.array(SOURCES[2]))   # an existing state is overwritten, the counts stay
        assert b.num_states() == [2] + [1] * (n - 1)
        for m, s in enumerate(shapes):
            assert np.array_equal(b.download_state(m, 0), expected(2, s, ext, "padded", dtype)), m
        # one excited step against state 0: the same batch set by load_state with the oracle's array
        for m, s in enumerate(shapes):
            twin.load_state(m, 0, np.array(expected(2, s, ext, "padded", dtype)))
        b.evolve(1, wnum=1)
        twin.evolve(1, wnum=1)
        for m in range(n):
            assert same_bits(b.download_phi(m), twin.download_phi(m)), m


def test_a_plain_mixed_batch_refuses_states(wa):
    with make_batch(wa, MIXED, mixed_shapes=True) as b:
        before = [b.download_phi(m) for m in range(len(MIXED))]
        for call in (lambda: b.resample_state(0, np.array(SOURCES[1])), lambda: b.resample_phi(("state", 0, 0))):
            with pytest.raises(wa.WaferError) as e:
                call()
            assert e.value.code == WAFER_ERR_INVALID and "mixed-shape" in str(e.value)
        assert all(same_bits(b.download_phi(m), before[m]) for m in range(len(MIXED)))


# ---- 6. a member as the source ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_resample_member(wa, dtype):
    """coarse (33, 20, 11) -> fine (65, 33, 20) on the device equals the download of the coarse work cells resampled from the host"""
    ext, fine = 2, [0, 1, 0, 0]
    with make_batch(wa, MIXED, dtype, ext, mixed_shapes=True, state_stores=True) as b:
        work = np.ascontiguousarray(b.download_phi(0)[ext:-ext, ext:-ext, ext:-ext])
        for basis in BASES:
            b.resample_phi(("member", 0), active=fine, basis=basis)
            got = b.download_phi(1)
            b.resample_phi(work, active=fine, basis=basis)
            assert got.any() and same_bits(got, b.download_phi(1)), basis
        # state -> phi
        st = np.array(member(MIXED[3], 3, dtype, ext)[2])
        b.load_state(0, 0, st)
        b.resample_phi(("state", 0, 0), active=[0, 1, 1, 0])
        got = [b.download_phi(1), b.download_phi(2)]
        b.resample_phi(np.ascontiguousarray(st[ext:-ext, ext:-ext, ext:-ext]), active=[0, 1, 1, 0])
        assert got[0].any() and same_bits(got[0], b.download_phi(1)) and same_bits(got[1], b.download_phi(2))
        # phi -> state, the source's own store among the targets (another buffer)
        b.resample_state(1, ("member", 0), active=[1, 0, 0, 0])
        b.resample_state(0, ("member", 0), active=[0, 1, 0, 1], basis="work")
        assert b.num_states() == [2, 1, 0, 1]
        got = [b.download_state(0, 1), b.download_state(1, 0), b.download_state(3, 0)]
        b.resample_state(1, work, active=[1, 0, 0, 0])
        b.resample_state(0, work, active=[0, 1, 0, 1], basis="work")
        assert same_bits(got[0], b.download_state(0, 1)) and same_bits(got[1], b.download_state(1, 0)) and same_bits(got[2], b.download_state(3, 0))
        assert same_bits(got[2][ext:-ext, ext:-ext, ext:-ext], work)   # the same shape under "work": the source's bits
        # the source as a target in the same buffer: refused, nothing changes
        before = [b.download_phi(m) for m in range(4)] + [b.download_state(0, 0), b.download_state(1, 0)]
        for call in (lambda: b.resample_phi(("member", 0)), lambda: b.resample_phi(("member", 1), active=[1, 1, 0, 0]),
                     lambda: b.resample_state(0, ("state", 0, 0), active=[1, 1, 0, 0])):
            with pytest.raises(wa.WaferError) as e:
                call()
            assert e.value.code == WAFER_ERR_INVALID
        with pytest.raises(wa.WaferError) as e:   # member 2 holds no state
            b.resample_phi(("state", 2, 0), active=fine)
        assert e.value.code == WAFER_ERR_STATE
        after = [b.download_phi(m) for m in range(4)] + [b.download_state(0, 0), b.download_state(1, 0)]
        assert all(same_bits(x, y) for x, y in zip(before, after)) and b.num_states() == [2, 1, 0, 1]
        b.resample_state(0, ("state", 0, 1), active=[1, 0, 0, 0])   # state 1 onto state 0 of the same member: two buffers
        got = b.download_state(0, 0)
        b.resample_state(0, np.ascontiguousarray(b.download_state(0, 1)[ext:-ext, ext:-ext, ext:-ext]), active=[1, 0, 0, 0])
        assert got.any() and same_bits(got, b.download_state(0, 0))


# ---- 7. errors: all or nothing ----------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing(wa):
    import ctypes as C
    src = np.array(SOURCES[1])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    with make_batch(wa, MIXED, mixed_shapes=True, state_stores=True, set_potential=False, phi=False) as b:
        with pytest.raises(wa.WaferError) as e:   # a source without phi
            b.resample_phi(("member", 0), active=[0, 1, 0, 0])
        assert e.value.code == WAFER_ERR_STATE
        b.set_potential(0, "Harmonic")
        for m, s in enumerate(MIXED):
            b.upload_phi(m, np.array(member(s, m)[2]))
        b.load_state(0, 0, np.array(member(MIXED[0], 0)[2]))
        before = [b.download_phi(m) for m in range(4)] + [b.download_state(0, 0)]
        bad = [
            (lambda: b.resample_phi(np.zeros((1, 5, 5))), WAFER_ERR_INVALID),
            (lambda: b.resample_potential(np.zeros((5, 5, 1))), WAFER_ERR_INVALID),
            (lambda: b._resample(7, 0, src, None, "padded"), WAFER_ERR_INVALID),
            (lambda: b._check(b._L.wafer_batch_resample(b._h, None, 0, 0, dp(src), *src.shape, 5)), WAFER_ERR_INVALID),
            (lambda: b._check(b._L.wafer_batch_resample_member(b._h, None, 1, 0, 4, 0, 0, 0)), WAFER_ERR_INVALID),
            (lambda: b._check(b._L.wafer_batch_resample_member(b._h, None, 1, 0, 0, 1, 0, 0)), WAFER_ERR_INVALID),   # src_kind POTENTIAL
            (lambda: b.resample_potsub(src, basis="padded"), WAFER_ERR_INVALID),
            (lambda: b.resample_potsub(src, active=[1, 0, 1, 0]), WAFER_ERR_STATE),       # member 2 has no potential: member 0 is not set either
            (lambda: b.resample_state(1, src), WAFER_ERR_STATE),                          # in order for member 0 only
            (lambda: b.resample_phi(("state", 0, 1), active=[0, 1, 0, 0]), WAFER_ERR_STATE),
        ]
        for call, code in bad:
            with pytest.raises(wa.WaferError) as e:
                call()
            assert e.value.code == code, str(e.value)
        with pytest.raises(ValueError):
            b.resample_phi(src, basis="frame")
        b.resample_phi(src, active=[0, 0, 0, 0])   # an empty set is no error, whatever the members would say
        b.resample_state(3, src, active=[0, 0, 0, 0])
        b.resample_potsub(src, active=[0, 0, 0, 0])
        after = [b.download_phi(m) for m in range(4)] + [b.download_state(0, 0)]
        assert all(same_bits(x, y) for x, y in zip(before, after)) and b.num_states() == [1, 0, 0, 0]
        with pytest.raises(wa.WaferError):   # the potentials the refused calls named were not set: members 1 to 3 still have none
            b.evolve(1)
        b.resample_potential(src, active=[0, 1, 1, 1])
        b.resample_potsub(src, active=[1, 0, 1, 0])
        b.evolve(1)
        obs = b.observables()
        assert [o["v_infinity"] != 0.0 for o in obs] == [True, False, True, False]


# ---- 8. the wide-range source on the other paths ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_wide_range_source_as_state_potential_and_member_source(wa, dtype):
    """values from 1e-280 to 1e280 (infinities and zeros once rounded to float): a state target, a potential, and a member that holds
    them as the source of another member"""
    ext, key = 2, 4
    src = np.array(SOURCES[key])
    pars = [member(s, k, dtype, ext)[1] for k, s in enumerate(MIXED)]
    with wa.Batch(pars, mixed_shapes=True, state_stores=True) as b:
        b.resample_state(0, src)
        b.resample_phi(src, basis="work")
        for m, s in enumerate(MIXED):
            assert np.array_equal(b.download_state(m, 0), expected(key, s, ext, "padded", dtype)), m
            assert np.array_equal(b.download_phi(m), expected(key, s, ext, "work", dtype)), m
        # member 0 (wide values, finite in its storage type or not) as the source of member 1: the host path from its download
        work = np.ascontiguousarray(b.download_phi(0)[ext:-ext, ext:-ext, ext:-ext])
        for kind, source_ in (("member", ("member", 0)), ("state", ("state", 0, 0))):
            if kind == "state":
                work = np.ascontiguousarray(b.download_state(0, 0)[ext:-ext, ext:-ext, ext:-ext])
            b.resample_phi(source_, active=[0, 1, 0, 0])
            got = b.download_phi(1)
            b.resample_phi(work, active=[0, 1, 0, 0])
            assert np.array_equal(got, b.download_phi(1), equal_nan=True) and np.isfinite(got).any(), kind
        if dtype != "f64":   # (rounded to float this V holds infinities: a step from it is NaN on both sides, nothing to compare)
            return
        b.resample_potential(src)   # V of this range is outside the short forms' range: the bookkeeping must say so, as a Context's does
        for m in range(len(MIXED)):
            b.set_initial_condition(m, "Boolean")
        b.evolve(1)
        for m, par in enumerate(pars):
            with wa.Context(par) as c:
                c.set_potential_resampled(src)
                assert np.array_equal(c.download_array("v"), expected(key, MIXED[m], ext, "padded", dtype)), m
                c.set_initial_condition("Boolean")
                c.evolve(0, 1)
                assert np.array_equal(b.download_phi(m), c.download_phi()), m
