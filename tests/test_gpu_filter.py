"""The Chebyshev filter of the stored states on the device: wafer_k_batch_store_filter through Batch.filter_states, the context's
wafer_k_filter_step through Context.filter_states, the spectral bound, the refusals, and Chebyshev-filtered subspace iteration
(solve_filtered) against the numpy backend of tests/filter_model.py.

The one guarantee: after filter_states every one of the first k stored states holds, bit for bit (==, uint64 views of the values,
which the storage type holds exactly), what tests/filter_model.py's filter gives from the same state, V and interval -- on f64, f32
and f32fast, ext 1 - 3.  The model knows neither k nor the other members nor who is listed, so equality with it for members with
k = 1, 2, 3, 5, 8 (a partial group, a full one, two groups) is also independence of all three; identical members with different k
are compared with each other directly as well.  phi, the states from k on, V, pot_sub (an array on the even members, a scalar on
the odd ones, read back after every call), every member not listed and every member listed with k = 0 keep every bit.

Shapes (tests/test_gpu_store_step.py's): (12, 10, 9) odd and smaller than a tile in x; (65, 6, 5) puts a column past the 64-wide tile
and gives a ragged tile row; (5, 4, 20) is cut into several z-chunks by the workgroup table.  The context kernel's 16-byte vectors
get the residual tests' wide shapes, (130, 20, 40) on f64 and (258, 20, 40) on float storage.  The calls of degree 1, 2, 3, 4 follow
one another on the same store: the first step alone, the first in-place overwrite, an odd degree with its trailing copy, an even
one -- and a later call starts from what an earlier one left in the slots and the shadows.  States are N(0, 1) inside a zero frame
(test_batch_bits_on_a_nonzero_frame: inside an N(0, 1) frame, which an even degree keeps and an odd one zeroes),
the potential is Harmonic (the residual tests': every division stays where wafer_div_invariant has the bits of /), and the
intervals put [a, b] over the spectrum and a0 below it, so nothing grows over the ten steps."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import filter_model as fm  # noqa: E402
from tests import ritz_model as rm  # noqa: E402

DT = 0.004
DTYPES = ["f64", "f32", "f32fast"]
SHAPES = [(12, 10, 9), (65, 6, 5), (5, 4, 20)]
DEGREES = [1, 2, 3, 4]
COMBOS = [(dtype, ext) for dtype in DTYPES for ext in (1, 2, 3)]


def storage_of(dtype):
    return np.float64 if dtype == "f64" else np.float32


def wide_shape(dtype):
    return (130, 20, 40) if dtype == "f64" else (258, 20, 40)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


def member(wa, shape, ext, dtype, m, max_states=10):
    """member m's Params: its own dn and mass (dt <= dn^2 / 3 for every one of them)"""
    return wa.Params(*shape, dn=0.2 + 0.03 * m, dt=DT, mass=1.3 - 0.1 * m, central_difference=ext, dtype=dtype, max_states=max_states)


def cfg_of(p, ext):
    return fm.Cfg(ext, p.dn, p.mass)


def interval(m):
    """member m's (a, b, a0): every member its own"""
    return 4.0 + m, 400.0 + 10.0 * m, 0.5 + 0.25 * m


def arrays_for(members, dtype, ext, counts, seed, frame=False):
    """per member counts[m] N(0, 1) arrays on the work cells inside a zero (or N(0, 1)) frame, rounded to the storage type"""
    return [rm.random_states(p.work_shape, ext, counts[m], seed + 17 * m, frame=frame, storage=storage_of(dtype)) for m, p in enumerate(members)]


def set_sub(target, p, m=None, seed=0):
    """a pot_sub of its own on a context (m None) or on member m of a batch: an N(0, 1) array of the work shape where m is even,
    a scalar where it is odd"""
    i = 0 if m is None else m
    args = (2, 0.0, np.random.default_rng(1000 + seed + i).standard_normal(p.work_shape)) if i % 2 == 0 else (1, -0.75 + i)
    if m is None:
        target.set_potsub(*args)
    else:
        target.set_potsub(m, *args)
    assert sub_of(target, m)[0] == args[0]


def sub_of(target, m=None):
    """(kind, scalar, the array where pot_sub is one) as the context or member m holds it now"""
    kind, scalar = target.potsub() if m is None else target.potsub(m)
    arr = None
    if kind == 2:
        arr = target.download_array("potsub") if m is None else target.download_array(m, "potsub")
    return kind, scalar, arr


def same_sub(x, y):
    return x[0] == y[0] and same(np.array([x[1]]), np.array([y[1]])) and (x[0] != 2 or same(x[2], y[2]))


def make_batch(wa, members, pots, states, phis):
    mixed = len({p.work_shape for p in members}) > 1
    b = wa.Batch(members, mixed_shapes=mixed, state_stores=mixed)
    if pots is not None:
        b.set_potentials(pots)
    for m, ls in enumerate(states):
        for j, l in enumerate(ls):
            b.load_state(m, j, l)
    if phis is not None:
        for m, phi in enumerate(phis):
            b.upload_phi(m, phi)
    return b


# ---- 1. batch bits -------------------------------------------------------------------------------------------------------------------------
def check_batch(wa, shapes, nst, ks, active, dtype, ext, seed, frame=False, degrees=DEGREES):
    B = len(shapes)
    members = [member(wa, shape, ext, dtype, m) for m, shape in enumerate(shapes)]
    states = arrays_for(members, dtype, ext, nst, seed, frame=frame)
    phis = [a[0] for a in arrays_for(members, dtype, ext, [1] * B, seed + 5000)]
    listed = [m for m in range(B) if active is None or active[m]]
    ivs = [interval(m) for m in range(B)]
    with make_batch(wa, members, ["Harmonic"] * B, states, phis) as b:
        for m in range(B):
            set_sub(b, members[m], m, seed)
        vs = [b.download_array(m, "v") for m in range(B)]
        subs = [sub_of(b, m) for m in range(B)]
        want = {m: [l.copy() for l in states[m][:ks[m]]] for m in listed}
        launches = 0
        assert b.filter_counts() == (0, 0)
        for degree in degrees:
            b.filter_states(degree, [iv[0] for iv in ivs], [iv[1] for iv in ivs], [iv[2] for iv in ivs], ks, active=active)
            launches += degree + (degree % 2)
            assert b.filter_counts()[0] == launches, (degree, b.filter_counts(), launches)   # degree launches, or degree + 1
            assert b.last_evolve_ms()[1] == degree
            for m in range(B):
                k = ks[m] if m in listed else 0
                for j in range(nst[m]):
                    got = b.download_state(m, j)
                    if j >= k:
                        assert same(got, states[m][j]), ("untouched", m, j, degree)
                        continue
                    want[m][j] = fm.filter(cfg_of(members[m], ext), vs[m], want[m][j], degree, *ivs[m], storage=storage_of(dtype))
                    assert same(got, want[m][j]), ("model", shapes[m], dtype, ext, m, j, degree,
                                                   int(np.count_nonzero(bits(got) != bits(want[m][j]))))
                    assert np.all(np.isfinite(got)) and np.any(got)
                assert same(b.download_phi(m), phis[m]), ("phi", m, degree)
                assert same(b.download_array(m, "v"), vs[m]), ("V", m, degree)
                assert same_sub(sub_of(b, m), subs[m]), ("pot_sub", m, degree)
        # a listed member with k = 0 and an empty list cost nothing, their intervals are not read, and every bit stays
        def everything():
            return [[b.download_state(m, j) for j in range(nst[m])] + [b.download_phi(m), b.download_array(m, "v")] for m in range(B)]

        before = everything()
        b.filter_states(3, np.nan, np.nan, np.nan, [0] * B)
        b.filter_states(3, np.nan, np.nan, np.nan, ks, active=[0] * B)
        assert b.filter_counts()[0] == launches
        for m, (was, now) in enumerate(zip(before, everything())):
            assert all(same(x, y) for x, y in zip(was, now)), ("k = 0 / not listed", m)
            assert same_sub(sub_of(b, m), subs[m]), ("pot_sub, k = 0 / not listed", m)


@pytest.mark.parametrize("dtype,ext", COMBOS)
def test_batch_bits_one_shape(wa, dtype, ext):
    """k = 1, 3, 8, and a fourth member that is listed with k = 0 beside them"""
    for s, shape in enumerate(SHAPES):
        check_batch(wa, [shape] * 4, [2, 3, 8, 2], [1, 3, 8, 0], None, dtype, ext, seed=100 * s + ext)


@pytest.mark.parametrize("dtype,ext", COMBOS)
def test_batch_bits_mixed_shapes(wa, dtype, ext):
    """the three shapes in one batch with state stores: k = 1, 3, 8, 2, 5, a sixth member that is not listed and a seventh that is
    listed with k = 0"""
    shapes = SHAPES + [SHAPES[0], SHAPES[1], SHAPES[2], SHAPES[0]]
    check_batch(wa, shapes, [2, 3, 8, 4, 6, 2, 2], [1, 3, 8, 2, 5, 2, 0], [1, 1, 1, 1, 1, 0, 1], dtype, ext, seed=700 + ext)


@pytest.mark.parametrize("dtype,ext", COMBOS)
def test_batch_bits_on_a_nonzero_frame(wa, dtype, ext):
    """states inside an N(0, 1) frame, degree 2 and then 3: the even degree keeps the state's frame, the odd one ends on zeros
    through the whole-span copy -- in a one-shape batch, in a mixed one, and bit for bit what a context holds after the same calls"""
    check_batch(wa, [SHAPES[0]] * 2, [2, 3], [1, 3], None, dtype, ext, seed=300 + ext, frame=True, degrees=(2, 3))
    check_batch(wa, SHAPES, [5, 3, 2], [5, 2, 1], None, dtype, ext, seed=400 + ext, frame=True, degrees=(2, 3))
    shape = SHAPES[1]
    p = member(wa, shape, ext, dtype, 0)
    states = rm.random_states(shape, ext, 3, 500 + ext, frame=True, storage=storage_of(dtype))
    a, b_, a0 = interval(2)
    with wa.Context(p) as ctx, make_batch(wa, [p], ["Harmonic"], [states], None) as b:
        ctx.set_potential("Harmonic")
        for j, l in enumerate(states):
            ctx.load_state(j, l)
        v = ctx.download_array("v")
        want = [l.copy() for l in states[:2]]
        for degree in (2, 3):
            ctx.filter_states(2, degree, a, b_, a0)
            b.filter_states(degree, a, b_, a0, [2])
            for j in range(2):
                want[j] = fm.filter(cfg_of(p, ext), v, want[j], degree, a, b_, a0, storage=storage_of(dtype))
                e = ext
                frame = want[j].copy()
                frame[e:-e, e:-e, e:-e] = 0.0
                assert np.any(frame) == (degree == 2), (degree, j)      # the model: the frame is kept, then zeroed
                assert same(ctx.download_state(j), want[j]), ("context", dtype, ext, degree, j)
                assert same(b.download_state(0, j), want[j]), ("batch", dtype, ext, degree, j)
            assert same(ctx.download_state(2), states[2]) and same(b.download_state(0, 2), states[2]), degree


def test_a_state_does_not_depend_on_k_or_on_who_else_is_listed(wa):
    """three members of the same Params, states and interval with k = 8, 3, 1 -- and the same again with only the middle one listed"""
    dtype, ext, shape = "f64", 2, SHAPES[1]
    p = member(wa, shape, ext, dtype, 0)
    ls = rm.random_states(shape, ext, 8, 41, frame=False)
    out = []
    for active in (None, [0, 1, 0]):
        with make_batch(wa, [p] * 3, ["Harmonic"] * 3, [ls, ls[:3], ls[:1]], None) as b:
            b.filter_states(3, 5.0, 400.0, 1.0, [8, 3, 1], active=active)
            out.append([[b.download_state(m, j) for j in range(n)] for m, n in enumerate([8, 3, 1])])
    full, solo = out
    for j in range(3):
        assert same(full[0][j], full[1][j]), j          # state j for k = 8 is state j for k = 3 ...
        assert same(full[1][j], solo[1][j]), j          # ... whoever else is listed
    assert same(full[0][0], full[2][0])                  # ... and for k = 1
    assert same(solo[0][0], ls[0]) and same(solo[2][0], ls[0]) and not same(full[0][7], ls[7])


@pytest.mark.parametrize("shapes,dtype,ext", [(SHAPES, "f64", 1), (SHAPES, "f32", 3), ([SHAPES[0]] * 3, "f64", 1)])
def test_evolve_states_and_filter_states_interleaved_on_one_batch(wa, shapes, dtype, ext):
    """evolve_states and filter_states are two callers of one host pass and share its tables (the workgroup table of the listed members,
    the per-member k, the shadows, the copy table): the two calls alternate on one batch with changing k and lists, odd and even
    counts, and after every call every stored state of every member holds the bits one Context per member holds after the same
    calls; phi, V, pot_sub and the states from k[m] on stay, and each call's launches go to its own counter."""
    B, nst, seed = 3, [3, 5, 4], 900 + ext
    calls = [("evolve", 3, (3, 0, 4), None), ("filter", 3, (2, 5, 0), (1, 1, 0)), ("evolve", 2, None, None), ("filter", 4, (3, 5, 4), None)]
    members = [member(wa, shape, ext, dtype, m) for m, shape in enumerate(shapes)]
    states = arrays_for(members, dtype, ext, nst, seed)
    phis = [a[0] for a in arrays_for(members, dtype, ext, [1] * B, seed + 5000)]
    ivs = [interval(m) for m in range(B)]
    ctxs = [wa.Context(p) for p in members]
    try:
        for m, ctx in enumerate(ctxs):
            ctx.set_potential("Harmonic")
            ctx.upload_phi(phis[m])
            for j, l in enumerate(states[m]):
                ctx.load_state(j, l)
        with make_batch(wa, members, ["Harmonic"] * B, states, phis) as b:
            assert b.num_shapes() == len(set(shapes))
            for m in range(B):
                set_sub(b, members[m], m, seed)
            vs = [b.download_array(m, "v") for m in range(B)]
            subs = [sub_of(b, m) for m in range(B)]
            held = [[l.copy() for l in states[m]] for m in range(B)]
            n_store, n_filter = 0, 0
            assert b.store_counts() == 0 and b.filter_counts()[0] == 0
            for c, (what, n, k, active) in enumerate(calls):
                ks = [(nst[m] if k is None else k[m]) if active is None or active[m] else 0 for m in range(B)]
                if what == "evolve":
                    b.evolve_states(n, k, active=active)
                    n_store += n + n % 2
                else:
                    b.filter_states(n, [iv[0] for iv in ivs], [iv[1] for iv in ivs], [iv[2] for iv in ivs], k, active=active)
                    n_filter += n + n % 2
                assert (b.store_counts(), b.filter_counts()[0]) == (n_store, n_filter), (c, what)
                assert b.last_evolve_ms()[1] == n
                for m in range(B):
                    if ks[m] and what == "evolve":
                        ctxs[m].evolve_states(ks[m], n)
                    elif ks[m]:
                        ctxs[m].filter_states(ks[m], n, *ivs[m])
                    for j in range(nst[m]):
                        got = b.download_state(m, j)
                        assert same(got, ctxs[m].download_state(j)), ("context", c, what, shapes[m], dtype, ext, m, j)
                        assert same(got, held[m][j]) == (j >= ks[m]), ("from k on, and only there, a state stays", c, what, m, j)
                        assert np.all(np.isfinite(got)) and np.any(got)
                        held[m][j] = got
                    assert same(b.download_phi(m), phis[m]), ("phi", c, m)
                    assert same(b.download_array(m, "v"), vs[m]), ("V", c, m)
                    assert same_sub(sub_of(b, m), subs[m]), ("pot_sub", c, m)
    finally:
        for ctx in ctxs:
            ctx.close()


# ---- 2. contexts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,ext", COMBOS)
def test_context_bits_are_the_models_and_a_one_member_batchs(wa, dtype, ext):
    for shape in (SHAPES[0], wide_shape(dtype)):
        p = wa.Params(*shape, dn=0.2, dt=DT, mass=1.1, central_difference=ext, dtype=dtype, max_states=8)
        arrays = rm.random_states(shape, ext, 4, 900 + ext + sum(shape), frame=False, storage=storage_of(dtype))
        states, phi = arrays[:3], arrays[3]
        k, (a, b_, a0) = 2, interval(1)
        with wa.Context(p) as ctx, make_batch(wa, [p], ["Harmonic"], [states], [phi]) as b:
            ctx.set_potential("Harmonic")
            set_sub(ctx, p)
            set_sub(b, p, 0)
            for j, l in enumerate(states):
                ctx.load_state(j, l)
            ctx.upload_phi(phi)
            ctx.evolve(1, 8)                   # (the two-step excited pass, where it applies, has built its images of the old states)
            ctx.upload_phi(phi)
            v = ctx.download_array("v")
            sub = sub_of(ctx)
            assert same(v, b.download_array(0, "v")) and same_sub(sub, sub_of(b, 0))
            want = [l.copy() for l in states[:k]]
            for degree in DEGREES:
                ctx.filter_states(k, degree, a, b_, a0)
                b.filter_states(degree, a, b_, a0, [k])
                assert ctx.last_evolve_ms()[1] == degree
                for j in range(k):
                    want[j] = fm.filter(fm.Cfg(ext, p.dn, p.mass), v, want[j], degree, a, b_, a0, storage=storage_of(dtype))
                    got = ctx.download_state(j)
                    assert same(got, want[j]), ("model", dtype, ext, shape, degree, j, int(np.count_nonzero(bits(got) != bits(want[j]))))
                    assert same(got, b.download_state(0, j)), ("batch", dtype, ext, shape, degree, j)
                assert same(ctx.download_state(2), states[2]), degree
                assert same(ctx.download_phi(), phi), ("phi / cur", degree)   # (a flipped cur would show the other buffer)
                assert same(ctx.download_array("v"), v)
                assert same_sub(sub_of(ctx), sub) and same_sub(sub_of(b, 0), sub), ("pot_sub", degree)
            ctx.evolve(1, 8)                   # the Gram matrix and the images follow the filtered store
            got = ctx.download_phi()
            final = [ctx.download_state(j) for j in range(3)]
        with wa.Context(p) as fresh:
            fresh.set_potential("Harmonic")
            set_sub(fresh, p)
            for j, l in enumerate(final):
                fresh.load_state(j, l)
            fresh.upload_phi(phi)
            fresh.evolve(1, 8)
            assert same(got, fresh.download_phi()), (dtype, ext, shape)


def test_context_filter_needs_no_phi_and_zeroes_a_dirty_shadow(wa):
    """states on a random frame: evolve_states leaves one of them in the shadow array, frame and all, and the filter's first step
    must not let that show -- an odd degree ends on a zero frame, as in a batch, whose shadows never hold anything else"""
    shape, ext = (12, 10, 9), 1
    p = wa.Params(*shape, dn=0.2, dt=DT, central_difference=ext, max_states=4)
    states = rm.random_states(shape, ext, 2, 5, frame=True)
    a, b_, a0 = interval(0)
    with wa.Context(p) as ctx:
        ctx.set_potential("Harmonic")
        for j, l in enumerate(states):
            ctx.load_state(j, l)
        ctx.evolve_states(2, 1)                # the shadow now holds what was state 1's slot
        for j, l in enumerate(states):
            ctx.load_state(j, l)
        v = ctx.download_array("v")
        ctx.filter_states(2, 3, a, b_, a0)
        for j in range(2):
            want = fm.filter(fm.Cfg(ext, p.dn, p.mass), v, states[j], 3, a, b_, a0)
            assert same(ctx.download_state(j), want), j
            assert not np.any(want[0]) and np.any(states[j][0])
        with pytest.raises(wa.WaferError):    # phi is still not set
            ctx.evolve(0, 1)


# ---- 3. the excited-state steps see the filtered store ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_excited_steps_after_filter_states_equal_a_fresh_batch(wa, variant):
    dtype, ext, shape = "f64", 1, (12, 10, 9)
    members = [member(wa, shape, ext, dtype, m) for m in range(3)]
    pots = ["Harmonic"] * 3
    arrays = arrays_for(members, dtype, ext, [4, 4, 4], 31)
    states, phis = [a[:3] for a in arrays], [a[3] for a in arrays]
    with make_batch(wa, members, pots, states, phis) as b:
        b.set_gs_variant(variant)
        b.evolve(2, wnum=2)                       # the one-pass form has formed its Gram matrices from the old store
        b.filter_states(3, 5.0, 400.0, 1.0, [2, 3, 1])
        filtered = [[b.download_state(m, j) for j in range(3)] for m in range(3)]
        phi_now = [b.download_phi(m) for m in range(3)]
        assert not same(filtered[0][0], states[0][0]) and same(filtered[2][1], states[2][1])
        b.evolve(4, wnum=2)
        got = [b.download_phi(m) for m in range(3)]
        assert b.gs_steps() == ((6, 0) if variant == 1 else (0, 6))   # (the form asked for ran, before and after)
    with make_batch(wa, members, pots, filtered, phi_now) as f:
        f.set_gs_variant(variant)
        f.evolve(4, wnum=2)
        for m in range(3):
            assert same(got[m], f.download_phi(m)), (variant, m)


# ---- 4. refusals change nothing ------------------------------------------------------------------------------------------------------------
def test_batch_refusals_change_nothing(wa):
    from wafer_amd.engine import FILTER_MAX_DEGREE, WAFER_ERR_INVALID, WAFER_ERR_STATE
    dtype, ext, B = "f64", 1, 3
    members = [member(wa, shape, ext, dtype, m) for m, shape in enumerate(SHAPES)]
    arrays = arrays_for(members, dtype, ext, [4, 4, 4], 55)
    states, phis = [a[:3] for a in arrays], [a[3] for a in arrays]
    good = ([5.0] * B, [400.0] * B, [1.0] * B)

    def unchanged(b, vs, subs, count=0):
        for m in range(B):
            assert same(b.download_phi(m), phis[m]), m
            for j in range(3):
                assert same(b.download_state(m, j), states[m][j]), (m, j)
            if vs[m] is not None:
                assert same(b.download_array(m, "v"), vs[m]), m
                assert same_sub(sub_of(b, m), subs[m]), m
        assert b.filter_counts()[0] == count

    def refused(b, ks, code, word, active=None, degree=2, iv=good):
        with pytest.raises(wa.WaferError, match=word) as e:
            b.filter_states(degree, iv[0], iv[1], iv[2], ks, active=active)
        assert e.value.code == code, (ks, e.value)
        unchanged(b, *held[0])

    with make_batch(wa, members, None, states, phis) as b:
        b.set_potential(0, "Harmonic")
        b.set_potential(2, "Cube")
        set_sub(b, members[0], 0)
        set_sub(b, members[2], 2)
        vs = [b.download_array(0, "v"), None, b.download_array(2, "v")]
        held = [(vs, [sub_of(b, 0), None, sub_of(b, 2)])]
        refused(b, [2, 2, 2], WAFER_ERR_STATE, "member 1: potential")       # member 1 has no potential
        with pytest.raises(wa.WaferError, match="member 1") as e:
            b.spectral_bound()
        assert e.value.code == WAFER_ERR_STATE
        unchanged(b, *held[0])
    with make_batch(wa, members, ["Harmonic", "Cube", "Harmonic"], states, phis) as b:
        for m in range(B):
            set_sub(b, members[m], m)
        vs = [b.download_array(m, "v") for m in range(B)]
        held = [(vs, [sub_of(b, m) for m in range(B)])]
        refused(b, [2, 2, 9], WAFER_ERR_INVALID, "member 2")                # above WAFER_RITZ_MAX
        refused(b, [4, 2, 2], WAFER_ERR_STATE, "member 0")                  # above the member's stored states
        refused(b, [2, 2, 4], WAFER_ERR_STATE, "member 2")                  # the checks run for every member before any launch
        refused(b, [2, 2, 2], WAFER_ERR_INVALID, "degree", degree=0)
        refused(b, [2, 2, 2], WAFER_ERR_INVALID, "degree", degree=FILTER_MAX_DEGREE + 1)
        for bad in (([5.0, 5.0, 5.0], [400.0, 400.0, 400.0], [1.0, 5.0, 1.0]),            # a0 == a
                    ([5.0, 5.0, 5.0], [400.0, 4.0, 400.0], [1.0, 1.0, 1.0]),              # b < a
                    ([5.0, np.nan, 5.0], [400.0, 400.0, 400.0], [1.0, 1.0, 1.0]),
                    ([5.0, 5.0, 5.0], [400.0, np.inf, 400.0], [1.0, 1.0, 1.0])):
            refused(b, [2, 2, 2], WAFER_ERR_INVALID, "member 1", iv=bad)
        unchanged(b, *held[0])
        b.filter_states(2, good[0], [400.0, np.nan, 400.0], good[2], [2, 2, 2], active=[1, 0, 1])   # ... which nobody reads of a member not listed
        assert b.filter_counts()[0] == 2 and same(b.download_state(1, 0), states[1][0])
        assert all(same_sub(sub_of(b, m), held[0][1][m]) for m in range(B))
    with wa.Batch(members, mixed_shapes=True) as b:                          # several shapes, no state stores
        b.set_potentials(["Harmonic"] * 3)
        for m in range(B):
            b.upload_phi(m, phis[m])
            set_sub(b, members[m], m)
        vs, subs = [b.download_array(m, "v") for m in range(B)], [sub_of(b, m) for m in range(B)]
        with pytest.raises(wa.WaferError, match="mixed-shape") as e:
            b.filter_states(2, good[0], good[1], good[2], [1, 1, 1])
        assert e.value.code == WAFER_ERR_INVALID and "wafer_batch_filter_states" in str(e.value)
        for m in range(B):
            assert same(b.download_phi(m), phis[m]) and same(b.download_array(m, "v"), vs[m]) and same_sub(sub_of(b, m), subs[m])


def test_context_refusals_change_nothing(wa):
    from wafer_amd.engine import FILTER_MAX_DEGREE, WAFER_ERR_INVALID, WAFER_ERR_STATE
    shape, ext = (12, 10, 9), 1
    arrays = rm.random_states(shape, ext, 4, 77, frame=False)
    states, phi = arrays[:3], arrays[3]

    def refused(ctx, k, code, degree=2, iv=(5.0, 400.0, 1.0)):
        with pytest.raises(wa.WaferError) as e:
            ctx.filter_states(k, degree, *iv)
        assert e.value.code == code, (k, e.value)
        for j in range(3):
            assert same(ctx.download_state(j), states[j]), (k, j)
        assert same(ctx.download_phi(), phi), k
        if held:
            assert same(ctx.download_array("v"), held[0]) and same_sub(sub_of(ctx), held[1]), k

    def loaded(ctx):
        for j, l in enumerate(states):
            ctx.load_state(j, l)
        ctx.upload_phi(phi)

    p = wa.Params(*shape, dn=0.2, dt=DT, central_difference=ext, max_states=10)
    held = []
    with wa.Context(p) as ctx:
        loaded(ctx)
        refused(ctx, 2, WAFER_ERR_STATE)       # no potential
        with pytest.raises(wa.WaferError) as e:
            ctx.spectral_bound()
        assert e.value.code == WAFER_ERR_STATE
        ctx.set_potential("Harmonic")
        set_sub(ctx, p)
        v = ctx.download_array("v")
        held[:] = [v, sub_of(ctx)]
        refused(ctx, 0, WAFER_ERR_INVALID)
        refused(ctx, 9, WAFER_ERR_INVALID)     # above WAFER_RITZ_MAX
        refused(ctx, 4, WAFER_ERR_STATE)       # above the stored states
        refused(ctx, 2, WAFER_ERR_INVALID, degree=0)
        refused(ctx, 2, WAFER_ERR_INVALID, degree=FILTER_MAX_DEGREE + 1)
        for iv in ((5.0, 400.0, 5.0), (5.0, 4.0, 1.0), (np.nan, 400.0, 1.0), (5.0, np.inf, 1.0), (5.0, 400.0, -np.inf)):
            refused(ctx, 2, WAFER_ERR_INVALID, iv=iv)
        assert same(ctx.download_array("v"), v) and same_sub(sub_of(ctx), held[1])
    held[:] = []
    slab = wa.Params(*shape, dn=0.2, dt=DT, central_difference=ext, max_states=10, z_begin=0, z_count=shape[2])
    with wa.Context(slab) as ctx:
        ctx.set_potential("Harmonic")
        set_sub(ctx, slab)
        loaded(ctx)
        held[:] = [ctx.download_array("v"), sub_of(ctx)]
        with pytest.raises(wa.WaferError, match="z-slab"):
            ctx.filter_states(2, 2, 5.0, 400.0, 1.0)
        refused(ctx, 2, WAFER_ERR_INVALID)
        with pytest.raises(wa.WaferError, match="z-slab"):
            ctx.spectral_bound()
        assert same(ctx.download_array("v"), held[0]) and same_sub(sub_of(ctx), held[1])


# ---- 5. the spectral bound -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,ext", COMBOS)
def test_spectral_bound_is_the_models(wa, dtype, ext):
    """==: the maximum of stored values is exact.  A context, a one-shape batch, a mixed batch (with and without state stores); pot_sub
    and V keep every bit"""
    pots = ["Harmonic", "Cube", "Periodic", "NoPotential"]
    shapes = SHAPES + [wide_shape(dtype)]
    members = [member(wa, shape, ext, dtype, m) for m, shape in enumerate(shapes)]
    for stores in (True, False):
        with wa.Batch(members, mixed_shapes=True, state_stores=stores) as b:
            b.set_potentials(pots)
            for m in range(4):
                set_sub(b, members[m], m)
            vs = [b.download_array(m, "v") for m in range(4)]
            subs = [sub_of(b, m) for m in range(4)]
            want = [fm.bound(cfg_of(members[m], ext), vs[m]) for m in range(4)]
            assert b.spectral_bound() == want
            assert b.spectral_bound(active=[0, 1, 0, 1]) == [None, want[1], None, want[3]]
            assert b.filter_counts() == (0, 2)                                   # one launch per call, whatever the members
            assert b.spectral_bound(active=[0, 0, 0, 0]) == [None] * 4 and b.filter_counts() == (0, 2)
            for m in range(4):
                assert same(b.download_array(m, "v"), vs[m]) and same_sub(sub_of(b, m), subs[m]), m
    with wa.Batch([members[1]] * 3) as b:
        b.set_potentials(pots[:3])
        assert b.spectral_bound() == [fm.bound(cfg_of(members[1], ext), b.download_array(m, "v")) for m in range(3)]
    with wa.Context(members[0]) as ctx:
        ctx.set_potential("Harmonic")
        set_sub(ctx, members[0])
        v, sub = ctx.download_array("v"), sub_of(ctx)
        assert ctx.spectral_bound() == want[0]
        assert same(ctx.download_array("v"), v) and same_sub(sub_of(ctx), sub)
    # a potential that is negative everywhere: the largest value, not the largest magnitude
    with wa.Context(members[0]) as ctx:
        v = -1.0 - rm.random_states(shapes[0], ext, 1, 3, frame=True, storage=storage_of(dtype))[0] ** 2
        ctx.set_potential_host(v)
        stored = ctx.download_array("v")
        assert ctx.spectral_bound() == fm.bound(cfg_of(members[0], ext), stored) < fm.ABS_WEIGHT[ext] / (
            {1: 2., 2: 24., 3: 360.}[ext] * members[0].dn ** 2 * members[0].mass)


# ---- 6. solve_filtered on the device -----------------------------------------------------------------------------------------------------------
DN = 0.1
GRIDS = {1: (9, 9, 9), 2: (5, 5, 5), 3: (7, 7, 7)}


def device_v(kind, shape, ext, dn=DN):
    return np.zeros(tuple(n + 2 * ext for n in shape)) if kind == "free" else fm.harmonic_v(shape, ext, dn)


@functools.lru_cache(maxsize=None)
def model_result(kind, shape, ext, dn=DN):
    """the numpy backend's loop on the member of the device run: the same potential and the same starting states; computed once"""
    return fm.solve_filtered([fm.Member(fm.Cfg(ext, dn), device_v(kind, shape, ext, dn), fm.start_states(shape, ext))])[0]


def solver_params(wa, shape, ext, dn=DN):
    return wa.Params(*shape, dn=dn, dt=0.9 * dn * dn / 3.0, central_difference=ext, max_states=8)


def check_against_model(r, model):
    from wafer_amd.engine import FILTER_CONVERGED
    n = fm.K - fm.GUARD
    print(r["status"], r["blocks"], r["evals"], model["blocks"], model["evals"], r["rho"])
    assert r["status"] == model["status"] == FILTER_CONVERGED
    assert r["blocks"] == model["blocks"] and r["steps"] == r["blocks"] * fm.DEGREE and len(r["rows"]) == r["blocks"]
    assert np.all(np.abs(r["evals"][:n] - model["evals"][:n]) <= 1e-9 * np.abs(model["evals"][:n])), (r["evals"], model["evals"])
    assert np.all(r["rho"][:n] < 1e-10), r["rho"]


@pytest.mark.parametrize("kind", ["free", "harmonic"])
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_context_solve_filtered(wa, ext, kind):
    shape = GRIDS[ext]
    with wa.Context(solver_params(wa, shape, ext)) as ctx:
        ctx.set_potential_host(device_v(kind, shape, ext))
        for j, l in enumerate(fm.start_states(shape, ext)):
            ctx.load_state(j, l)
        r = ctx.solve_filtered(fm.K, fm.TOLERANCE, fm.DEGREE, fm.MAX_BLOCKS)
    check_against_model(r, model_result(kind, shape, ext))


def test_batch_solve_filtered_two_shapes_one_stops_earlier(wa):
    """(9, 9, 9) harmonic needs a block less than (8, 9, 10) free: it leaves the active set and its states stay as they are -- the
    bits a batch of that member alone ends with"""
    cases = [("harmonic", (9, 9, 9)), ("free", (8, 9, 10))]
    models = [model_result(kind, shape, 1) for kind, shape in cases]
    assert models[0]["blocks"] + 1 == models[1]["blocks"]
    members = [solver_params(wa, shape, 1) for _, shape in cases]

    def loaded(b, which):
        for m, c in enumerate(which):
            b.set_potential_host(m, device_v(cases[c][0], cases[c][1], 1))
            for j, l in enumerate(fm.start_states(cases[c][1], 1)):
                b.load_state(m, j, l)

    with wa.Batch(members, mixed_shapes=True, state_stores=True) as b:
        loaded(b, [0, 1])
        rs = b.solve_filtered(fm.K, fm.TOLERANCE, fm.DEGREE, fm.MAX_BLOCKS)
        # an even degree: one launch per step for the members still going, whatever their number; one bound launch in all
        assert b.filter_counts() == (fm.DEGREE * max(r["blocks"] for r in rs), 1)
        early = [b.download_state(0, j) for j in range(fm.K)]
    for r, model in zip(rs, models):
        check_against_model(r, model)
    with wa.Batch(members[:1]) as solo:
        loaded(solo, [0])
        r = solo.solve_filtered(fm.K, fm.TOLERANCE, fm.DEGREE, fm.MAX_BLOCKS)[0]
        assert r["blocks"] == rs[0]["blocks"] and np.array_equal(bits(r["evals"]), bits(rs[0]["evals"]))
        for j in range(fm.K):
            assert same(solo.download_state(0, j), early[j]), j
