"""Mixed-shape batches whose members SHARE shapes (1 < num_shapes < n_members), and active sets that empty a shape, on the MI355X.

A mixed batch indexes two things by member (the array offsets off[m]; the partials offsets obs_off, n2_off) and one thing by shape
(the geometry, geoms[shape_of[m]]).  tests/test_gpu_batch_mixed.py gives every member a shape of its own, so there shape_of[m] == m
and the two indexings cannot be told apart.  Here most members have shape_of[m] != m, members that share a shape differ in
everything else, and the masks freeze member 0, the largest member, and every member of a shape -- so the kernels' "one-shape"
arguments (taken from geoms[0] and from the first active member) and their grid extents (taken from the largest launched member)
come from members other than the ones the existing tests take them from.

The bars are the project's own: 0 ulp against the oracle, byte equality against a Context of the member's own Params, == on the
observables, REL_SUM where tests/test_gpu_batch_mixed.py uses it.  tests/test_batch_mixed_plan.py feeds SHAPE_LIST and masks() to
the host plan without a GPU: the evidence that these inputs separate the two indexings."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.gpu_common import make_pair, random_phi, ulp_diff  # noqa: E402
from tests.test_gpu_batch_mixed import CALLS, REL_SUM, expected_passes, host_v, same_bits  # noqa: E402

# ragged in every axis; a second 128-element pitch tile on doubles, fewer rows than a 12-row fused tile, thinner than a fused chunk;
# one workgroup; one column past a 64-wide tile, odd rows, nz < 2R+1 at R = 3; enough planes for several z-chunks -- the largest by
# cells and by observables workgroups; wider than one 256-wide float observables tile and five 64-wide normalise tiles -- many
# tiles per plane but few planes, so with (37, 50, 23) frozen the normalise grid takes max_tiles from it and max_planes from another
SHAPES = [(37, 50, 23), (130, 6, 5), (8, 8, 8), (65, 13, 3), (40, 36, 44), (260, 5, 4)]
LARGEST, WIDEST, SMALLEST = 4, 5, 2
# dt <= 0.2 mass dn^2 throughout: every member decays under all three stencils (no growing mode to amplify rounding)
SPECS = [
    dict(potential="Harmonic", dn=0.2, dt=0.004, mass=1.0),
    dict(potential="Coulomb", dn=0.25, dt=0.005, mass=0.5),
    dict(potential="host_potsub", dn=0.3, dt=0.003, mass=1.5),   # host V with a pot_sub array
    dict(potential="Harmonic", dn=0.25, dt=0.006, mass=2.0),
    dict(potential="Coulomb", dn=0.3, dt=0.0045, mass=1.0),
    dict(potential="host_potsub", dn=0.2, dt=0.0035, mass=0.5),
]
# (shape index, spec index) of every member.  Shapes 0 1 0 2 4 1 3 5 2 4 2 0: (37,50,23) and (8,8,8) three times, (130,6,5) and
# (40,36,44) twice.
MEMBERS = [(0, 0), (1, 3), (0, 1), (2, 0), (4, 3), (1, 4), (3, 2), (5, 5), (2, 1), (4, 5), (2, 2), (0, 2)]
N = len(MEMBERS)
SHAPE_LIST = [SHAPES[s] for s, _ in MEMBERS]   # what tests/test_batch_mixed_plan.py feeds the plan driver
IN_ORDER = list(range(N))
REVERSED = IN_ORDER[::-1]
PERMUTED = [7, 10, 4, 3, 0, 1, 9, 6, 8, 11, 5, 2]   # the shapes first appear in another order: 5 2 4 0 1 3


def first_appearance(shapes):
    """the batch's table of distinct shapes, and every member's index into it (wafer_batch_layout's rule)"""
    table = list(dict.fromkeys(shapes))
    return table, [table.index(s) for s in shapes]


def cells(shape):
    return shape[0] * shape[1] * shape[2]


def tiles(shape):
    """64 x 4 tiles per plane: the one-step and normalise kernels'"""
    return ((shape[0] + 63) // 64) * ((shape[1] + 3) // 4)


def masks(shapes):
    """the active sets of test 4 for a list of member shapes, as lists of 0/1:
    (a) every member of the most-used shape frozen; (b) member 0 and every member of the largest shape frozen; (c) only the
    two members of one shared shape active; (d) only the (260, 5, 4) member and one (8, 8, 8) member active"""
    shapes = list(shapes)
    count = {s: shapes.count(s) for s in shapes}
    most = max(count, key=lambda s: (count[s], -shapes.index(s)))
    largest = max(count, key=cells)
    pair = next(s for s in shapes if count[s] == 2 and s != largest)
    out = {
        "a_most_used_shape_frozen": [int(s != most) for s in shapes],
        "b_member0_and_largest_frozen": [int(m != 0 and s != largest) for m, s in enumerate(shapes)],
        "c_one_shared_shape_active": [int(s == pair) for s in shapes],
        "d_widest_and_one_smallest_active": [int(m in (shapes.index(SHAPES[WIDEST]), shapes.index(SHAPES[SMALLEST]))) for m in range(len(shapes))],
    }
    return out


MASK_NAMES = sorted(masks(SHAPE_LIST))


def _check_member_list():
    """what the list is for; asserted at import so that it is not simplified later"""
    assert N >= 9 and sorted(PERMUTED) == IN_ORDER and len(set(MEMBERS)) == N
    assert max(SHAPES, key=cells) == SHAPES[LARGEST]
    # the normalise grid takes its tile count from one member and its plane count from another -- with everyone active ((37, 50, 23):
    # 13 tiles of 64 x 4; (40, 36, 44): 44 planes), with (37, 50, 23) frozen ((260, 5, 4): 10 tiles, 4 planes) and under mask (d)
    for active in ([1] * N, masks(SHAPE_LIST)["a_most_used_shape_frozen"], masks(SHAPE_LIST)["d_widest_and_one_smallest_active"]):
        on = [s for s, a in zip(SHAPE_LIST, active) if a]
        assert max(on, key=tiles) != max(on, key=lambda s: s[2]), active
    assert max(set(SHAPE_LIST) - {SHAPES[0]}, key=tiles) == SHAPES[WIDEST] and SHAPES[WIDEST][0] > 256
    tables = []
    for order in (IN_ORDER, REVERSED, PERMUTED):
        shapes = [SHAPE_LIST[k] for k in order]
        table, shape_of = first_appearance(shapes)
        tables.append(table)
        assert 1 < len(table) < N
        assert sum(1 for m, k in enumerate(shape_of) if k != m) > N // 2, shape_of            # shape_of[m] != m for most members
        # a shape reappears after another shape has first appeared
        assert any(shape_of[m] < max(shape_of[:m]) for m in range(1, N)), shape_of
        assert shapes[0] != SHAPES[LARGEST] and shape_of[-1] != len(table) - 1, shape_of
    assert len({tuple(t) for t in tables}) == 3   # three orders of first appearance
    uses = sorted(SHAPE_LIST.count(s) for s in set(SHAPE_LIST))
    assert uses[-1] >= 3 and uses[-3] >= 2, uses
    assert set(SHAPE_LIST) == set(SHAPES)
    for i in range(N):   # members that share a shape differ in everything else (the start: member()'s seed is the pair's own)
        for j in range(i + 1, N):
            if MEMBERS[i][0] == MEMBERS[j][0]:
                a, b = SPECS[MEMBERS[i][1]], SPECS[MEMBERS[j][1]]
                assert all(a[q] != b[q] for q in ("potential", "dn", "dt", "mass")), (i, j)
    for name, mask in masks(SHAPE_LIST).items():
        assert 0 < sum(mask) < N, name
    m = masks(SHAPE_LIST)
    frozen = lambda name: {SHAPE_LIST[k] for k in range(N) if not m[name][k]}   # noqa: E731
    active = lambda name: {SHAPE_LIST[k] for k in range(N) if m[name][k]}       # noqa: E731
    assert SHAPES[0] in frozen("a_most_used_shape_frozen") and SHAPES[0] not in active("a_most_used_shape_frozen")
    assert m["b_member0_and_largest_frozen"][0] == 0 and SHAPES[LARGEST] not in active("b_member0_and_largest_frozen")
    assert active("c_one_shared_shape_active") == {SHAPES[1]} and sum(m["c_one_shared_shape_active"]) == 2
    assert active("d_widest_and_one_smallest_active") == {SHAPES[WIDEST], SHAPES[SMALLEST]} and sum(m["d_widest_and_one_smallest_active"]) == 2
    assert all(mask[0] == 0 for name, mask in m.items() if name[0] in "acd")   # the first active member is not member 0


_check_member_list()


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


@functools.lru_cache(maxsize=None)
def member(wo, s, p, ext, dtype="f64"):
    """the member of shape SHAPES[s] and spec SPECS[p]: (cfg, par, v, potsub, phi) -- computed once, shared, never written to"""
    spec = SPECS[p]
    host = spec["potential"] == "host_potsub"
    cfg, par = make_pair(SHAPES[s], ext=ext, potential="Harmonic" if host else spec["potential"], dn=spec["dn"], dt=spec["dt"],
                         mass=spec["mass"], dtype=dtype)
    if host:
        v, potsub = host_v(cfg), (2, 0.0, np.random.default_rng(100 + 10 * s + p).standard_normal(cfg.work_shape))
    else:
        v, potsub = wo.potential_generate(cfg), wo.potential_sub(cfg)
    phi = random_phi(cfg, seed=1 + 10 * s + p)
    for a in (v, phi, potsub[2]):
        if a is not None:
            a.setflags(write=False)
    return cfg, par, v, potsub, phi


def set_up(obj, wo, k, ext, dtype="f64", slot=None, host_arrays=False):
    """member k's potential and start into a Batch (slot given) or a Context, by the same calls"""
    s, p = MEMBERS[k]
    cfg, par, v, potsub, phi = member(wo, s, p, ext, dtype)
    at = () if slot is None else (slot,)
    if host_arrays or SPECS[p]["potential"] == "host_potsub":
        obj.set_potential_host(*at, np.array(v), potsub[0], potsub[1], None if potsub[2] is None else np.array(potsub[2]))
    else:
        obj.set_potential(*at, SPECS[p]["potential"])
    obj.upload_phi(*at, np.array(phi))


def make_batch(wa, wo, ext, dtype="f64", order=IN_ORDER, variant=None, mixed=True, host_arrays=False):
    """slot i of the batch is member order[i]"""
    b = wa.Batch([member(wo, *MEMBERS[k], ext, dtype)[1] for k in order], mixed_shapes=mixed)
    if variant is not None:
        b.set_step_variant(variant)
    for slot, k in enumerate(order):
        set_up(b, wo, k, ext, dtype, slot=slot, host_arrays=host_arrays)
    return b


def make_context(wa, wo, k, ext, dtype="f64", host_arrays=False):
    ctx = wa.Context(member(wo, *MEMBERS[k], ext, dtype)[1])
    set_up(ctx, wo, k, ext, dtype, host_arrays=host_arrays)
    return ctx


@functools.lru_cache(maxsize=None)
def oracle_after(wo, k, ext, steps):
    """member k's fp64 phi after `steps` steps from its start (the oracle; shared by the tests)"""
    cfg, par, v, potsub, phi = member(wo, *MEMBERS[k], ext)
    a_, b_ = wo.ab(cfg, v)
    out = np.array(phi)
    wo.evolve(cfg, 0, a_, b_, out, [], steps)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def context_after(wa, wo, k, ext, dtype, steps):
    """member k's phi after `steps` steps in a Context of its own Params (shared by the tests)"""
    with make_context(wa, wo, k, ext, dtype) as ctx:
        ctx.evolve(0, steps)
        out = ctx.download_phi()
    out.setflags(write=False)
    return out


def reference_after(wa, wo, k, ext, dtype, steps):
    """what member k must hold after `steps` steps: the oracle on fp64 (compared at 0 ulp), a Context on float storage (bytes)"""
    return oracle_after(wo, k, ext, steps) if dtype == "f64" else context_after(wa, wo, k, ext, dtype, steps)


def equals_reference(got, want, dtype):
    return ulp_diff(got, want) == 0 if dtype == "f64" else same_bits(got, want)


def frame_is_zero(phi, e):
    return not (np.any(phi[:e]) or np.any(phi[-e:]) or np.any(phi[:, :e]) or np.any(phi[:, -e:]) or np.any(phi[:, :, :e]) or np.any(phi[:, :, -e:]))


# ---- 1. fp64 evolve against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_shared_shapes_evolve_matches_oracle(wa, wo, ext, variant):
    with make_batch(wa, wo, ext, variant=variant) as b:
        assert b.num_shapes() == len(set(SHAPE_LIST)) == len(SHAPES) < len(b)
        total = 0
        for n in CALLS:
            b.evolve(n)
            total += n
            got = [b.download_phi(k) for k in range(N)]
            for k in range(N):
                assert ulp_diff(got[k], oracle_after(wo, k, ext, total)) == 0, (ext, variant, total, k, MEMBERS[k])
                assert frame_is_zero(got[k], ext), (ext, variant, total, k)
            for i in range(N):   # no two members of one shape hold the same bits: a member read for another would show
                for j in range(i + 1, N):
                    assert MEMBERS[i][0] != MEMBERS[j][0] or not same_bits(got[i], got[j]), (total, i, j)
        # launches of ONE batch: every launch covers all twelve members
        assert b.passes() == expected_passes(ext, variant, CALLS), (b.passes(), b.dispatch())


# ---- 2. float dtypes against Contexts -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("ext", [1, 2, 3])
@pytest.mark.parametrize("dtype", ["f32", "f32fast"])
def test_shared_shapes_float_members_equal_contexts(wa, wo, dtype, ext, variant):
    with make_batch(wa, wo, ext, dtype=dtype, variant=variant) as b:
        d = b.dispatch()
        assert d["dtype"] == dtype and ("float,double" if dtype == "f32" else "float,float") in d["kernel"], d
        assert "WaferBatchGeomTable" in d["kernel"] and d["shapes"] == str(len(SHAPES)), d
        b.evolve(7)
        for k in range(N):
            assert same_bits(b.download_phi(k), context_after(wa, wo, k, ext, dtype, 7)), (dtype, ext, variant, k, MEMBERS[k])


# ---- 3. observables, norm2, normalise ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [1, 2, 3])
@pytest.mark.parametrize("dtype", ["f64", "f32", "f32fast"])
def test_shared_shapes_observables_norm2_and_normalise(wa, wo, dtype, ext):
    """V and pot_sub go up as host arrays here, so that on float storage the oracle can be given what the device holds: the
    arrays rounded to float (uploads round to nearest even)."""
    held = (lambda a: a) if dtype == "f64" else (lambda a: a.astype(np.float32).astype(np.float64))
    with make_batch(wa, wo, ext, dtype=dtype, host_arrays=True) as b:
        b.evolve(5)
        obs, n2 = b.observables(), b.norm2()
        phis = [b.download_phi(k) for k in range(N)]
        b.normalise([o["norm2"] for o in obs])
        for k in range(N):
            cfg, par, v, potsub, _ = member(wo, *MEMBERS[k], ext, dtype)
            with make_context(wa, wo, k, ext, dtype, host_arrays=True) as ctx:
                ctx.upload_phi(phis[k])
                want, want_n2 = ctx.observables(), ctx.norm2()
                print(dtype, ext, MEMBERS[k], obs[k], want, n2[k], want_n2)
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


# ---- 4. masks that empty a shape ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_name", MASK_NAMES)
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dtype", ["f64", "f32fast"])
def test_masks_that_empty_a_shape(wa, wo, dtype, variant, mask_name):
    """evolve and normalise under an active set that freezes whole shapes, member 0 or the largest member, then under its
    complement, then (evolve) with everyone: 7 steps are an odd number of launches under both variants at ext = 1 and 6 an even
    one, so after the second call the two halves of the batch stand in different buffers (cur), side by side in the third."""
    ext = 1
    mask = masks(SHAPE_LIST)[mask_name]
    comp = [1 - a for a in mask]
    done = [0] * N
    with make_batch(wa, wo, ext, dtype=dtype, variant=variant) as b:
        for steps, active in ((7, mask), (6, comp), (3, [1] * N)):
            before = [b.download_phi(k) for k in range(N)]
            b.evolve(steps, active=active)
            for k in range(N):
                got = b.download_phi(k)
                if not active[k]:
                    assert same_bits(got, before[k]), ("evolve: frozen", steps, k)
                    continue
                done[k] += steps
                assert equals_reference(got, reference_after(wa, wo, k, ext, dtype, done[k]), dtype), ("evolve", steps, k, done[k])
        assert done == [10 if a else 9 for a in mask]
        n2 = b.norm2()
        start = [b.download_phi(k) for k in range(N)]
        want = []
        for k in range(N):
            with make_context(wa, wo, k, ext, dtype) as ctx:
                ctx.upload_phi(start[k])
                ctx.normalise(n2[k])
                want.append(ctx.download_phi())
        b.normalise(n2, active=mask)
        for k in range(N):
            assert same_bits(b.download_phi(k), want[k] if mask[k] else start[k]), ("normalise", k, mask[k])
        b.normalise(n2, active=comp)
        for k in range(N):
            assert same_bits(b.download_phi(k), want[k]), ("normalise: complement", k)


# ---- 5. order independence ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext,variant", [(1, 0), (1, 1), (2, 1), (3, 0)])
def test_member_results_do_not_depend_on_the_order(wa, wo, ext, variant):
    def run(order, mixed=True):
        with make_batch(wa, wo, ext, variant=variant, order=order, mixed=mixed) as b:
            b.evolve(7)
            phi, obs, n2 = [b.download_phi(i) for i in range(len(order))], b.observables(), b.norm2()
        return {k: (phi[i], obs[i], n2[i]) for i, k in enumerate(order)}
    first = run(IN_ORDER)
    others = [("reversed", run(REVERSED)), ("permuted", run(PERMUTED))] + [("alone %d" % k, run([k], mixed=False)) for k in range(N)]
    for name, other in others:
        for k, (phi, obs, n2) in other.items():
            assert same_bits(phi, first[k][0]), (name, k)
            assert obs == first[k][1], (name, k, obs, first[k][1])
            assert n2 == first[k][2], (name, k, n2, first[k][2])


# ---- 6. solve with shared shapes, the largest member finishing first ------------------------------------------------------------------
def test_shared_shapes_solve_largest_finishes_first(wa, wo):
    """dt chosen with the oracle's solve (Harmonic, dn 0.2, Gaussian start, tolerance 1e-6, rows every 50 steps) so that the two
    members of the largest shape converge first, at different blocks, and one small member runs into max_steps: solve's active
    set then freezes the largest members while the small ones go on.  The oracle's last rows: (24, 24, 24) at dt 0.012 step 600
    and at 0.008 step 900; (16, 16, 16) at 0.004 step 1200 and at 0.0015 step 2850; (20, 24, 18) at 0.006 step 1300 -- each with
    the row before it at least 6 % above the tolerance and its own at least 17 % below."""
    shapes = [(16, 16, 16), (24, 24, 24), (20, 24, 18), (24, 24, 24), (16, 16, 16)]
    dts = [0.004, 0.012, 0.006, 0.008, 0.0015]
    big, capped = (1, 3), 4
    tol, su = 1e-6, 50
    pars = [wa.Params(*s, dn=0.2, dt=dt, mass=1.0) for s, dt in zip(shapes, dts)]
    phis = [wo.initial_condition(make_pair(s, dn=0.2, dt=dt)[0], "Gaussian") for s, dt in zip(shapes, dts)]

    def ref(k, max_steps):
        with wa.Context(pars[k]) as ctx:
            ctx.set_potential("Harmonic")
            ctx.upload_phi(phis[k])
            rows, final, converged = ctx.solve_state(0, tol, su, max_steps)
            return rows, final, converged, ctx.download_phi()
    n = len(shapes)
    last = [ref(k, None)[0][-1]["step"] for k in range(n)]
    print("last blocks", last)
    small = [k for k in range(n) if k not in big]
    max_steps = max(last[k] for k in small if k != capped)
    assert max(last[k] for k in big) < min(last[k] for k in small), last   # both largest members finish before any smaller one
    assert last[capped] > max_steps + su, last                                  # one small member hits max_steps
    assert last[big[0]] != last[big[1]], last                                   # the members of one shared shape finish apart
    refs = [ref(k, max_steps) for k in range(n)]
    with wa.Batch(pars, mixed_shapes=True) as b:
        assert b.num_shapes() == 3
        for k in range(n):
            b.set_potential(k, "Harmonic")
            b.upload_phi(k, phis[k])
        got = b.solve(tol, su, max_steps)
        for k, (rows, final, converged, status) in enumerate(got):
            rrows, rfinal, rconv, rphi = refs[k]
            assert rows == rrows, k
            assert final == rfinal, k
            assert converged == rconv == (k != capped), k
            assert status == (wa.engine.WAFER_ERR_MAX_STEP if k == capped else wa.engine.WAFER_OK), (k, status)
            assert same_bits(b.download_phi(k), rphi), k


# ---- 7. refusals still name the case ----------------------------------------------------------------------------------------------
def test_state_store_calls_are_refused_with_shared_shapes(wa, wo):
    with make_batch(wa, wo, 1) as b:
        before = [b.download_phi(k) for k in range(N)]
        calls = {
            "wafer_batch_push_state": lambda: b.push_state(),
            "wafer_batch_evolve_state": lambda: b.evolve(1, wnum=1),
            "wafer_batch_set_gs_variant": lambda: b.set_gs_variant(1),
        }
        for name, call in calls.items():
            with pytest.raises(wa.WaferError) as e:
                call()
            assert e.value.code == -1, (name, str(e.value))
            assert "mixed-shape" in str(e.value) and name in str(e.value), (name, str(e.value))
        for k in range(N):
            assert same_bits(b.download_phi(k), before[k]), k
