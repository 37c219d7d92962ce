"""The full arithmetic forms of the step kernels (short_forms(c) false: the IEEE 1 / x for b, x / den with the extra Markstein round
or, in fp32, the division itself) held to the references the short forms are held to, under the three triggers of
tests/full_forms_cases.py: WAFER_FLAG_UNPLANNED_DIV on an in-range V ("unplanned"), a potential with 1 + dt V/2 = 2^600 and -2^450
cells ("huge"), and one with a cell where 1 + dt V/2 rounds to 0 ("tiny"; on float storage V = inf, "inf").

  contexts, ground state   every row of the float kernel table (tests/test_gpu_fp32_reference.py: KERNELS) on f32 and f32fast, every
                           row of F64_ROWS (tests/test_gpu_float_range.py) on f64 -- the three-step rows with the table's switches and
                           on every grid of whole tiles as well -- bit for bit over the whole padded array (any NaN equals any NaN,
                           the frame is +0.0), and every case asserts the kernel instance that ran (VIR = false; XS, DIR and the
                           y-mirrored read VS where the grid and the switches select them)
  contexts, the rest       excited steps (the bar of test_gpu_parity.py::test_excited_state_evolve, no two-step pass, the closed-form V
                           dropped), evolve_states against clone_state_to_phi + evolve(0, n), the sums at REL_SUM
  batches                  five members, planned / unplanned / huge / tiny / planned-and-never-listed, in ONE launch, on one shape
                           and on mixed shapes: ground state (both step variants) against the oracle and a Context of each member's
                           own Params, excited steps (both gs variants), evolve_states, observables / Ritz / residual sums

A reference with more than fc.CAP of its work cells non-finite is not compared at that count (fc.compared; the conditions on the
inputs, and the counts this leaves, are asserted on the CPU by tests/test_full_forms_host.py)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import batch_setup_model as model  # noqa: E402
from tests import fp32_reference as ref  # noqa: E402
from tests import full_forms_cases as fc  # noqa: E402
from tests import residual_model as res  # noqa: E402
from tests import ritz_model as rm  # noqa: E402
from tests.test_gpu_float_range import F64_ROWS  # noqa: E402
from tests.test_gpu_fp32_reference import F3, KERNELS, instance_prefix, params  # noqa: E402

REL_SUM = 1e-12    # every global sum
OBSERVED = set()   # every kernel instance name a case saw after an evolve (printed when the module is done)
FIXED = -3.5       # a theta that is nobody's Rayleigh quotient (tests/test_gpu_residual.py)


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
    yield wafer_amd
    print("\nkernel instances observed by tests/test_gpu_full_forms.py:")
    for name in sorted(OBSERVED):
        print("   ", name)


def sid(shape):
    return "x".join(map(str, shape))


def bits_differ(got, want, storage=np.float64):
    """number of entries whose bit patterns differ (any NaN equals any NaN), over arrays or scalars"""
    return int(ref.differing_bits(np.atleast_1d(got), np.atleast_1d(want), storage).sum())


def host_potential(ctx_or_batch, wo, cfg, v, slot=None):
    """set_potential_host of the (read-only) V with the oracle's pot_sub"""
    kind, scalar, arr = wo.potential_sub(cfg)
    args = (np.array(v), kind, scalar, arr)
    if slot is None:
        ctx_or_batch.set_potential_host(*args)
    else:
        ctx_or_batch.set_potential_host(slot, *args)


# ---- which instance has to run ----------------------------------------------------------------------------------------------------
def vir_false_prefix(kernel, dtype):
    """the template-id of a family that records it, up to and including VIR = false"""
    return (kernel + "<double, double, " if dtype == "f64" else instance_prefix(kernel, dtype)) + "false"


def check_instance(ctx, dtype, kernel, spl, steps, shape, env, v, ext):
    """the kernel named by the row ran; where the family reports a template-id (once a whole pass of it ran) it names VIR = false;
    the three-step kernel names XS = true on grids of whole tiles of ITS tile (128 x 16; all-fp32: 256 x 16) with the direction
    the switches select -- 1 up, 2 down (WAFER_F3_PLAIN_DOWN=1), 0 both (WAFER_F3_SCHED=1 from 16 planes on: two halves marched
    outwards) -- and the y-mirrored read (a trailing `true`) exactly where launch_step3 takes it: fp64, V its own mirror image on
    the bits, at least two tile rows, marching up"""
    instance = ctx.stencil_kernel_instance()
    assert ctx.stencil_kernel_name() == kernel
    if steps < spl or kernel not in ("wafer_k_step3_fused", "wafer_k_step2_wide"):
        assert instance.startswith(kernel), instance
        return instance
    assert instance.startswith(vir_false_prefix(kernel, dtype)), instance
    OBSERVED.add(instance)
    if kernel == "wafer_k_step3_fused":
        args = instance[instance.index("<") + 1:-1].split(", ")
        xs = shape[0] % (256 if dtype == "f32fast" else 128) == 0 and shape[1] % 16 == 0
        halves = env.get("WAFER_F3_SCHED") == "1" and shape[2] >= 16
        direction = 0 if (not xs or halves) else 2 if env.get("WAFER_F3_PLAIN_DOWN") == "1" else 1
        vs = dtype == "f64" and xs and direction == 1 and shape[1] // 16 >= 2 and model.y_symmetric(v, ext)
        want = ["false", "0", "true" if xs else "false", str(direction)] + (["true"] if vs else [])
        assert args[2:] == want, (instance, want)
    return instance


# ---- contexts, ground state -------------------------------------------------------------------------------------------------------
def f64_rows():
    """F64_ROWS; its three-step row once per row of the float table that runs that kernel (the switches and shapes set there)"""
    out = []
    for ext, variant, kernel, spl in F64_ROWS:
        table = [(r[2], fc.shapes_of_row(r[6], r[4])) for r in KERNELS if r[0] == ext and r[1] == 3] if variant == 3 else [({}, ref.RANGE_SHAPES)]
        for env, shapes in table:
            switches = "".join(f"-{k[6:]}={v}" for k, v in env.items() if k != "WAFER_FUSE3_MIN_NY")
            for shape in shapes:
                out.append(pytest.param(ext, variant, env, kernel, spl, shape, id=f"ext{ext}-v{variant}{switches}-{sid(shape)}"))
    return out


def f64_kinds(variant, shape):
    """unplanned, huge, tiny; on the three-step kernel over whole tiles the mirrored huge and tiny too (v_ysym = 1 with v_in_range = 0;
    the base V of these grids is its own mirror image already, so "unplanned" there runs the mirrored read as well)"""
    mirrored = variant == 3 and shape in ref.WHOLE_TILES
    return ["unplanned", "huge", "tiny"] + (["huge_mirror", "tiny_mirror"] if mirrored else [])


def split_kind(kind):
    """-> (the potential's kind in fc.KINDS, unplanned_div)"""
    return kind.replace("unplanned", "base"), kind.startswith("unplanned")


@pytest.mark.parametrize("ext,variant,env,kernel,spl,shape", f64_rows())
def test_fp64_steps_in_the_full_forms_equal_the_oracle(wo, wa, monkeypatch, ext, variant, env, kernel, spl, shape):
    """dtype f64 under unplanned / huge / tiny (and their mirrored potentials on whole tiles): wo.evolve on wo.ab(cfg, V), bit for
    bit over the whole padded array after 1, 2, 3, 7 (and 12) steps from the same uploaded start"""
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    for kind in f64_kinds(variant, shape):
        vkind, unplanned = split_kind(kind)
        cfg, v, phi = fc.case(wo, shape, ext, vkind)
        want = fc.oracle_f64(wo, shape, ext, vkind)
        with wa.Context(params(wa, cfg, "f64", unplanned_div=unplanned)) as ctx:
            ctx.set_stencil_variant(variant)
            host_potential(ctx, wo, cfg, v)
            assert ctx.stencil_kernel_name() == kernel and ctx.steps_per_launch() == spl
            assert ref.describe_mismatch_bits(ctx.download_array("v"), v, ext, storage=np.float64) is None
            for steps in fc.compared(want, ext):
                ctx.upload_phi(np.array(phi))
                ctx.evolve(0, steps)
                got = ctx.download_phi()
                instance = check_instance(ctx, "f64", kernel, spl, steps, shape, env, v, ext)
                msg = ref.describe_mismatch_bits(got, want[steps], ext, storage=np.float64)
                assert msg is None, f"{kind} after {steps} steps of {instance}: {msg}"


def test_the_mirrored_read_runs_in_its_full_form(wo, wa, monkeypatch):
    """the mirrored "huge" on whole tiles, ThreePoint, variant 3, marching up: launch_step3 takes the VS instantiation whatever
    short_forms says (wafer_launch_step3_fused: WAFER_F3_LAUNCH_VS(false)), so it reports VIR = false WITH the trailing true --
    and gives the oracle's bits"""
    for k, val in F3.items():
        monkeypatch.setenv(k, val)
    for shape in ((256, 32, 11), (128, 48, 23)):            # two and three tile rows (an odd count leaves the middle row unpaired)
        cfg, v, phi = fc.case(wo, shape, 1, "huge_mirror")
        want = fc.oracle_f64(wo, shape, 1, "huge_mirror")
        with wa.Context(params(wa, cfg, "f64")) as ctx:
            ctx.set_stencil_variant(3)
            host_potential(ctx, wo, cfg, v)
            for steps in (3, 7):
                ctx.upload_phi(np.array(phi))
                ctx.evolve(0, steps)
                instance = ctx.stencil_kernel_instance()
                OBSERVED.add(instance)
                assert instance == "wafer_k_step3_fused<double, double, false, 0, true, 1, true>", instance
                msg = ref.describe_mismatch_bits(ctx.download_phi(), want[steps], 1, storage=np.float64)
                assert msg is None, f"{shape} after {steps} steps of {instance}: {msg}"


def float_rows():
    out = []
    for row in KERNELS:
        ext, variant, env, kernel, spl, ab, shapes = row
        switches = "".join(f"-{k[6:]}={v}" for k, v in env.items() if k != "WAFER_FUSE3_MIN_NY")
        for shape in fc.shapes_of_row(shapes, spl):
            out.append(pytest.param(row, shape, id=f"ext{ext}-v{variant}{switches}-{sid(shape)}"))
    return out


def run_float_row(wo, wa, setenv, dtype, row, shape, kind, starts, compare):
    """one row of the float table on one shape under one trigger: from each of `starts`, after each count the reference is compared
    at, compare(start, steps, instance, got)"""
    ext, variant, env, kernel, spl, ab, _ = row
    for k, val in env.items():
        setenv(k, val)
    vkind, unplanned = split_kind(kind)
    cfg, v, _ = fc.case(wo, shape, ext, vkind, "f32")
    with wa.Context(params(wa, cfg, dtype, unplanned_div=unplanned)) as ctx:
        ctx.set_stencil_variant(variant)
        host_potential(ctx, wo, cfg, v)
        assert ctx.stencil_kernel_name() == kernel and ctx.steps_per_launch() == spl
        assert ref.describe_mismatch_bits(ctx.download_array("v"), v, ext) is None
        for start in starts:
            phi = fc.start_of(wo, shape, ext, start)
            counts = fc.compared(fc.model_f32(wo, dtype, shape, ext, vkind, ab, start), ext)
            for steps in counts:
                ctx.upload_phi(np.array(phi))
                ctx.evolve(0, steps)
                got = ctx.download_phi()
                instance = check_instance(ctx, dtype, kernel, spl, steps, shape, env, v, ext)
                compare(start, steps, instance, got)


@pytest.mark.parametrize("row,shape", float_rows())
@pytest.mark.parametrize("dtype", ["f32", "f32fast"])
def test_float_steps_in_the_full_forms_equal_the_reference(wo, wa, monkeypatch, dtype, row, shape):
    """every row of the float kernel table under unplanned and V = inf: f32 against the C oracle rounding to float, f32fast against
    the all-float model that DIVIDES (division="ieee": the full form is x / den itself) -- unplanned from the in-domain start and
    from "low", where the planned three instructions are not the quotient (the control below)"""
    ext, ab = row[0], row[5]
    for kind in ("unplanned", "inf"):
        vkind = split_kind(kind)[0]
        starts = ["domain", "low"] if (dtype, kind) == ("f32fast", "unplanned") else ["domain"]

        def compare(start, steps, instance, got):
            want = fc.model_f32(wo, dtype, shape, ext, vkind, ab, start)[steps]
            msg = ref.describe_mismatch_bits(got, want, ext)
            assert msg is None, f"{kind} from {start} after {steps} steps of {instance}: {msg}"

        run_float_row(wo, wa, monkeypatch.setenv, dtype, row, shape, kind, starts, compare)


@pytest.fixture(scope="module")
def low_planned_shares(wo, wa):
    """{case id: {steps: share}}: the share of cells in which the model with the PLANNED division differs from the unplanned f32fast
    kernel on "low", over the whole table (its own runs of the kernels: it depends on no other test)"""
    shares = {}
    for p in float_rows():
        row, shape = p.values
        ext, ab = row[0], row[5]

        def compare(start, steps, instance, got, case=shares.setdefault(p.id, {})):
            other = fc.model_f32(wo, "f32fast", shape, ext, "base", ab, "low", "planned")[steps]
            case[steps] = float(np.mean(ref.differing_bits(got, other)))

        with pytest.MonkeyPatch.context() as mp:
            run_float_row(wo, wa, mp.setenv, "f32fast", row, shape, "unplanned", ["low"], compare)
    return shares


def test_the_unplanned_f32fast_kernels_are_not_the_planned_model_below_the_checked_range(low_planned_shares):
    """the control of the unplanned f32fast comparison: on "low" every division is below 2^-100, where the planned three instructions
    are not the quotient, so a kernel that still ran them would match the division="planned" model and not the one that divides.  The
    share of differing cells is printed per case."""
    for case_id, shares in sorted(low_planned_shares.items()):
        print(f"planned-division model against the unplanned kernel on low, {case_id}: " + ", ".join(f"{n}: {s:.4%}" for n, s in sorted(shares.items())))
    worst = max(max(s.values()) for s in low_planned_shares.values())
    live = sum(1 for s in low_planned_shares.values() if max(s.values()) > 0.0)
    print(f"{live} of {len(low_planned_shares)} cases differ from the planned-division model; largest share of cells {worst:.4%}")
    assert live >= 1


@pytest.mark.parametrize("ext,variant", [(1, 1), (2, 1), (1, 2), (1, 3)])
def test_a_builtin_potential_without_the_plan_drops_the_closed_form(wo, wa, monkeypatch, ext, variant):
    """the ground-state kernels that may evaluate Coulomb in closed form (wafer_launch_step_lds: `dflt` needs v_in_range; the fused
    kernels' VG) under unplanned_div: WAFER_VGEN=1 and WAFER_VGEN=0 give the same bits, the oracle's"""
    for k, val in (F3 if variant == 3 else {}).items():
        monkeypatch.setenv(k, val)
    shape = (150, 37, 29)
    cfg, _, phi = ref.case_inputs(wo, shape, ext, "Coulomb")
    v = wo.potential_generate(cfg)
    a, b = wo.ab(cfg, v)
    want = np.array(phi)
    wo.evolve(cfg, 0, a, b, want, [], 7)
    for vgen in ("1", "0"):
        monkeypatch.setenv("WAFER_VGEN", vgen)
        with wa.Context(params(wa, cfg, "f64", unplanned_div=True)) as ctx:
            ctx.set_stencil_variant(variant)
            ctx.set_potential("Coulomb")
            ctx.upload_phi(np.array(phi))
            ctx.evolve(0, 7)
            msg = ref.describe_mismatch_bits(ctx.download_phi(), want, ext, storage=np.float64)
            assert msg is None, f"WAFER_VGEN={vgen} {ctx.stencil_kernel_instance()}: {msg}"


# ---- contexts: excited states, stored states, sums -----------------------------------------------------------------------------------
STATE_CASES = [pytest.param(s, e, id=f"{sid(s)}-ext{e}") for s in fc.STATE_SHAPES for e in (1, 2, 3)]


@functools.lru_cache(maxsize=None)
def orthonormal_store(wo, shape, ext, wnum, seed=30):
    """an orthonormal set, as converged states would be (tests/test_gpu_parity.py: test_excited_state_evolve)"""
    cfg = fc.case(wo, shape, ext)[0]
    lowers = []
    for i in range(wnum):
        l = np.zeros(cfg.padded_shape)
        fc.work(l, ext)[...] = np.random.default_rng(seed + i).standard_normal(cfg.work_shape)
        wo.orthogonalise(i, l, lowers)
        wo.normalise(l, wo.norm2(cfg, l))
        lowers.append(l)
    return tuple(lowers)


@pytest.mark.parametrize("wnum", [1, 3])
@pytest.mark.parametrize("shape,ext", STATE_CASES)
def test_excited_steps_in_the_full_forms(wo, wa, shape, ext, wnum):
    """evolve(wnum, 5) under unplanned, huge and tiny against wo.evolve with the bar of test_gpu_parity.py::test_excited_state_evolve
    (1e-13 per cell, norm2 to 1e-12, overlaps below 1e-13), and no two-step pass (x2_agree needs short_forms).  Under "tiny" the
    first normalisation meets an infinite norm and the projection spreads NaN: the oracle's state is non-finite in more than fc.CAP
    of the cells, which is asserted of the engine's too and nothing else."""
    steps = 5
    lowers = list(orthonormal_store(wo, shape, ext, wnum))
    for kind in ("unplanned", "huge", "tiny"):
        vkind, unplanned = split_kind(kind)
        cfg, v, phi = fc.case(wo, shape, ext, vkind)
        want = np.array(phi)
        with np.errstate(all="ignore"):
            a, b = wo.ab(cfg, np.array(v))
            wo.evolve(cfg, wnum, a, b, want, lowers, steps)
        with wa.Context(params(wa, cfg, "f64", unplanned_div=unplanned)) as ctx:
            host_potential(ctx, wo, cfg, v)
            for i, l in enumerate(lowers):
                ctx.load_state(i, l)
            ctx.upload_phi(np.array(phi))
            ctx.evolve(wnum, steps)
            assert ctx.x2_passes() == 0, kind
            d = ctx.dispatch(wnum)
            assert d.get("v", "streamed") == "streamed" or d["kernel"] == "wafer_k_xstep2", d
            got, n2 = ctx.download_phi(), ctx.norm2()
        if fc.non_finite_share(want, ext) > fc.CAP:
            assert kind == "tiny" and fc.non_finite_share(got, ext) > fc.CAP
            continue
        assert np.isfinite(want).all(), kind
        err = float(np.max(np.abs(got - want)))
        print(f"{kind} {shape} ext {ext} wnum {wnum}: max|dphi| {err:.3e} norm2 {n2!r} oracle {wo.norm2(cfg, want)!r}")
        assert np.allclose(got, want, rtol=0, atol=1e-13), (kind, err)
        assert n2 == pytest.approx(wo.norm2(cfg, want), rel=1e-12), kind
        for l in lowers:
            assert abs(np.sum(l * got)) < 1e-13, kind


@pytest.mark.parametrize("wnum", [1, 3])
def test_excited_steps_of_a_builtin_potential_without_the_plan_drop_the_closed_form(wo, wa, monkeypatch, wnum):
    """built-in Coulomb under unplanned_div: with WAFER_VGEN=1 the excited-state kernel must stream V (the closed form is evaluated
    with the short reciprocal: wafer_diag_dispatch's `cf` needs short_forms) -- the same bits as with WAFER_VGEN=0, no two-step
    pass; the planned context on the same grid does take the closed form or the two-step pass, so the switch is live here"""
    shape, ext, steps = (130, 36, 40), 1, 6
    cfg, _, phi = ref.case_inputs(wo, shape, ext, "Coulomb")
    lowers = []
    for i in range(wnum):
        l = np.zeros(cfg.padded_shape)
        fc.work(l, ext)[...] = np.random.default_rng(60 + i).standard_normal(cfg.work_shape)
        wo.orthogonalise(i, l, lowers)
        wo.normalise(l, wo.norm2(cfg, l))
        lowers.append(l)
    out, planned = {}, {}
    for vgen in ("1", "0"):
        monkeypatch.setenv("WAFER_VGEN", vgen)
        for unplanned in (True, False):
            with wa.Context(params(wa, cfg, "f64", unplanned_div=unplanned)) as ctx:
                ctx.set_potential("Coulomb")
                for i, l in enumerate(lowers):
                    ctx.load_state(i, l)
                ctx.upload_phi(np.array(phi))
                d = ctx.dispatch(wnum)
                ctx.evolve(wnum, steps)
                if unplanned:
                    assert ctx.x2_passes() == 0
                    assert d["kernel"] == "wafer_k_xstep2" or d["v"] == "streamed", d
                    out[vgen] = ctx.download_phi()
                else:
                    planned[vgen] = (ctx.x2_passes(), d["v"])
    assert bits_differ(out["1"], out["0"]) == 0
    assert planned["1"][0] > 0 or planned["1"][1] == "closed_form", planned


@pytest.mark.parametrize("shape,ext", STATE_CASES)
def test_evolve_states_in_the_full_forms(wo, wa, shape, ext):
    """evolve_states(k, n) == clone_state_to_phi(j) + evolve(0, n), bit for bit (any NaN equals any NaN), n = 1, 3, 7: the statement
    of tests/test_gpu_store_step.py::test_context_evolve_states under unplanned, huge and tiny"""
    k = 2
    for kind in ("unplanned", "huge", "tiny"):
        vkind, unplanned = split_kind(kind)
        cfg, v, _ = fc.case(wo, shape, ext, vkind)
        arrays = rm.random_states(shape, ext, 4, 900 + ext + sum(shape), frame=False)
        states, phi = arrays[:3], arrays[3]
        with wa.Context(params(wa, cfg, "f64", unplanned_div=unplanned, max_states=4)) as ctx:
            host_potential(ctx, wo, cfg, v)
            for n in (1, 3, 7):
                for j, l in enumerate(states):
                    ctx.load_state(j, l)
                want = []
                for j in range(k):
                    ctx.clone_state_to_phi(j)
                    ctx.evolve(0, n)
                    want.append(ctx.download_phi())
                ctx.upload_phi(phi)
                ctx.evolve_states(k, n)
                for j in range(k):
                    msg = ref.describe_mismatch_bits(ctx.download_state(j), want[j], ext, storage=np.float64)
                    assert msg is None, f"{kind} state {j} after {n} steps: {msg}"
                assert bits_differ(ctx.download_state(2), states[2]) == 0 and bits_differ(ctx.download_phi(), phi) == 0, (kind, n)
            if kind == "tiny":
                assert not np.isfinite(want[0]).all()


def damped(states, cells, ext, factor=2.0 ** -305):
    """the states with their values at the given work cells multiplied by 2^-305, as a wavefunction inside a wall of 2^609 is: the
    energy terms V l^2 there are of the size of the others, and every sum of the references stays finite"""
    out = []
    for l in states:
        l = l.copy()
        for cell, _ in cells:
            fc.work(l, ext)[cell] *= factor
        out.append(l)
    return out


@pytest.mark.parametrize("shape,ext", STATE_CASES)
def test_sums_in_the_full_forms(wo, wa, shape, ext):
    """observables() after three steps against wo.observables on the downloaded state (rel 1e-12 of the reference value, which on
    "huge" is the 2^609 cell's term and must be finite); ritz_matrices(3) against tests/ritz_model.py and residuals(3) against
    tests/residual_model.py with the bars of test_gpu_ritz.py::test_matrices_against_the_model and
    test_gpu_residual.py::test_sums_against_the_model (1e-12 of the sum of |terms|), on states damped at huge's cells so that every
    reference is finite"""
    for kind in ("unplanned", "huge"):
        vkind, unplanned = split_kind(kind)
        cfg, v, phi = fc.case(wo, shape, ext, vkind)
        states = damped(rm.random_states(shape, ext, 3, 500 + ext + sum(shape), frame=False), fc.altered_cells("huge", cfg.work_shape, cfg.dt), ext)
        with wa.Context(params(wa, cfg, "f64", unplanned_div=unplanned, max_states=4)) as ctx:
            host_potential(ctx, wo, cfg, v)
            ctx.upload_phi(np.array(phi))
            ctx.evolve(0, 3)
            state, obs = ctx.download_phi(), ctx.observables()
            for j, l in enumerate(states):
                ctx.load_state(j, l)
            h, s = ctx.ritz_matrices(3)
            fixed = ctx.residuals(3, theta=np.full(3, FIXED))
            ray = ctx.residuals(3)
        want = wo.observables(cfg, np.array(v), state, wo.potential_sub(cfg))
        for key in want:
            print(f"{kind} {shape} ext {ext} {key}: got {obs[key]!r} want {want[key]!r}")
            assert np.isfinite(want[key]), (kind, key)
            assert obs[key] == pytest.approx(want[key], rel=REL_SUM, abs=0.0), (kind, key)
        mh, ms, ah, as_ = rm.matrices(cfg, v, states, scales=True)
        assert np.isfinite(mh).all() and np.isfinite(ah).all(), kind
        assert np.all(np.abs(h - mh) <= REL_SUM * ah), (kind, np.max(np.abs(h - mh) / ah))
        assert np.all(np.abs(s - ms) <= REL_SUM * as_), (kind, np.max(np.abs(s - ms) / as_))
        for j, l in enumerate(states):
            for label, out, th in (("fixed", fixed, FIXED), ("rayleigh", ray, ray["theta"][j])):
                r2, wh, s2, awh = res.sums(cfg, v, l, th, scales=True)
                assert np.isfinite(r2) and np.isfinite(awh), (kind, label, j)
                assert out["theta"][j] == th
                assert abs(out["r2"][j] - r2) <= REL_SUM * r2, (kind, label, j, out["r2"][j], r2)
                assert abs(out["norm2"][j] - s2) <= REL_SUM * s2, (kind, label, j)
            _, wh, s2, awh = res.sums(cfg, v, l, 0.0, scales=True)
            assert abs(ray["theta"][j] * ray["norm2"][j] - wh) <= REL_SUM * awh, (kind, j, ray["theta"][j], wh, awh)


# ---- batches: both forms in one launch ------------------------------------------------------------------------------------------------
def member_list(wo, dtype, ext, mixed):
    """[dict(shape, kind, unplanned, listed, cfg, v, phi)] of the five members"""
    spec = fc.F64_MEMBERS if dtype == "f64" else fc.F32_MEMBERS
    out = []
    for shape, (kind, unplanned, listed) in zip(fc.batch_shapes(mixed), spec):
        cfg, v, phi = fc.case(wo, shape, ext, kind, "f64" if dtype == "f64" else "f32")
        out.append(dict(shape=shape, kind=kind, unplanned=unplanned, listed=listed, cfg=cfg, v=v, phi=phi))
    return out


def member_params(wa, m, dtype, max_states=4):
    return params(wa, m["cfg"], dtype, unplanned_div=m["unplanned"], max_states=max_states)


def make_batch(wa, wo, ms, dtype, mixed, max_states=4):
    """the five members with their potentials and starts; the mixed-shape batch with state stores, so that every call works on it"""
    pars = [member_params(wa, m, dtype, max_states) for m in ms]
    b = wa.Batch(pars, mixed_shapes=True, state_stores=True) if mixed else wa.Batch(pars)
    for slot, m in enumerate(ms):
        host_potential(b, wo, m["cfg"], m["v"], slot)
        b.upload_phi(slot, np.array(m["phi"]))
    assert [b.member_info(k)["short_forms"] for k in range(len(ms))] == fc.SHORT_FORMS
    assert b.num_shapes() == len({m["shape"] for m in ms})
    return b


def member_context(wa, wo, m, dtype, max_states=4):
    ctx = wa.Context(member_params(wa, m, dtype, max_states))
    host_potential(ctx, wo, m["cfg"], m["v"])
    return ctx


CONTEXT_RUNS = {}   # (dtype, shape, ext, kind, unplanned) -> {steps: phi} of a Context under default dispatch, computed once


def context_run(wa, wo, m, dtype):
    key = (dtype, m["shape"], m["cfg"].ext, m["kind"], m["unplanned"])
    if key not in CONTEXT_RUNS:
        out = {}
        with member_context(wa, wo, m, dtype) as ctx:
            for steps in fc.BATCH_COUNTS:
                ctx.upload_phi(np.array(m["phi"]))
                ctx.evolve(0, steps)
                out[steps] = ctx.download_phi()
        CONTEXT_RUNS[key] = out
    return CONTEXT_RUNS[key]


def member_reference(wo, m, dtype):
    """{steps: phi} of the member's reference: the oracle on f64, the float models of the context tests above otherwise"""
    ext = m["cfg"].ext
    if dtype == "f64":
        return fc.oracle_f64(wo, m["shape"], ext, m["kind"])
    return fc.model_f32(wo, dtype, m["shape"], ext, m["kind"], "registers")


def run_ground(wa, wo, dtype, ext, variant, mixed):
    ms = member_list(wo, dtype, ext, mixed)
    storage = np.float64 if dtype == "f64" else np.float32
    K = 1 if variant == 0 or ext == 3 else 3 if ext == 1 else 2
    with make_batch(wa, wo, ms, dtype, mixed) as b:
        b.set_step_variant(variant)
        assert b.steps_per_launch() == K
        d = b.dispatch()
        assert d["kernel"].startswith("wafer_k_batch_step<%d" % ext if K == 1 else "wafer_k_batch_stepk<%d,%d" % (ext, K)), d
        assert ("WaferBatchGeomTable" in d["kernel"]) == mixed, d
        fused = single = 0
        for steps in fc.BATCH_COUNTS:
            for slot, m in enumerate(ms):
                b.upload_phi(slot, np.array(m["phi"]))
            b.evolve(steps, active=fc.ACTIVE)
            fused, single = fused + (steps // K if K > 1 else 0), single + (steps % K if K > 1 else steps)
            assert b.passes() == (fused, single), (steps, b.passes())
            for slot, m in enumerate(ms):
                got = b.download_phi(slot)
                if not m["listed"]:
                    assert bits_differ(got, m["phi"], storage) == 0, ("the member not listed", steps)
                    continue
                want = member_reference(wo, m, dtype)
                if steps not in fc.compared(want, ext):
                    continue
                what = f"member {slot} ({sid(m['shape'])}, {m['kind']}{', unplanned' if m['unplanned'] else ''}) after {steps} steps"
                msg = ref.describe_mismatch_bits(got, want[steps], ext, storage=storage)
                assert msg is None, f"{what} against the reference: {msg}"
                msg = ref.describe_mismatch_bits(got, context_run(wa, wo, m, dtype)[steps], ext, storage=storage)
                assert msg is None, f"{what} against its Context: {msg}"


@pytest.mark.parametrize("mixed", [False, True], ids=["one_shape", "mixed_shapes"])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_fp64_batch_of_both_forms_equals_the_oracle_and_its_contexts(wo, wa, ext, variant, mixed):
    """planned / unplanned / huge / tiny / planned-and-not-listed in one launch per step (variant 0) or per pass of K steps (1: K = 3
    ThreePoint, 2 FivePoint), after 1, 3 and 7 steps: every listed member bit for bit the oracle's and a Context's of its own Params
    and V, the member not listed keeps every bit, passes() counts the fused passes that ran"""
    run_ground(wa, wo, "f64", ext, variant, mixed)


@pytest.mark.parametrize("mixed", [False, True], ids=["one_shape", "mixed_shapes"])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("ext", [1, 2, 3])
@pytest.mark.parametrize("dtype", ["f32", "f32fast"])
def test_float_batch_of_both_forms_equals_the_models_and_its_contexts(wo, wa, dtype, ext, variant, mixed):
    """float storage: planned / unplanned on the base V and on V = inf, against the models of the context tests (f32: the C oracle
    rounding to float; f32fast: the all-float model that divides) and a Context each"""
    run_ground(wa, wo, dtype, ext, variant, mixed)


@pytest.mark.parametrize("mixed", [False, True], ids=["one_shape", "mixed_shapes"])
@pytest.mark.parametrize("gs", [0, 1])
@pytest.mark.parametrize("ext", [1, 2])
def test_batch_excited_steps_of_both_forms_equal_their_contexts(wo, wa, ext, gs, mixed):
    """evolve(5, wnum=2) under both gs variants: every listed member within the bar of
    tests/test_gpu_batch_states.py::test_batch_excited_evolve_matches_contexts of a Context of its own (1e-13 per cell, norm2 to
    1e-12), gs_steps() confirms the form; the tiny member's state is non-finite beyond fc.CAP on both sides (see
    test_excited_steps_in_the_full_forms) and the member not listed keeps every bit"""
    wnum, steps = 2, 5
    ms = member_list(wo, "f64", ext, mixed)
    stores = [list(orthonormal_store(wo, m["shape"], ext, wnum, seed=100 + 10 * k)) for k, m in enumerate(ms)]
    with make_batch(wa, wo, ms, "f64", mixed) as b:
        b.set_gs_variant(gs)
        for k in range(len(ms)):
            for i, l in enumerate(stores[k]):
                b.load_state(k, i, l)
        b.evolve(steps, active=fc.ACTIVE, wnum=wnum)
        assert b.gs_steps() == ((steps, 0) if gs == 1 else (0, steps)), b.gs_steps()
        n2 = b.norm2()
        for k, m in enumerate(ms):
            got = b.download_phi(k)
            if not m["listed"]:
                assert bits_differ(got, m["phi"]) == 0
                continue
            with member_context(wa, wo, m, "f64") as ctx:
                for i, l in enumerate(stores[k]):
                    ctx.load_state(i, l)
                ctx.upload_phi(np.array(m["phi"]))
                ctx.evolve(wnum, steps)
                assert ctx.x2_passes() == 0 or m["kind"] == "base" and not m["unplanned"], k
                want, want_n2 = ctx.download_phi(), ctx.norm2()
            if fc.non_finite_share(want, ext) > fc.CAP:
                assert m["kind"] == "tiny" and fc.non_finite_share(got, ext) > fc.CAP, k
                continue
            err = float(np.max(np.abs(got - want)))
            print("member", k, m["kind"] + (" unplanned" if m["unplanned"] else ""), "max|dphi|", err, "norm2", n2[k], "context", want_n2)
            assert err <= 1e-13, (k, err)
            assert n2[k] == pytest.approx(want_n2, rel=1e-12), k
            for l in stores[k]:
                assert abs(float(np.sum(l * got))) < 1e-13, k


@pytest.mark.parametrize("mixed", [False, True], ids=["one_shape", "mixed_shapes"])
@pytest.mark.parametrize("dtype,ext", [("f64", 1), ("f64", 2), ("f64", 3), ("f32", 1), ("f32", 2)])
def test_batch_evolve_states_of_both_forms_equals_contexts_started_there(wo, wa, dtype, ext, mixed):
    """evolve_states(n, [2, 3, 8, 1, 0]) -- the third member's eight states span two groups of states_per_workgroup = 4 -- for
    n = 3 and then 1 more: every stepped state bit for bit evolve(0, n) of a Context of the member's Params and V started there (any
    NaN equals any NaN); the states beyond k, phi and the member that steps nothing keep every bit"""
    ks, nst = [2, 3, 8, 1, 0], [3, 3, 8, 2, 1]
    storage = np.float64 if dtype == "f64" else np.float32
    ms = member_list(wo, dtype, ext, mixed)
    states = [rm.random_states(m["shape"], ext, nst[k], 700 + 17 * k + ext, frame=False, storage=storage) for k, m in enumerate(ms)]
    calls = [3, 1]
    want = {}
    for k, m in enumerate(ms):
        with member_context(wa, wo, m, dtype, max_states=8) as ctx:
            for j in range(ks[k]):
                ctx.upload_phi(states[k][j])
                per_call = []
                for n in calls:
                    ctx.evolve(0, n)
                    per_call.append(ctx.download_phi())
                want[k, j] = per_call
    with make_batch(wa, wo, ms, dtype, mixed, max_states=8) as b:
        d = b.store_dispatch()
        assert d["kernel"].startswith("wafer_k_batch_store_step<%d," % ext) and d["states_per_workgroup"] == 4, d
        assert ("WaferBatchGeomTable" in d["kernel"]) == mixed, d
        for k in range(len(ms)):
            for j, l in enumerate(states[k]):
                b.load_state(k, j, l)
        for c, n in enumerate(calls):
            b.evolve_states(n, ks)
            for k, m in enumerate(ms):
                for j in range(nst[k]):
                    got = b.download_state(k, j)
                    if j >= ks[k]:
                        assert bits_differ(got, states[k][j], storage) == 0, ("untouched", k, j, n)
                        continue
                    msg = ref.describe_mismatch_bits(got, want[k, j][c], ext, storage=storage)
                    assert msg is None, f"member {k} ({sid(m['shape'])}, {m['kind']}) state {j} after call {c}: {msg}"
                assert bits_differ(b.download_phi(k), m["phi"], storage) == 0, ("phi", k, n)
    if dtype == "f64":
        assert not np.isfinite(want[3, 0][0]).all()      # (the tiny member's states did meet its cell)


@pytest.mark.parametrize("mixed", [False, True], ids=["one_shape", "mixed_shapes"])
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_batch_sums_of_both_forms_are_their_contexts(wo, wa, ext, mixed):
    """observables() after three steps, ritz_matrices(3) and residuals(3, theta) per member, bit for bit the solo Context's (the
    contract those kernels state; any NaN equals any NaN) when m.short_forms differs between the members of one launch"""
    ms = member_list(wo, "f64", ext, mixed)
    states = [rm.random_states(m["shape"], ext, 3, 300 + 13 * k + ext, frame=False) for k, m in enumerate(ms)]
    theta = [np.full(3, FIXED) if m["listed"] else None for m in ms]
    with make_batch(wa, wo, ms, "f64", mixed) as b:
        b.evolve(3, active=fc.ACTIVE)
        phis = [b.download_phi(k) for k in range(len(ms))]
        obs = b.observables()
        for k in range(len(ms)):
            for j, l in enumerate(states[k]):
                b.load_state(k, j, l)
        mats = b.ritz_matrices(3, active=fc.ACTIVE)
        resid = b.residuals(3, theta=theta, active=fc.ACTIVE)
        assert mats[4] is None and resid[4] is None
        for k, m in enumerate(ms):
            with member_context(wa, wo, m, "f64") as ctx:
                ctx.upload_phi(phis[k])
                want = ctx.observables()
                for key in want:
                    assert bits_differ(obs[k][key], want[key]) == 0, (k, m["kind"], key, obs[k][key], want[key])
                if not m["listed"]:
                    continue
                for j, l in enumerate(states[k]):
                    ctx.load_state(j, l)
                h, s = ctx.ritz_matrices(3)
                r = ctx.residuals(3, theta=theta[k])
            assert bits_differ(mats[k][0], h) == 0 and bits_differ(mats[k][1], s) == 0, (k, m["kind"])
            for key in ("theta", "r2", "norm2"):
                assert bits_differ(resid[k][key], r[key]) == 0, (k, m["kind"], key, resid[k][key], r[key])
            if m["kind"] == "huge":
                assert np.isfinite(h).all() and np.abs(h).max() > 2.0 ** 590, (k, h)      # (the 2^609 cell is in the sums)
