"""Float storage outside the normal floats: the step kernels of tests/test_gpu_fp32_reference.py's table, the element-wise and
set-up operations and the batches, on starts that are subnormal, underflow to zero, overflow to inf or carry NaN, +-inf, -0.0 and
+-2^-149 at the corners, tile seams and chunk boundaries (tests/fp32_reference.py: ramp_start, seeded_start).  Everything is an
equality of bit patterns over the whole padded array (describe_mismatch_bits: the sign of a zero counts, so the frame must be
+0.0; any NaN equals any NaN):

  f32      against the C oracle with V and every step's result rounded to float (gradual underflow, overflow to inf)
  f32fast  against the all-float model with the kernels' planned division restated (division="planned"), which is a reference
           below 2^-100 as well -- where the model that divides differs, measured by the control at the end of the step tests
  f64      the seeded start against wo.evolve: the NaN front after n steps is the oracle's, cell by cell

tests/test_fp32_reference.py (CPU) holds the planned restatement to wafer_divplan_qf, asserts that each start reaches what it is
for after every step count used here, and shows that a flushing store or load, a saturating store, a frame formed by a product
with 0 and the IEEE division each change bits on these starts."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import fp32_reference as ref  # noqa: E402
from tests.test_gpu_fp32_reference import F3, KERNELS, instance_prefix, params  # noqa: E402

REL_SUM = 1e-12   # every global sum
DTYPES = ["f32", "f32fast"]
COUNTS = ref.RANGE_STEP_COUNTS


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


def starts_of(dtype):
    """f32fast is not run on "top": its FivePoint and SevenPoint sums take 16 x and 2 x as ONE fused multiply-add
    (wafer_fma_pow2), which on purpose does not overflow where the reference's separate product does"""
    return [s for s in ref.STARTS if dtype == "f32" or s != "top"]


@functools.lru_cache(maxsize=None)
def start_of(wo, shape, ext, start):
    cfg, v = ref.range_case(wo, shape, ext)
    phi = ref.named_start(cfg, start)
    phi.setflags(write=False)
    return cfg, v, phi


@functools.lru_cache(maxsize=None)
def reference(wo, dtype, shape, ext, ab, start, division="planned"):
    """{steps: phi} from the named start, shared by every row that reads it"""
    cfg, v, phi = start_of(wo, shape, ext, start)
    want, _ = ref.evolve(wo, cfg, v, np.array(phi), COUNTS, dtype, ab, division=division if dtype == "f32fast" else "ieee")
    return want


def sid(shape):
    return "x".join(map(str, shape))


# ---- ground-state steps on float storage ------------------------------------------------------------------------------------------
def rows():
    out = []
    for row in KERNELS:
        ext, variant, env, kernel, spl, ab, shapes = row
        switches = "".join(f"-{k[6:]}={v}" for k, v in env.items() if k != "WAFER_FUSE3_MIN_NY")
        for shape in (ref.RANGE_SHAPES if shapes is ref.SHAPES else shapes):
            out.append(pytest.param(row, shape, id=f"ext{ext}-v{variant}{switches}-{sid(shape)}"))
    return out


def run_row(wo, wa, setenv, dtype, row, shape, starts, compare):
    """one row of the table on one shape: from each of `starts`, after each of COUNTS, compare(start, steps, instance, got)"""
    ext, variant, env, kernel, spl, ab, _ = row
    for k, val in env.items():
        setenv(k, val)
    cfg, v, _ = start_of(wo, shape, ext, "low")
    with wa.Context(params(wa, cfg, dtype)) as ctx:
        ctx.set_stencil_variant(variant)
        ctx.set_potential(cfg.potential)
        assert ctx.stencil_kernel_name() == kernel and ctx.steps_per_launch() == spl
        assert ref.describe_mismatch_bits(ctx.download_array("v"), v, ext) is None
        for start in starts:
            phi = start_of(wo, shape, ext, start)[2]
            for steps in COUNTS:
                ctx.upload_phi(np.array(phi))
                ctx.evolve(0, steps)
                got = ctx.download_phi()
                instance = ctx.stencil_kernel_instance()
                assert ctx.stencil_kernel_name() == kernel
                assert instance.startswith(instance_prefix(kernel, dtype) if steps >= spl else kernel), instance
                compare(start, steps, instance, got)


@pytest.mark.parametrize("row,shape", rows())
@pytest.mark.parametrize("dtype", DTYPES)
def test_steps_outside_the_normal_floats_equal_the_reference(wo, wa, monkeypatch, dtype, row, shape):
    """every row of the kernel table, from "low", "deep", "seeded" and (f32) "top", after 1, 2, 3, 7 and 12 steps from the same
    uploaded start: the bit patterns of the whole padded array, and the case ran the kernel it names"""
    ext, ab = row[0], row[5]

    def compare(start, steps, instance, got):
        msg = ref.describe_mismatch_bits(got, reference(wo, dtype, shape, ext, ab, start)[steps], ext)
        assert msg is None, f"{start} after {steps} steps of {instance}: {msg}"

    run_row(wo, wa, monkeypatch.setenv, dtype, row, shape, starts_of(dtype), compare)


@pytest.fixture(scope="module")
def low_ieee_shares(wo, wa):
    """{case id: {steps: share}}: the share of cells in which the model that DIVIDES differs from the f32fast kernel on "low",
    over the whole table (its own runs of the kernels: it depends on no other test)"""
    shares = {}
    for p in rows():
        row, shape = p.values
        ext, ab = row[0], row[5]

        def compare(start, steps, instance, got, case=shares.setdefault(p.id, {})):
            other = reference(wo, "f32fast", shape, ext, ab, start, "ieee")[steps]
            case[steps] = float(np.mean(ref.differing_bits(got, other)))

        with pytest.MonkeyPatch.context() as mp:
            run_row(wo, wa, mp.setenv, "f32fast", row, shape, ["low"], compare)
    return shares


def test_the_model_that_divides_is_not_the_f32fast_kernels_below_the_checked_range(low_ieee_shares):
    """the control of the f32fast comparison: on "low" every division is below 2^-100, and there the model with the IEEE division
    differs from the kernels in some case -- so the equalities above are live where the planned division is not the quotient.
    The share of differing cells is printed per case."""
    for case_id, shares in sorted(low_ieee_shares.items()):
        print(f"IEEE-division model against the kernel on low, {case_id}: " + ", ".join(f"{n}: {s:.4%}" for n, s in sorted(shares.items())))
    worst = max(max(s.values()) for s in low_ieee_shares.values())
    live = sum(1 for s in low_ieee_shares.values() if max(s.values()) > 0.0)
    print(f"{live} of {len(low_ieee_shares)} cases differ from the IEEE-division model; largest share of cells {worst:.4%}")
    assert live >= 1


# ---- fp64: the seeded start against the oracle -------------------------------------------------------------------------------------
# (ext, variant, the kernel that has to run, steps per pass): the names of the float table's rows, which fp64 shares
F64_ROWS = [(1, 0, "wafer_k_step_direct", 1), (1, 1, "wafer_k_step_lds", 1), (1, 2, "wafer_k_step2_fused", 2),
            (1, 3, "wafer_k_step3_fused", 3), (1, -1, "wafer_k_step2_fused", 2),
            (2, 0, "wafer_k_step_direct", 1), (2, 1, "wafer_k_step_lds", 1), (2, 2, "wafer_k_step2_wide", 2),
            (3, 0, "wafer_k_step_direct", 1), (3, 1, "wafer_k_step_lds", 1)]


@functools.lru_cache(maxsize=None)
def oracle_f64(wo, shape, ext):
    cfg, _, phi = start_of(wo, shape, ext, "seeded")
    v = wo.potential_generate(cfg)
    a, b = wo.ab(cfg, v)
    state, done, out = np.array(phi), 0, {}
    for steps in COUNTS:
        wo.evolve(cfg, 0, a, b, state, [], steps - done)
        out[steps], done = state.copy(), steps
    return cfg, v, out


@pytest.mark.parametrize("shape", ref.RANGE_SHAPES, ids=sid)
@pytest.mark.parametrize("ext,variant,kernel,spl", F64_ROWS)
def test_fp64_steps_carry_nan_inf_and_signed_zeros_as_the_oracle_does(wo, wa, monkeypatch, ext, variant, kernel, spl, shape):
    """dtype f64 from the seeded start (NaN, +-inf, -0.0, +-2^-149 at corners, seams and chunk boundaries), bit for bit against
    wo.evolve with any NaN equal to any NaN and the frame +0.0: the NaN front after n steps is the oracle's, cell by cell,
    through the fused passes' halos -- and the case ran the kernel it names"""
    if variant == 3:
        for k, val in F3.items():
            monkeypatch.setenv(k, val)
    cfg, v, want = oracle_f64(wo, shape, ext)
    phi = start_of(wo, shape, ext, "seeded")[2]
    with wa.Context(params(wa, cfg, "f64")) as ctx:
        ctx.set_stencil_variant(variant)
        ctx.set_potential(cfg.potential)
        assert ctx.stencil_kernel_name() == kernel and ctx.steps_per_launch() == spl
        assert ref.describe_mismatch_bits(ctx.download_array("v"), v, ext, storage=np.float64) is None
        for steps in COUNTS:
            ctx.upload_phi(np.array(phi))
            ctx.evolve(0, steps)
            instance = ctx.stencil_kernel_instance()
            assert ctx.stencil_kernel_name() == kernel and instance.startswith(kernel), instance
            msg = ref.describe_mismatch_bits(ctx.download_phi(), want[steps], ext, storage=np.float64)
            assert msg is None, f"after {steps} steps of {instance}: {msg}"


# ---- element-wise operations and set-up on float storage ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,ext", [((65, 33, 20), 1), ((3, 2, 5), 2), ((17, 17, 17), 3)])
def test_an_upload_rounds_to_nearest_even_at_both_ends_of_the_floats(wa, dtype, shape, ext):
    """upload_phi then download_phi at the ends of the float range, frame cells included, both signs: midpoints between
    neighbouring subnormals (ties: the even neighbour) and the doubles next to them; 2^-150, which goes to 0, and the doubles on
    either side (0 and 2^-149); the midpoint between the largest float and 2^128, which goes to inf, and the doubles on either
    side (the largest float and inf); random values of the subnormal binades"""
    par = wa.Params(*shape, dn=ref.DN, dt=ref.DT, central_difference=ext, dtype=dtype)
    rng = np.random.default_rng(4)
    n = int(np.prod(par.padded_shape))
    tiny, fmax = 2.0 ** -149, ref.F32_MAX
    k = rng.integers(0, 1 << 23, n // 8).astype(np.float64)
    mid = (k + 0.5) * tiny                                      # between the subnormals k and k + 1 (k = 0: 2^-150); exact in fp64
    over = (fmax + 2.0 ** 128) / 2.0                            # exact in fp64
    ends = np.array([tiny / 2.0, np.nextafter(tiny / 2.0, 0.0), np.nextafter(tiny / 2.0, 1.0), over, np.nextafter(over, 0.0),
                     np.nextafter(over, np.inf), fmax, tiny, ref.F32_TINY, np.nextafter(ref.F32_TINY, 0.0), 2.0 ** 128, 1e300, 1e-300])
    want_ends = np.array([0.0, 0.0, tiny, np.inf, fmax, np.inf, fmax, tiny, ref.F32_TINY, ref.F32_TINY, np.inf, np.inf, 0.0])
    with np.errstate(all="ignore"):
        assert np.array_equal(ref.r32(ends), want_ends) and np.all(ref.r32(mid) != mid)    # (what r32 itself does there)
    mids = np.concatenate([mid, np.nextafter(mid, np.inf), np.nextafter(mid, 0.0)])
    special = np.concatenate([ends, -ends, mids, -mids])
    phi = rng.standard_normal(n) * 2.0 ** rng.integers(-156, -120, n)
    m = min(special.size, n)
    phi[:m] = special[:m]
    assert m >= 2 * ends.size
    phi = np.ascontiguousarray(rng.permutation(phi).reshape(par.padded_shape))
    with np.errstate(all="ignore"):
        want = ref.r32(phi)
    with wa.Context(par) as ctx:
        ctx.upload_phi(phi)
        msg = ref.describe_mismatch_bits(ctx.download_phi(), want, ext)
    assert msg is None, msg


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,ext", [((65, 33, 20), 1), ((150, 37, 29), 2), ((3, 2, 5), 3)])
def test_normalise_rounds_into_the_subnormals(wa, wo, dtype, shape, ext):
    """normalise(4^20) of the "deep" start: (phi / 2^20) in fp64 rounded to float -- another 20 binades of the tail become
    subnormal or zero, each by one rounding"""
    cfg, _, phi = start_of(wo, shape, ext, "deep")
    n2 = 4.0 ** 20
    want = ref.r32(phi / np.sqrt(n2))
    assert np.count_nonzero(want != phi / np.sqrt(n2)) > 0          # the rounding is not the identity
    with wa.Context(params(wa, cfg, dtype)) as ctx:
        ctx.upload_phi(np.array(phi))
        ctx.normalise(n2)
        msg = ref.describe_mismatch_bits(ctx.download_phi(), want, ext)
    assert msg is None, msg


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("start", ["low", "deep"])
@pytest.mark.parametrize("shape,ext", [((65, 33, 20), 1), ((150, 37, 29), 2), ((256, 32, 11), 3)])
def test_sums_over_subnormal_states_match_the_oracle_on_the_same_values(wo, wa, dtype, start, shape, ext):
    """observables() and norm2() of the "low" and "deep" starts after three steps against the oracle ON THE DOWNLOADED ARRAYS:
    rel 1e-12, the project's bar for sums (a load that took subnormals for zero would lose all of "low"'s smallest terms)"""
    cfg, _, phi = start_of(wo, shape, ext, start)
    with wa.Context(params(wa, cfg, dtype)) as ctx:
        ctx.set_potential(cfg.potential)
        ctx.upload_phi(np.array(phi))
        ctx.evolve(0, 3)
        state, stored_v = ctx.download_phi(), ctx.download_array("v")
        obs, n2 = ctx.observables(), ctx.norm2()
    assert np.count_nonzero((np.abs(state) < ref.F32_TINY) & (state != 0)) > 0
    want = wo.observables(cfg, stored_v, state, wo.potential_sub(cfg))
    for k in want:
        print(f"{dtype} {start} ext {ext} {k}: got {obs[k]!r} want {want[k]!r}")
        assert obs[k] == pytest.approx(want[k], rel=REL_SUM, abs=0.0), k
    assert n2 == pytest.approx(wo.norm2(cfg, state), rel=REL_SUM, abs=0.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_resampled_upload_rounds_into_the_subnormals(wo, wa, dtype):
    """upload_phi_resampled of 9 x 7 x 11 sources onto (20, 13, 33) ext 1 and (9, 30, 12) ext 3: the oracle's trilinear resample
    (fp64) rounded to float, every bit, the frame +0.0.  Sources: the "deep" ramp, 1 down to 2^-170, and a ramp 2^-100 ... 2^-200
    -- the second target's work area samples the middle of the source only (the basis is the padded size) and meets the deep
    ramp's subnormal end nowhere; on the lower ramp both targets hold normal, subnormal and underflowed cells."""
    src_cfg = wo.Config(9, 7, 11, ext=1, potential="Coulomb", dn=ref.DN, dt=ref.DT)
    for ramp in (ref.RAMPS["deep"][0], (-100, -200)):
        src = np.ascontiguousarray(ref.ramp_start(src_cfg, *ramp, seed=15)[1:-1, 1:-1, 1:-1])
        for ext, shape in ((1, (20, 13, 33)), (3, (9, 30, 12))):
            want = np.zeros(tuple(s + 2 * ext for s in shape))
            exact = wo.trilerp_resize(src, shape, basis=want.shape)
            want[ext:-ext, ext:-ext, ext:-ext] = exact
            want = ref.r32(want)
            held = want[ext:-ext, ext:-ext, ext:-ext]
            small = np.abs(held) < ref.F32_TINY
            assert np.count_nonzero(~small) > 0
            if ramp[0] < 0:
                assert np.count_nonzero(small & (held != 0)) > 0 and np.count_nonzero((held == 0) & (exact != 0)) > 0
            with wa.Context(wa.Params(*shape, dn=ref.DN, dt=ref.DT, central_difference=ext, dtype=dtype)) as ctx:
                ctx.upload_phi_resampled(src)                          # basis = padded target size
                msg = ref.describe_mismatch_bits(ctx.download_phi(), want, ext)
            assert msg is None, f"{ramp} onto {shape}: {msg}"


# ---- batches -------------------------------------------------------------------------------------------------------------------------
CONTEXT_RUNS = {}   # (dtype, shape, ext, start) -> {steps: phi} of a Context under default dispatch, computed once


def host_inputs(wo, shape, ext):
    cfg, v = ref.range_case(wo, shape, ext)
    return cfg, v, wo.potential_sub(cfg)


def context_run(wo, wa, dtype, shape, ext, start):
    """{steps: phi} of a Context under default dispatch (a, b formed from the stored V) -- itself held to the reference here, since
    the step tests above do not run the batches' own shapes (40 x 24 x 31, 17 x 17 x 17)"""
    key = (dtype, shape, ext, start)
    if key not in CONTEXT_RUNS:
        cfg, v, potsub = host_inputs(wo, shape, ext)
        phi = start_of(wo, shape, ext, start)[2]
        want = reference(wo, dtype, shape, ext, "registers", start)
        out = {}
        with wa.Context(params(wa, cfg, dtype)) as ctx:
            ctx.set_potential_host(v, potsub[0], potsub[1], potsub[2])
            for steps in ref.BATCH_STEP_COUNTS:
                ctx.upload_phi(np.array(phi))
                ctx.evolve(0, steps)
                out[steps] = ctx.download_phi()
                msg = ref.describe_mismatch_bits(out[steps], want[steps], ext)
                assert msg is None, f"the Context on {sid(shape)} from {start} after {steps} steps: {msg}"
        CONTEXT_RUNS[key] = out
    return CONTEXT_RUNS[key]


def run_batch(wo, wa, dtype, ext, variant, members, mixed):
    """members: [(shape, start)]; every member against a Context of its own Params from the same start"""
    ins = [host_inputs(wo, shape, ext) for shape, _ in members]
    with wa.Batch([params(wa, cfg, dtype) for cfg, _, _ in ins], mixed_shapes=mixed) as b:
        b.set_step_variant(variant)
        for slot, (cfg, v, potsub) in enumerate(ins):
            b.set_potential_host(slot, v, potsub[0], potsub[1], potsub[2])
        assert b.steps_per_launch() == (1 if variant == 0 or ext == 3 else 3 if ext == 1 else 2)
        for steps in ref.BATCH_STEP_COUNTS:
            for slot, (shape, start) in enumerate(members):
                b.upload_phi(slot, np.array(start_of(wo, shape, ext, start)[2]))
            b.evolve(steps)
            for slot, (shape, start) in enumerate(members):
                want = context_run(wo, wa, dtype, shape, ext, start)[steps]
                msg = ref.describe_mismatch_bits(b.download_phi(slot), want, ext)
                assert msg is None, f"member {slot} ({sid(shape)}, {start}) after {steps} steps: {msg}"


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_shape_batch_members_equal_their_contexts(wo, wa, dtype, ext, variant):
    """a batch of 40 x 24 x 31 members, one per start ("low", "deep", "seeded" and, on f32, "top"), one step per launch (0) and
    fused passes (1), after 1, 3 and 7 steps: every member's bit patterns are those of a Context from the same start -- which the
    step tests above hold to the reference, so the batch kernels inherit it"""
    run_batch(wo, wa, dtype, ext, variant, [(ref.BATCH_ONE_SHAPE, s) for s in starts_of(dtype)], mixed=False)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("dtype,start", [(d, s) for d in DTYPES for s in starts_of(d)])
def test_mixed_shape_batch_members_equal_their_contexts(wo, wa, dtype, ext, variant, start):
    """(65, 33, 20) + (17, 17, 17) + (3, 2, 5) in one mixed-shape batch, all from the same named start: as above"""
    run_batch(wo, wa, dtype, ext, variant, [(shape, start) for shape in ref.BATCH_MIXED], mixed=True)
