"""The fp32-storage ("f32") and all-fp32 ("f32fast") ground-state step kernels against tests/fp32_reference.py, every cell's
bits over the whole downloaded array: every stencil order, every kernel variant and the kernel families the switches reach,
ragged grids / grids of whole 128 x 16 tiles / grids smaller than a tile, step counts with every remainder of the two- and
three-step passes.  tests/test_fp32_reference.py (CPU) holds the reference to the oracle and this file's inputs to the domain in
which the f32fast model is one to the bit.  Also on fp32 storage: the stored V / a / b arrays, the rounding of an upload, the
reductions (rel 1e-12, the project's bar for sums) and normalise (to the bit)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import fp32_reference as ref  # noqa: E402

REL_SUM = 1e-12   # every global sum
DTYPES = ["f32", "f32fast"]
OBSERVED = set()   # every kernel instance name a case saw after an evolve (printed when the module is done)


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
    print("\nkernel instances observed by tests/test_gpu_fp32_reference.py:")
    for name in sorted(OBSERVED):
        print("   ", name)


@functools.lru_cache(maxsize=None)
def reference(wo, dtype, shape, ext, ab):
    cfg, v, phi = ref.case_inputs(wo, shape, ext)
    want, _ = ref.evolve(wo, cfg, v, phi, ref.STEP_COUNTS, dtype, ab)
    return cfg, v, phi, want


def params(wa, cfg, dtype, **kw):
    return wa.Params(cfg.nx, cfg.ny, cfg.nz, dn=cfg.dn, dt=cfg.dt, mass=cfg.mass, sig=cfg.sig, central_difference=cfg.ext, dtype=dtype, **kw)


def instance_prefix(kernel, dtype):
    """the template-id a family that records its instance reports (wafer_stencil_kernel_instance); the others report the family name"""
    if kernel in ("wafer_k_step3_fused", "wafer_k_step2_wide"):
        return kernel + ("<wafer_f32_wide, double, " if dtype == "f32" else "<float, float, ")
    return kernel


# ---- ground-state steps -------------------------------------------------------------------------------------------------------
# (ext, variant, switches, the kernel that has to run, steps per pass, where its a, b come from, shapes)
F3 = {"WAFER_FUSE3_MIN_NY": "1"}     # the three-step kernel on grids below its size thresholds
SOME = [ref.RAGGED[0], ref.WHOLE_TILES[1], ref.SMALL[0]]
KERNELS = []
for _ext in (1, 2, 3):
    KERNELS += [(_ext, 0, {}, "wafer_k_step_direct", 1, "stored", ref.SHAPES),
                (_ext, 1, {}, "wafer_k_step_lds", 1, "registers", ref.SHAPES),
                (_ext, 1, {"WAFER_ABV": "0"}, "wafer_k_step_lds", 1, "stored", SOME)]
KERNELS += [
    # ThreePoint: two and three steps per pass; the default dispatch of a grid this small is the two-step kernel
    (1, 2, {}, "wafer_k_step2_fused", 2, "registers", ref.SHAPES),
    (1, 3, F3, "wafer_k_step3_fused", 3, "registers", ref.SHAPES),
    (1, -1, {}, "wafer_k_step2_fused", 2, "registers", ref.SHAPES),
    (1, 2, {"WAFER_ZCHUNK": "3"}, "wafer_k_step2_fused", 2, "registers", SOME),
    (1, 3, dict(F3, WAFER_ZCHUNK="1"), "wafer_k_step3_fused", 3, "registers", ref.WHOLE_TILES + [ref.RAGGED[2]]),
    (1, 3, dict(F3, WAFER_ZCHUNK="5"), "wafer_k_step3_fused", 3, "registers", ref.WHOLE_TILES + [ref.RAGGED[2]]),
    (1, 3, dict(F3, WAFER_F3_SCHED="1", WAFER_F3_PLAIN_DOWN="0"), "wafer_k_step3_fused", 3, "registers", ref.WHOLE_TILES + [ref.RAGGED[2]]),
    (1, 3, dict(F3, WAFER_F3_SCHED="0", WAFER_F3_PLAIN_DOWN="1"), "wafer_k_step3_fused", 3, "registers", ref.WHOLE_TILES + [ref.RAGGED[2]]),
    # FivePoint: the 128 x 16-tile two-step kernel (also the default) and the one with helper waves
    (2, 2, {}, "wafer_k_step2_wide", 2, "registers", ref.SHAPES),
    (2, 2, {"WAFER_F2_WIDE": "0"}, "wafer_k_step2_fused", 2, "registers", ref.SHAPES),
    (2, -1, {}, "wafer_k_step2_wide", 2, "registers", ref.SHAPES),
    (2, 2, {"WAFER_ZCHUNK": "3"}, "wafer_k_step2_wide", 2, "registers", SOME),
    # SevenPoint on fp32 storage has no multi-step kernel: the default is the LDS kernel
    (3, -1, {}, "wafer_k_step_lds", 1, "registers", ref.SHAPES),
]


def ground_cases():
    out = []
    for ext, variant, env, kernel, spl, ab, shapes in KERNELS:
        for shape in shapes:
            for dtype in DTYPES:
                switches = "".join(f"-{k[6:]}={v}" for k, v in env.items() if k != "WAFER_FUSE3_MIN_NY")
                out.append(pytest.param(dtype, ext, variant, env, kernel, spl, ab, shape,
                                        id=f"{dtype}-ext{ext}-v{variant}{switches}-{'x'.join(map(str, shape))}"))
    return out


@pytest.mark.parametrize("dtype,ext,variant,env,kernel,spl,ab,shape", ground_cases())
def test_ground_state_steps_equal_the_reference(wo, wa, monkeypatch, dtype, ext, variant, env, kernel, spl, ab, shape):
    """after 1, 2, 3, 7, 8 and 12 steps from the same uploaded start: np.array_equal on the whole array, and the case ran the
    kernel it names"""
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    cfg, v, phi, want = reference(wo, dtype, shape, ext, ab)
    with wa.Context(params(wa, cfg, dtype)) as ctx:
        ctx.set_stencil_variant(variant)
        ctx.set_potential(cfg.potential)
        assert ctx.stencil_kernel_name() == kernel and ctx.steps_per_launch() == spl
        assert ref.describe_mismatch(ctx.download_array("v"), v, ext) is None
        for steps in ref.STEP_COUNTS:
            ctx.upload_phi(phi)
            ctx.evolve(0, steps)
            got = ctx.download_phi()
            instance = ctx.stencil_kernel_instance()
            assert ctx.stencil_kernel_name() == kernel
            # (a family that records its template-id has one once a whole pass of it ran)
            assert instance.startswith(instance_prefix(kernel, dtype) if steps >= spl else kernel), instance
            OBSERVED.add(instance)
            msg = ref.describe_mismatch(got, want[steps], ext)
            assert msg is None, f"after {steps} steps of {instance}: {msg}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_comparison_tells_the_two_readings_of_a_b_apart(wo, wa, dtype):
    """a control of the comparison itself: one step of the direct kernel (stored a, b) is NOT the "registers" reference and one
    step of the LDS kernel (a, b from V) is NOT the "stored" one -- they differ by a, b's float rounding only, the size of
    mistake the equalities above exist to catch"""
    shape, ext = ref.RAGGED[0], 1
    for variant, other in ((0, "registers"), (1, "stored")):
        cfg, _, phi, want = reference(wo, dtype, shape, ext, other)
        with wa.Context(params(wa, cfg, dtype)) as ctx:
            ctx.set_stencil_variant(variant)
            ctx.set_potential(cfg.potential)
            ctx.upload_phi(phi)
            ctx.evolve(0, 1)
            assert ref.describe_mismatch(ctx.download_phi(), want[1], ext) is not None, variant


# ---- stored arrays ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("potential", ["Coulomb", "SimpleCornell", "Cube", "Harmonic", "ElipticalCoulomb"])
@pytest.mark.parametrize("shape,ext", [((65, 33, 20), 1), ((9, 12, 16), 2), ((17, 17, 17), 3)])
def test_stored_potential_arrays_are_the_oracles_rounded_to_float(wo, wa, dtype, potential, shape, ext):
    """V is (float) of the oracle's V; the a, b arrays (what variant 0 streams) are formed in fp64 from the STORED V and then
    rounded to float -- for both dtypes: wafer_k_ab computes in fp64 whatever the step kernels' arithmetic"""
    cfg, v, _ = ref.case_inputs(wo, shape, ext, potential)
    a, b = wo.ab_n(cfg.dt, v)
    with wa.Context(params(wa, cfg, dtype)) as ctx:
        ctx.set_potential(potential)
        for which, want in (("v", v), ("a", ref.r32(a)), ("b", ref.r32(b))):
            msg = ref.describe_mismatch(ctx.download_array(which), want, ext)
            assert msg is None, f"{which}: {msg}"
    ma, mb = ref.ab_of(v, cfg.dt, np.float64, "stored")
    assert np.array_equal(ma, ref.r32(a)) and np.array_equal(mb, ref.r32(b))     # ... which is the reference's "stored"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,ext", [((65, 33, 20), 1), ((3, 2, 5), 2), ((17, 17, 17), 3)])
def test_an_upload_rounds_to_nearest_even(wa, dtype, shape, ext):
    """upload_phi then download_phi is round-to-nearest-even of the fp64 input, frame cells included: random values over 60
    binades, and floats' midpoints (ties: the even neighbour), the doubles next to a midpoint on either side, both signs"""
    par = wa.Params(*shape, dn=ref.DN, dt=ref.DT, central_difference=ext, dtype=dtype)
    rng = np.random.default_rng(3)
    n = int(np.prod(par.padded_shape))
    phi = rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)
    f = np.abs(rng.standard_normal(n // 8)).astype(np.float32) * np.float32(2.0) ** rng.integers(-20, 20, n // 8).astype(np.float32)
    mid = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2.0      # exact in fp64
    ties = np.concatenate([mid, -mid, np.nextafter(mid, np.inf), -np.nextafter(mid, 0.0)])
    assert np.all(ref.r32(mid) != mid) and np.array_equal(ref.r32(-mid), -ref.r32(mid))
    k = min(ties.size, n)
    phi[:k] = ties[:k]
    phi = np.ascontiguousarray(rng.permutation(phi).reshape(par.padded_shape))
    with wa.Context(par) as ctx:
        ctx.upload_phi(phi)
        msg = ref.describe_mismatch(ctx.download_phi(), ref.r32(phi), ext)
    assert msg is None, msg


# ---- any start, any potential ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("potential", ["Periodic", "FullCornell"])
@pytest.mark.parametrize("ic", ["Gaussian", "Coulomb"])
@pytest.mark.parametrize("shape,ext", [((65, 33, 21), 1), ((41, 21, 13), 2), ((17, 17, 17), 3)])
def test_steps_from_the_devices_own_start_and_potential(wo, wa, dtype, potential, ic, shape, ext):
    """the start and V taken FROM the device (download_phi, download_array("v")), both sides evolved: bit exact also where V
    (Periodic, FullCornell) and the start (Gaussian, Coulomb) come from the device's libm.  Default dispatch, 7 steps."""
    cfg = wo.Config(*shape, ext=ext, potential=potential, dn=ref.DN, dt=ref.DT, mass=ref.MASS, sig=ref.SIG)
    with wa.Context(params(wa, cfg, dtype)) as ctx:
        ctx.set_potential(potential)
        ctx.set_initial_condition(ic, seed=5)
        v, phi = ctx.download_array("v"), ctx.download_phi()
        # conditions on the inputs: float values, finite, and (f32fast) quotients inside the planned division's checked range
        assert np.isfinite(v).all() and np.isfinite(phi).all() and phi.any()
        assert np.array_equal(v, ref.r32(v)) and np.array_equal(phi, ref.r32(phi))
        want, div = ref.evolve(wo, cfg, v, phi, [7], dtype)
        if div is not None:
            assert 2.0 ** -100 <= min(div.x_min, div.q_min) and max(div.x_max, div.q_max) < 2.0 ** 101, div
        ctx.evolve(0, 7)
        instance = ctx.stencil_kernel_instance()
        OBSERVED.add(instance)
        msg = ref.describe_mismatch(ctx.download_phi(), want[7], ext)
    assert msg is None, f"{instance}: {msg}"


# ---- reductions and element-wise operations on fp32 storage ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,ext", [((65, 33, 20), 1), ((150, 37, 29), 2), ((257, 20, 11), 3)])
def test_sums_over_float_arrays_match_the_oracle_on_the_same_values(wo, wa, dtype, shape, ext):
    """observables() and norm2() of a float state against the oracle ON THE DOWNLOADED ARRAYS (the sums are fp64 on both
    sides): rel 1e-12"""
    cfg, v, phi = ref.case_inputs(wo, shape, ext)
    with wa.Context(params(wa, cfg, dtype)) as ctx:
        ctx.set_potential(cfg.potential)
        ctx.upload_phi(phi)
        ctx.evolve(0, 3)
        state, stored_v = ctx.download_phi(), ctx.download_array("v")
        obs, n2 = ctx.observables(), ctx.norm2()
    want = wo.observables(cfg, stored_v, state, wo.potential_sub(cfg))
    for k in want:
        print(f"{dtype} ext {ext} {k}: got {obs[k]!r} want {want[k]!r}")
        assert obs[k] == pytest.approx(want[k], rel=REL_SUM, abs=0.0), k
    assert n2 == pytest.approx(wo.norm2(cfg, state), rel=REL_SUM, abs=0.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,ext", [((65, 33, 20), 1), ((150, 37, 29), 2), ((3, 2, 5), 3)])
def test_normalise_divides_in_fp64_and_rounds_to_float(wa, wo, dtype, shape, ext):
    """normalise(n2) with an explicit n2: (phi / sqrt(n2)) in fp64, rounded to float, every cell's bits"""
    cfg, _, phi = ref.case_inputs(wo, shape, ext)
    n2 = 7.25 * float(np.sum(phi * phi))
    with wa.Context(params(wa, cfg, dtype)) as ctx:
        ctx.upload_phi(phi)
        ctx.normalise(n2)
        msg = ref.describe_mismatch(ctx.download_phi(), ref.r32(phi / np.sqrt(n2)), ext)
    assert msg is None, msg
