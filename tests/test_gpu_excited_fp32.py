"""The excited-state steps of a single Context on float storage (dtype "f32"; "f32fast" computes them in fp64 too) on the MI355X,
per cell against numpy models that say where every float rounding happens.

  * two steps per pass (wafer_k_xstep2 on the storage tag, the default for ThreePoint, k <= 3, >= 4 steps): tests/x2_fp32_model.py;
  * the transform-on-load kernel (FivePoint / SevenPoint, k = 4, WAFER_X2=0): tests/batch_onepass_model.py;
  * the kernel-per-projection path (variant 0, or more stored states than the fused overlaps carry) and orthogonalise alone: the
    chain of tests/batch_fp32_model.py.

The bar comes from the model alone (x2_fp32_model.measure).  The GPU's sums are partitioned differently from numpy's, so a scalar
can differ in its last bits and flip a float rounding in a rare cell.  Per case the model is computed twice, with exact scalars
and with every scalar moved by +-1e-12 relative (the project's bar for sums): D_ref is the largest difference of the two in
units of u (the float spacing at max |phi|), F_ref the number of work cells in which they differ at all.  Then
    the download holds float values;
    max |gpu - model| <= max(1, 4 D_ref) u;
    the work cells that differ from the exact-scalar model number at most max(F_ref, ceil(cells / 2000)),
and the last rule holds as well, with their own F_ref and size, on the outermost layer of the work area and on the cells beside
a tile seam (x = 127, 0 mod 128; y = TY - 1, 0 mod TY) wherever those hold 1000 cells -- a fault confined to tile edges cannot
hide in the overall share.  Why F_ref is a cap: the GPU's scalars differ from numpy's by fp64 rounding of another partition,
1e-16 .. 1e-15 relative, three to four orders below the perturbed run's 1e-12; the chance that a rounding boundary falls inside
a scalar's movement is proportional to that movement, so F_ref overstates what the GPU may do.  The floor of one cell in 2000
keeps a case with F_ref = 0 from failing on a single legitimate flip.  tests/test_x2_fp32_model.py (CPU) holds the model to the
oracle, asserts F_ref <= 0.25 % of the cells on every case of these tables (cases over it have fewer steps there) and shows that
each of the model's five mutations -- a rounding point misread -- falls outside this bar.

Measured on the CPU (the model against its perturbed self, 60 cases): D_ref <= 1.5; F_ref <= 0.14 % of the work cells after the
first call, <= 0.24 % after the second (365 of 160 950 at (150, 37, 29)); one-step tables: D_ref <= 0.75, F_ref <= 0.21 %.
Measured on the MI355X over the 223 comparisons of this file (135 of the two-step pass, 48 of the transform-on-load kernel, 22 of the
kernel-per-projection path, 18 of orthogonalise): no cell differs from the exact-scalar model in any of them (max error 0 u, 0 cells)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import batch_fp32_model as chain  # noqa: E402
from tests import fp32_reference as ref  # noqa: E402
from tests import x2_fp32_model as xm  # noqa: E402


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


def context(wa, wo, cfg, v, dtype="f32", lowers=(), variant=None, **kw):
    """a Context of `dtype` on cfg with the stored V and the stored states loaded"""
    par = wa.Params(cfg.nx, cfg.ny, cfg.nz, dn=cfg.dn, dt=cfg.dt, mass=cfg.mass, sig=cfg.sig, central_difference=cfg.ext, dtype=dtype, **kw)
    ctx = wa.Context(par)
    kind, scalar, arr = wo.potential_sub(cfg)
    ctx.set_potential_host(v, kind, scalar, arr)
    if variant is not None:
        ctx.set_stencil_variant(variant)
    for i, l in enumerate(lowers):
        ctx.load_state(i, l)
    return ctx


def tile_rows(d):
    """TY of the dispatch line's tile=128xTY (0: the kernel has no tile)"""
    return int(d["tile"].split("x")[1]) if "tile" in d else 0


def within(got, cfg, exact, perturbed, ty, what):
    fig, bad = xm.measure(got, cfg, exact, perturbed, ty)
    print(what, "D_ref", fig["d_ref"], "F_ref", fig["f_ref"], "u", fig["u"], "gpu max err / u", fig["err"], "gpu cells differing", fig["differ"],
          "of", cfg.nx * cfg.ny * cfg.nz)
    assert not bad, (what, bad)


def store_untouched(ctx, lowers):
    for i, l in enumerate(lowers):
        assert np.array_equal(ctx.download_state(i), l), i


def sid(shape):
    return "x".join(map(str, shape))


# ---- 1. two steps per pass ---------------------------------------------------------------------------------------------------------------
def run_x2_case(wa, wo, shape, k, steps, dtype, ry=None):
    """the calls of a case on a Context of `dtype`: [phi after each call]; asserts that wafer_k_xstep2 ran, pass by pass"""
    cfg, v, phi, lowers, calls = xm.case_models(wo, shape, k, steps)
    out = []
    with context(wa, wo, cfg, v, dtype, lowers) as ctx:
        d = ctx.dispatch(k)
        assert d["kernel"] == "wafer_k_xstep2" and d["dtype"] == dtype and d["v"] == "streamed", d
        assert tile_rows(d) == xm.tile_height(k, ry), d
        ctx.upload_phi(phi)
        passes = 0
        for n, _, _ in calls:
            ctx.evolve(k, n)
            passes += (n - 2 - n % 2) // 2
            assert ctx.x2_passes() == passes, "the two-step kernel did not run"
            out.append(ctx.download_phi())
        store_untouched(ctx, lowers)
    return out


def check_x2_case(wa, wo, shape, k, steps, ry=None, what=""):
    cfg, _, _, _, calls = xm.case_models(wo, shape, k, steps)
    got = run_x2_case(wa, wo, shape, k, steps, "f32", ry)
    for g, (n, exact, perturbed) in zip(got, calls):
        within(g, cfg, exact, perturbed, xm.tile_height(k, ry), f"x2 {shape} k={k} case {steps}{what}: call of {n} steps")
    return got


@pytest.mark.parametrize("steps", xm.STEPS)
@pytest.mark.parametrize("k", xm.KS)
@pytest.mark.parametrize("shape", xm.SHAPES, ids=sid)
def test_two_steps_per_pass_follow_the_model(wa, wo, shape, k, steps, monkeypatch):
    """evolve(k, steps) and a second evolve(k, 6) from the materialised phi (x2_fp32_model.case_of: the counts, the store --
    orthonormal or 0.4-correlated -- and the potential -- Coulomb or Cube, streamed -- of the case) against the model; then the
    same calls on dtype f32fast give f32's bits (excited steps compute in fp64 on both dtypes)."""
    monkeypatch.setenv("WAFER_X2_MAX_K", "3")
    got = check_x2_case(wa, wo, shape, k, steps)
    fast = run_x2_case(wa, wo, shape, k, steps, "f32fast")
    for g, f in zip(got, fast):
        msg = ref.describe_mismatch(f, g, 1)
        assert msg is None, f"f32fast against f32: {msg}"


@pytest.mark.parametrize("k", xm.KS)
@pytest.mark.parametrize("zchunk", ["1", "3"])
def test_two_steps_per_pass_under_every_z_chunking(wa, wo, zchunk, k, monkeypatch):
    """WAFER_ZCHUNK only repartitions the sums (the chunks overlap by a plane of Y1 on each side): the same bar.  (The default
    chunking is the table's own run above.)"""
    monkeypatch.setenv("WAFER_X2_MAX_K", "3")
    monkeypatch.setenv("WAFER_ZCHUNK", zchunk)
    check_x2_case(wa, wo, (150, 37, 29), k, 12, what=f" zchunk={zchunk}")


@pytest.mark.parametrize("ry", [1, 2])
def test_two_steps_per_pass_on_both_tile_heights(wa, wo, ry, monkeypatch):
    """WAFER_X2_RY = 1 (128 x 8 tiles) and 2 (128 x 16) at k = 1: the same bar, the seam cells those of the tile that ran"""
    monkeypatch.setenv("WAFER_X2_RY", str(ry))
    check_x2_case(wa, wo, (150, 37, 29), 1, 7, ry=ry, what=f" ry={ry}")


# ---- 2. the transform-on-load kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext,wnum,x2", xm.XF_CASES)
@pytest.mark.parametrize("shape", xm.ONE_STEP_SHAPES, ids=sid)
def test_transform_on_load_steps_follow_the_one_pass_model(wa, wo, shape, ext, wnum, x2, monkeypatch):
    """1 and 4 steps of the one-step excited kernel where it never takes the two-step pass (FivePoint, SevenPoint, four stored
    states) or is kept from it (WAFER_X2=0): the load transform rounds x to float into the LDS tile, so one pass per step
    performs the operations of batch_onepass_model (step, raw sums, one apply rounded once)"""
    if x2 is not None:
        monkeypatch.setenv("WAFER_X2", x2)
    cfg, lowers, out = xm.onepass_models(wo, shape, ext, wnum)
    _, v, phi = chain.member_inputs(wo, xm.member_of(ext, wnum), shape, ext)
    with context(wa, wo, cfg, v, "f32", lowers) as ctx:
        d = ctx.dispatch(wnum)
        assert d["kernel"] == "wafer_k_step_lds" and d["nlow"] == wnum and d["steps_per_pass"] == 1, d
        for steps in xm.ONE_STEP_STEPS:
            ctx.upload_phi(phi)
            ctx.evolve(wnum, steps)
            within(ctx.download_phi(), cfg, *out[steps], tile_rows(d), f"transform on load {shape} ext={ext} wnum={wnum}: {steps} steps")
        assert ctx.x2_passes() == 0
        store_untouched(ctx, lowers)


@pytest.mark.parametrize("wnum", [1, 3, 4])
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_one_pass_per_step_equals_two_on_float_storage(wa, wo, ext, wnum, monkeypatch):
    """WAFER_ONE_PASS=0 (every step materialises phi: step, sums, wafer_k_gs_apply) against the default (the next step
    normalises and projects on load) with WAFER_X2=0: both round x to float once per step, on the same operands -- identical
    bits, as test_one_pass_excited_step_equals_two_pass holds for fp64"""
    shape = (65, 33, 20)
    monkeypatch.setenv("WAFER_X2", "0")
    cfg, lowers, _ = xm.onepass_models(wo, shape, ext, wnum)
    _, v, phi = chain.member_inputs(wo, xm.member_of(ext, wnum), shape, ext)
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("WAFER_ONE_PASS", mode)
        with context(wa, wo, cfg, v, "f32", lowers) as ctx:
            ctx.upload_phi(phi)
            ctx.evolve(wnum, 7)
            ctx.evolve(wnum, 1)
            assert ctx.x2_passes() == 0
            out[mode] = (ctx.download_phi(), ctx.norm2())
    msg = ref.describe_mismatch(out["0"][0], out["1"][0], ext)
    assert msg is None, msg
    assert out["0"][1] == out["1"][1]


# ---- 3. the kernel-per-projection path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext,wnum,variant,ab", xm.ROWS_CASES)
@pytest.mark.parametrize("shape", xm.ROWS_SHAPES, ids=sid)
def test_kernel_per_projection_steps_follow_the_chain_model(wa, wo, shape, ext, wnum, variant, ab):
    """launch_excited_rows -- the direct kernel (variant 0: a, b streamed as the float arrays wafer_k_ab stored) or more stored
    states than the fused overlaps carry (wnum = 5) -- is step, normalise, then one projection per stored state, phi rounded to
    float after each: the chain of batch_fp32_model"""
    cfg, v, phi, lowers, out = xm.chain_models(wo, shape, ext, wnum, ab)
    with context(wa, wo, cfg, v, "f32", lowers, variant=None if variant < 0 else variant, max_states=max(4, wnum)) as ctx:
        d = ctx.dispatch(wnum)
        assert d["kernel"] == ("wafer_k_step_direct" if variant == 0 else "wafer_k_step_lds") and d["nlow"] == 0 and "then" in d, d
        for steps in xm.rows_steps(shape, ext, wnum):
            ctx.upload_phi(phi)
            ctx.evolve(wnum, steps)
            within(ctx.download_phi(), cfg, *out[steps], 0, f"rows {shape} ext={ext} wnum={wnum} variant={variant}: {steps} steps")
        assert ctx.x2_passes() == 0
        store_untouched(ctx, lowers)


@pytest.mark.parametrize("wnum", xm.ORTHO_WNUM)
@pytest.mark.parametrize("ext", [1, 2, 3])
@pytest.mark.parametrize("shape", xm.ROWS_SHAPES, ids=sid)
def test_orthogonalise_alone_follows_the_chain_model(wa, wo, shape, ext, wnum):
    """Context.orthogonalise(wnum) on float arrays: modified Gram-Schmidt in storage order, phi rounded to float after each
    projection; the store is read and never written"""
    cfg, v, phi, lowers, out = xm.chain_models(wo, shape, ext, wnum)
    with context(wa, wo, cfg, v, "f32", lowers, max_states=max(4, wnum)) as ctx:
        ctx.upload_phi(phi)
        ctx.orthogonalise(wnum)
        within(ctx.download_phi(), cfg, *out["orthogonalise"], 0, f"orthogonalise {shape} ext={ext} wnum={wnum}")
        store_untouched(ctx, lowers)
