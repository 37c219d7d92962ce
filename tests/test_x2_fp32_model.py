"""CPU: tests/x2_fp32_model.py, the model tests/test_gpu_excited_fp32.py holds a float Context's excited-state steps to.

  * on storage float64 the model is the oracle's excited-state evolve (to 1e-14 per cell), so its pass plan and its algebra are
    the reference's; what float storage adds are roundings only;
  * every case of the GPU table is computed twice, with exact scalars and with every scalar moved by +-1e-12 relative: the
    model alone must reach the caps the GPU test applies (F_ref, the work cells in which the two runs differ, at most 0.25 % of
    them), or a legitimate GPU result could not either.  A case over the cap has fewer steps in the table, never a higher cap;
  * each of the model's mutations (a rounding point misread) must FAIL the GPU test's bar on at least one case of the table
    when the mutated model stands in for the GPU -- otherwise the bar would not tell that mistake from the code.

Measured here (60 cases x up to two calls; dn 0.3, dt 0.01, Coulomb / Cube, N(0, 1) starts): D_ref <= 1.5 u; F_ref <= 0.14 % of the
work cells after the first call and <= 0.24 % after the second; per shape the worst case is
    (150, 37, 29) 365 of 160 950   (128, 32, 20) 190 of 81 920   (260, 8, 40) 185 of 83 200   (24, 20, 28) 17 of 13 440   (3, 2, 5) 0 of 30.
With the engine's roundings misread, cells that differ from the model (share of the work cells, over the cases tried):
    sums_before_rounding 0.6 - 5.3 %, images_unrounded 0.09 - 1.2 %, x_rounded_between_passes / y1_rounded 22 - 54 % (by 1.5 - 3 u),
    one_rounding_at_the_end 25 - 26 %.  On storage float64 the model stays within 2.3e-16 of the oracle.  All five are distinguished (test_the_bar_tells_the_mutations_apart)."""
import numpy as np
import pytest

from tests import x2_fp32_model as xm

CAP = 0.0025


@pytest.fixture(scope="module")
def wo():
    from oracle import wafer_oracle
    wafer_oracle.build()
    return wafer_oracle


def sid(shape):
    return "x".join(map(str, shape))


# ---- 1. storage float64: the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("correlated", [False, True], ids=["orthonormal", "correlated"])
@pytest.mark.parametrize("k", xm.KS)
@pytest.mark.parametrize("shape", [(24, 20, 28), (3, 2, 5), (65, 33, 20)], ids=sid)
def test_on_float64_storage_the_model_is_the_oracle(wo, shape, k, correlated):
    """every step count of the GPU table and the second call from the materialised phi, against wo.evolve (grid.rs:562-686:
    step, norm, normalise, modified Gram-Schmidt after every step): 1e-14 per cell"""
    cfg, v, phi0 = xm.inputs(wo, shape, "Coulomb", storage=np.float64)
    lowers = xm.stored_states(cfg, k, correlated, storage=np.float64)
    a, b = wo.ab(cfg, v)
    model = xm.Model(cfg, v, lowers, np.float64)
    for steps in xm.STEPS:
        got, want = phi0, phi0.copy()
        for n in (steps, xm.SECOND):
            got = model.evolve(got, n)
            wo.evolve(cfg, k, a, b, want, lowers, n)
            err = float(np.max(np.abs(got - want)))
            print(shape, k, correlated, steps, n, "max |model - oracle|", err)
            assert err <= 1e-14, (steps, n, err)


def test_the_plan_is_the_planner_s():
    """wafer_x2_head and the pass count the GPU test asserts on Context.x2_passes()"""
    assert [xm.head_steps(n) for n in (4, 5, 6, 7, 12)] == [2, 3, 2, 3, 2]
    assert [xm.x2_passes(n) for n in (4, 5, 6, 7, 12)] == [1, 1, 2, 2, 5]
    assert all(xm.x2_passes(n) == (n - 2 - n % 2) // 2 for n in range(4, 40))
    for shape, k, steps in xm.CASES:
        first, second, _, _ = xm.case_of(shape, k, steps)
        assert 4 <= first <= steps and second in (0, 4, xm.SECOND), (shape, k, steps)
    for shape in xm.SHAPES:          # every shape and every k meets both stores and both potentials
        for k in xm.KS:
            seen = {xm.case_of(shape, k, steps)[2:] for steps in xm.STEPS}
            assert {c for c, _ in seen} == {False, True}
            assert {p for _, p in seen} == ({"Coulomb"} if min(shape) < 4 else {"Coulomb", "Cube"})


# ---- 2. the caps are reachable by the reference alone -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", xm.KS)
@pytest.mark.parametrize("shape", xm.SHAPES, ids=sid)
def test_the_caps_are_reachable_by_the_model_alone(wo, shape, k):
    for steps in xm.STEPS:
        cfg, _, _, _, calls = xm.case_models(wo, shape, k, steps)
        cells = cfg.nx * cfg.ny * cfg.nz
        for n, exact, perturbed in calls:
            u, d_ref, f_ref = xm.reference_figures(cfg, exact, perturbed, xm.tile_height(k))
            print(shape, "k", k, "case", steps, "call of", n, "steps: D_ref", d_ref, "F_ref", f_ref, "of", cells, "u", u)
            assert np.array_equal(exact, xm.store(exact, np.float32)) and np.all(np.isfinite(exact))
            assert f_ref["work"] <= CAP * cells, (steps, n, f_ref, cells)
            assert d_ref <= 2.0, (steps, n, d_ref)    # (a flipped rounding is one u; a cell next to flipped ones moves a fraction more)


def _one_step_tables(wo):
    for shape in xm.ONE_STEP_SHAPES:
        for ext, wnum, _ in xm.XF_CASES:
            cfg, _, out = xm.onepass_models(wo, shape, ext, wnum)
            for steps in xm.ONE_STEP_STEPS:
                yield ("transform on load", shape, ext, wnum, steps), cfg, out[steps]
    for shape in xm.ROWS_SHAPES:
        for ext, wnum, _, ab in xm.ROWS_CASES:
            cfg, _, _, _, out = xm.chain_models(wo, shape, ext, wnum, ab)
            for steps in xm.rows_steps(shape, ext, wnum):
                yield ("rows", shape, ext, wnum, steps), cfg, out[steps]
        for ext in (1, 2, 3):
            for wnum in xm.ORTHO_WNUM:
                cfg, _, _, _, out = xm.chain_models(wo, shape, ext, wnum)
                yield ("orthogonalise", shape, ext, wnum), cfg, out["orthogonalise"]


def test_the_caps_of_the_one_step_tables_are_reachable(wo):
    """the tables of the transform-on-load kernel, the kernel-per-projection path and orthogonalise alone: the same check"""
    n = 0
    for what, cfg, (exact, perturbed) in _one_step_tables(wo):
        cells = cfg.nx * cfg.ny * cfg.nz
        u, d_ref, f_ref = xm.reference_figures(cfg, exact, perturbed, 0)
        print(what, "D_ref", d_ref, "F_ref", f_ref, "of", cells)
        assert f_ref["work"] <= CAP * cells, (what, f_ref, cells)
        assert d_ref <= 2.0, (what, d_ref)
        n += 1
    assert n == 2 * len(xm.XF_CASES) * len(xm.ONE_STEP_SHAPES) + sum(
        len(xm.rows_steps(s, e, w)) for s in xm.ROWS_SHAPES for e, w, _, _ in xm.ROWS_CASES) + 9 * len(xm.ROWS_SHAPES)


# ---- 3. the bar tells the mistakes apart -------------------------------------------------------------------------------------------------
MUTATION_CASES = [((150, 37, 29), 1, 12), ((128, 32, 20), 2, 12), ((260, 8, 40), 3, 7), ((24, 20, 28), 3, 12), ((150, 37, 29), 3, 4)]


@pytest.mark.parametrize("mutation", xm.MUTATIONS)
def test_the_bar_tells_the_mutations_apart(wo, mutation):
    """the mutated model in the GPU's place, first call of a few cases of the table: the bar of tests/test_gpu_excited_fp32.py
    (xm.measure) must name a violation on at least one of them.  (The unmutated model passes it by construction: it IS the
    reference.)"""
    exposed = []
    for shape, k, steps in MUTATION_CASES:
        cfg, v, phi, lowers, calls = xm.case_models(wo, shape, k, steps)
        n, exact, perturbed = calls[0]
        got = xm.Model(cfg, v, lowers, np.float32, mutation=mutation).evolve(phi, n)
        fig, bad = xm.measure(got, cfg, exact, perturbed, xm.tile_height(k))
        cells = cfg.nx * cfg.ny * cfg.nz
        print(mutation, shape, k, steps, "err / u", fig["err"], "differ", fig["differ"], "of", cells, "F_ref", fig["f_ref"], "->", bad or "inside the bar")
        assert not xm.measure(exact, cfg, exact, perturbed, xm.tile_height(k))[1]
        if bad:
            exposed.append((shape, k, steps))
    assert exposed, f"{mutation}: no case of {MUTATION_CASES} is outside the bar -- list it in DESIGN.md section 3 as not distinguished"
