"""compute_observables (grid.rs:303-445) read twice: the numpy reading of tests/observables_reading.py against the per-cell terms
of the C oracle (wo.observables_cells, the code wo.observables sums), bit for bit; and the oracle's sums against the exact sum of
those terms -- equal on integer-valued data, within the bound of recursive summation on random data.  No GPU."""
import math

import numpy as np
import pytest

from tests import observables_reading as rd
from tests.fp32_reference import denominator, stencil_sum

SHAPES = [(11, 8, 13), (33, 5, 7), (1, 1, 1)]
# the shapes tests/test_gpu_observables_exact.py uploads (one context f64 / f32, slabs)
GPU_SHAPES = [(129, 17, 5), (128, 16, 3), (257, 9, 4), (3, 2, 5), (1, 1, 1), (257, 17, 5), (256, 16, 3), (129, 17, 11)]
INPUTS = ["normal", "tiny", "huge", "boolean", "integer"]
DN, DT, MASS = 0.2, 0.004, 1.3


@pytest.fixture(scope="module")
def wo(oracle):
    return oracle


def in_frame(work, e):
    out = np.zeros(tuple(n + 2 * e for n in work.shape))
    out[e:-e, e:-e, e:-e] = work
    return out


def problem(wo, shape, ext, kind):
    """(cfg, phi, [V ...], pot_sub array) of one input kind"""
    rng = np.random.default_rng(100 * ext + SHAPES.index(shape) if shape in SHAPES else 5)
    if kind == "integer":
        case = rd.integer_case(shape, ext, seed=3)
        cfg = wo.Config(*shape, ext=ext, dn=case.dn, dt=DT, mass=case.mass)
        phi, own_v, potsub = case.phi, [case.v], case.potsub
    else:
        cfg = wo.Config(*shape, ext=ext, dn=DN, dt=DT, mass=MASS)
        if kind == "boolean":
            phi = wo.initial_condition(cfg, "Boolean")
        else:
            # 1e-140 and 1e140: w*w, v*w*w, w*S and w*w*r2 stay normal and finite (|S| < 3000 |w|, r2 < 1000, |V| < 100)
            scale = {"normal": 1.0, "tiny": 1e-140, "huge": 1e140}[kind]
            phi = in_frame(rng.standard_normal(shape) * scale, ext)
        own_v, potsub = [], rng.standard_normal(shape)
    vs = list(own_v)
    for pot in ("Harmonic", "Coulomb"):
        vs.append(wo.potential_generate(wo.Config(*shape, ext=ext, potential=pot, dn=cfg.dn, dt=DT, mass=cfg.mass)))
    vs.append(rng.standard_normal(cfg.padded_shape))
    return cfg, phi, vs, potsub


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_cells_equal_the_oracle_bit_for_bit(wo, ext, kind):
    for shape in SHAPES:
        cfg, phi, vs, potsub = problem(wo, shape, ext, kind)
        assert np.isfinite(phi).all()
        for v in vs:
            for form in ((0, 0.0, None), (1, 0.75, None), (2, 0.0, potsub)):
                got = rd.cells(cfg, v, phi, form)
                want = wo.observables_cells(cfg, v, phi, form)
                for k in rd.QUANTITIES:
                    if k == "v_infinity" and form[0] == 0:
                        assert isinstance(got[k], float) and got[k] == 0.0 and not want[k].any()
                        continue
                    assert np.isfinite(want[k]).all(), (shape, k)
                    assert got[k].shape == shape
                    assert np.array_equal(got[k], want[k]), (shape, form[0], k)
                    assert np.array_equal(np.signbit(got[k]), np.signbit(want[k])), (shape, form[0], k)
                if kind != "boolean" and shape != (1, 1, 1):
                    assert np.count_nonzero(want["energy"]) and np.count_nonzero(want["r2"])


@pytest.mark.parametrize("ext", [1, 2, 3])
def test_the_comparison_is_not_vacuous(wo, ext):
    """three other associations of the same formulas each differ from the oracle's cells somewhere on N(0, 1) data.
    (The r2 bracket cannot be told apart this way: dx*dx, dy*dy, dz*dz are quarter-integers below 2^53 and their sum is exact
    in any grouping, so nothing is asserted about it.)"""
    shape = SHAPES[0]
    cfg, phi, vs, potsub = problem(wo, shape, ext, "normal")
    v = vs[0]
    want = wo.observables_cells(cfg, v, phi, (2, 0.0, potsub))
    e = ext
    w, vv = phi[e:-e, e:-e, e:-e], v[e:-e, e:-e, e:-e]
    S, den = stencil_sum(phi, e), denominator(cfg)
    assert np.array_equal((vv * w) * w - (w * S) / den, want["energy"])
    assert np.count_nonzero(vv * (w * w) - (w * S) / den != want["energy"]) >= 1
    assert np.count_nonzero((vv * w) * w - w * (S / den) != want["energy"]) >= 1
    assert np.array_equal((w * w) * potsub, want["v_infinity"])
    assert np.count_nonzero(w * (w * potsub) != want["v_infinity"]) >= 1


@pytest.mark.parametrize("ext", [1, 2, 3])
def test_sums_are_exact_on_integer_data(wo, ext):
    for shape in GPU_SHAPES:
        for storage in ("f64", "f32"):
            case = rd.integer_case(shape, ext, seed=11 + GPU_SHAPES.index(shape), storage=storage)
            cfg = wo.Config(*shape, ext=ext, dn=case.dn, dt=DT, mass=case.mass)
            for form in rd.POTSUB_FORMS:
                got, want = wo.observables(cfg, case.v, case.phi, case.potsub_form(form)), case.sums(form)
                for k in rd.QUANTITIES:
                    assert got[k] == want[k], (shape, form, k)
                assert want["norm2"] > 0 or shape == (1, 1, 1)


def test_integer_case_is_what_the_issue_describes():
    for ext, q in ((1, 1.0), (2, 3.0), (3, 45.0)):
        case = rd.integer_case((9, 6, 7), ext, seed=1)
        assert denominator(case) == q and case.dn == 0.5 and case.potsub_scalar == 0.75
        k = case.phi[ext:-ext, ext:-ext, ext:-ext] / q
        assert np.array_equal(k, np.round(k)) and k.min() >= -8 and k.max() <= 8 and len(np.unique(k)) > 8
        assert np.array_equal(case.v, np.round(case.v)) and case.v.min() == -4 and case.v.max() == 4
        assert np.array_equal(case.potsub, np.round(case.potsub)) and case.potsub.min() == -5 and case.potsub.max() == 5
        frame = case.phi.copy()
        frame[ext:-ext, ext:-ext, ext:-ext] = 0
        assert not frame.any()
        for t in case.cells("array").values():       # all four terms are in fact integers or quarters, and not all zero
            assert t.any()
        assert np.array_equal(case.cells("array")["energy"], np.round(case.cells("array")["energy"]))


@pytest.mark.parametrize("ext", [1, 2, 3])
def test_sums_are_bounded_on_random_data(wo, ext):
    """|sum in any order - exact| <= (N - 1) u sum|t| with u = 2^-53 (recursive summation of N terms in any order and grouping,
    to first order in u).  The oracle adds in long double and rounds once, (N - 1) 2^-64 + 2^-53 relative to sum|t|, and fsum
    is the exact sum rounded once (2^-53 more): inside the bound for N >= 4; for N = 1 both are the term itself."""
    for shape in SHAPES:
        cfg, phi, vs, potsub = problem(wo, shape, ext, "normal")
        n = shape[0] * shape[1] * shape[2]
        for v in vs:
            for form in ((1, 0.75, None), (2, 0.0, potsub)):
                c = wo.observables_cells(cfg, v, phi, form)
                got, want = wo.observables(cfg, v, phi, form), rd.exact_sums(c)
                for k in rd.QUANTITIES:
                    bound = (n - 1) * 2.0 ** -53 * math.fsum(np.abs(c[k]).ravel().tolist())
                    assert abs(got[k] - want[k]) <= bound, (shape, k, got[k], want[k], bound)
