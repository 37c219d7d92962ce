"""CPU side of tests/test_gpu_full_forms.py: conditions on the inputs of tests/full_forms_cases.py, on the oracle and the numpy
models alone (never tolerances: a case that breaks a condition is not compared at that count), the liveness of the unplanned
f32fast comparison, and the fp64 host statement of the division an unchecked divisor runs."""
import os
import subprocess
from fractions import Fraction as F

import numpy as np
import pytest

from oracle import wafer_oracle as wo
from tests import batch_setup_model as model
from tests import fp32_reference as ref
from tests import full_forms_cases as fc
from tests.test_div_plan import DENS_IN_USE, DENS_NEEDING_A_MOVED_ZL, exact_div, exact_q

wo.build()

CASES = [pytest.param(s, e, id=f"{'x'.join(map(str, s))}-ext{e}") for e in (1, 2, 3) for s in fc.SHAPES]
BIG = lambda shape: int(np.prod(shape)) >= 1000


@pytest.mark.parametrize("shape,ext", CASES)
def test_huge_stays_finite_and_tiny_stays_under_the_cap(shape, ext):
    """on wo.evolve alone, plain and mirrored: "huge" has no non-finite cell at any count; "tiny" has one from the first step on
    (so from step 3 on), and on a grid of at least 1000 cells stays under the cap through 3 steps at the least -- the counts the
    GPU file compares are those under the cap (fc.compared), printed here.  Shares of non-finite work cells after 1, 2, 3, 7 steps,
    plain / mirrored, largest over the shapes of at least 1000 cells: ext 1: 2.8 % / 4.8 %, ext 2: 9.4 % / 12.7 %, ext 3: 16.7 % /
    21.0 % (over the cap at 7 steps: (128, 16, 5) and, mirrored, (65, 33, 20) too, 19.9 %; every other case stays below 13 %)."""
    for mirror in ("", "_mirror"):
        for steps, p in fc.oracle_f64(wo, shape, ext, "huge" + mirror).items():
            assert np.isfinite(p).all(), (mirror, steps)
        out = fc.oracle_f64(wo, shape, ext, "tiny" + mirror)
        shares = {n: fc.non_finite_share(p, ext) for n, p in out.items()}
        print(f"tiny{mirror} {shape} ext {ext}: " + ", ".join(f"{n}: {s:.4%}" for n, s in shares.items()),
              "compared:", fc.compared(out, ext))
        assert all(s > 0.0 for s in shares.values()), shares
        assert set(fc.compared(out, ext)) >= ({1, 2, 3} if BIG(shape) else {1}), shares
        assert all(shares[n] <= fc.CAP for n in fc.compared(out, ext))


@pytest.mark.parametrize("shape,ext", CASES)
def test_an_infinite_float_potential_stays_under_the_cap(shape, ext):
    """float storage: V = inf at one cell (b = 0, a = NaN) under both float references, plain and mirrored, as above"""
    for mirror in ("", "_mirror"):
        for dtype in ("f32", "f32fast"):
            for ab in ("registers", "stored"):
                out = fc.model_f32(wo, dtype, shape, ext, "inf" + mirror, ab)
                shares = {n: fc.non_finite_share(p, ext) for n, p in out.items()}
                print(f"inf{mirror} {dtype} {ab} {shape} ext {ext}: " + ", ".join(f"{n}: {s:.4%}" for n, s in shares.items()))
                assert all(s > 0.0 for s in shares.values()), shares
                assert set(fc.compared(out, ext)) >= ({1, 2, 3} if BIG(shape) else {1}), shares


@pytest.mark.parametrize("shape,ext", CASES)
def test_the_engines_two_questions_have_the_answers_the_cases_are_for(shape, ext):
    """batch_setup_model (the restatement of check_v_range): out of range for huge, tiny and inf, in range for the base V; its own
    mirror image for every mirrored variant, and the plain ragged cases are not (or the mirrored ones would add nothing)"""
    for storage, kinds in (("f64", ("huge", "tiny")), ("f32", ("inf",))):
        cfg, v, _ = fc.case(wo, shape, ext, "base", storage)
        assert model.in_range(v, cfg.dt)
        cfg, vm, _ = fc.case(wo, shape, ext, "base_mirror", storage)
        assert model.in_range(vm, cfg.dt) and model.y_symmetric(vm, ext)
        for kind in kinds:
            cfg, v, _ = fc.case(wo, shape, ext, kind, storage)
            assert not model.in_range(v, cfg.dt), kind
            cfg, vm, _ = fc.case(wo, shape, ext, kind + "_mirror", storage)
            assert not model.in_range(vm, cfg.dt) and model.y_symmetric(vm, ext), kind
            if cfg.work_shape[1] > 2:
                assert not model.y_symmetric(v, ext), kind       # (one altered cell off the mirror line)


def test_the_batch_members_inputs():
    """the batches' own shapes: huge finite, tiny non-finite from the first step, both out of range"""
    for ext in (1, 2, 3):
        for shape in [ref.BATCH_ONE_SHAPE] + ref.BATCH_MIXED:
            cfg, v, _ = fc.case(wo, shape, ext, "base")
            assert model.in_range(v, cfg.dt)
            for kind in ("huge", "tiny"):
                cfg, v, _ = fc.case(wo, shape, ext, kind)
                assert not model.in_range(v, cfg.dt)
                out = fc.oracle_f64(wo, shape, ext, kind)
                shares = {n: fc.non_finite_share(p, ext) for n, p in out.items()}
                print(f"batch {kind} {shape} ext {ext}: " + ", ".join(f"{n}: {s:.4%}" for n, s in shares.items()))
                assert all((s == 0.0) if kind == "huge" else (s > 0.0) for s in shares.values())
                assert 1 in fc.compared(out, ext)
            cfg, v, _ = fc.case(wo, shape, ext, "inf", "f32")
            assert not model.in_range(v, cfg.dt)


def test_the_ieee_model_is_not_the_planned_one_on_low_for_every_row_of_the_table():
    """the unplanned f32fast kernels are compared with division="ieee" from "low" (every division below 2^-100), where the planned
    three instructions are NOT the quotient: for every row of the float kernel table, the two models differ in at least one cell of
    one of the row's shapes -- so that comparison tells which division the kernel ran"""
    from tests.test_gpu_fp32_reference import KERNELS
    seen = {}
    for ext, variant, env, kernel, spl, ab, shapes in KERNELS:
        total = 0
        for shape in fc.shapes_of_row(shapes, spl):
            key = (shape, ext, ab)
            if key not in seen:
                ieee = fc.model_f32(wo, "f32fast", shape, ext, "base", ab, "low", "ieee")
                planned = fc.model_f32(wo, "f32fast", shape, ext, "base", ab, "low", "planned")
                seen[key] = sum(int(ref.differing_bits(ieee[n], planned[n]).sum()) for n in fc.COUNTS)
                print(f"ieee against planned on low, {shape} ext {ext} {ab}: {seen[key]} cells over the counts")
            total += seen[key]
        assert total >= 1, (ext, variant, env)


def test_the_unchecked_fp64_division_is_the_quotient(tmp_path):
    """wafer_divplan_q_round (wafer_divplan.h: q = fma(x, zh, RN(x zl)), r = fma(-q, den, x), fma(r, zh, q)), compiled for the host,
    with the zl an UNCHECKED plan carries (RN(1/den - zh), never moved): the bits of x / den on the candidates
    tests/test_div_plan.py draws -- the significands nearest a rounding boundary, those a wrong zl fails among them -- in three
    binades and both signs, and on random operands, for the divisors in use, the ones whose first zl fails and the step tests'
    own.  The round has work to do: without it (exact_q) some of these operands miss the quotient."""
    from wafer_amd import engine
    exe = str(tmp_path / "divplan_round")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", os.path.join(root, "tests", "divplan_round_driver.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    hexd = lambda d: "%016x" % int(np.array([d], dtype=np.float64).view(np.uint64)[0])
    rng = np.random.default_rng(23)
    repaired = 0
    for den in DENS_IN_USE + DENS_NEEDING_A_MOVED_ZL + [c * ref.DN * ref.DN * ref.MASS for c in (2.0, 24.0, 360.0)]:
        plan, cand = engine.div_plan(den)
        zh = 1.0 / den
        assert plan.zh == zh
        e1 = (F(1) - F(zh) * F(den)) / F(den)
        zl = e1.numerator / e1.denominator                        # int / int: correctly rounded
        cand = np.asarray(cand, dtype=np.float64)
        x = np.concatenate([s * cand * 2.0 ** e for s in (1.0, -1.0) for e in (-52, -300, 250)]
                           + [rng.standard_normal(4096) * 2.0 ** rng.integers(-300, 300, 4096)])
        x.tofile(str(tmp_path / "x.bin"))
        out = str(tmp_path / "q.bin")
        r = subprocess.run([exe, str(tmp_path / "x.bin"), out, hexd(den), hexd(zh), hexd(zl)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        got = np.fromfile(out, dtype=np.float64)
        bad = ref.differing_bits(got, x / den, np.float64)
        assert not bad.any(), (den, int(bad.sum()), float(x[bad][0]))
        repaired += sum(exact_q(float(c), zh, zl) != exact_div(float(c), den) for c in cand)
    assert repaired > 0
