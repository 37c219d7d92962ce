"""tests/fp32_reference.py held to the CPU oracle, and the inputs of tests/test_gpu_fp32_reference.py held to the domain in which
that reference is one to the bit.  No GPU: the numpy step restates oracle/wafer_oracle.c:wo_stencil_step, and everything here
compares whole arrays with np.array_equal.  Second half: the inputs of tests/test_gpu_float_range.py, which leave the normal floats
on purpose -- the planned division's restatement held to wafer_divplan_qf and to the dividing model, conditions that each start
reaches what it is for, and the mistakes a bit comparison on those starts notices.  That half asks the library for the fp32 plan
(engine.div_plan_f32: host code, no GPU), so like tests/test_div_plan.py it needs the engine built (python -m wafer_amd.build)."""
import os
import subprocess

import numpy as np
import pytest

from oracle import wafer_oracle as wo
from tests import fp32_reference as ref

ALL_STEPS = list(range(1, max(ref.STEP_COUNTS) + 1))


@pytest.fixture(scope="module", autouse=True)
def built_oracle():
    wo.build()
    wo.set_threads(4)


def cases():
    return [pytest.param(shape, ext, id=f"{'x'.join(map(str, shape))}-ext{ext}") for ext in (1, 2, 3) for shape in ref.SHAPES]


@pytest.mark.parametrize("shape,ext", cases())
def test_the_numpy_step_in_float64_is_the_oracles_step(shape, ext):
    """arithmetic and storage float64: wo.ab's a, b and wo.evolve's phi, every bit, after every step count the GPU file runs"""
    cfg, v, phi = ref.case_inputs(wo, shape, ext)
    a, b = wo.ab(cfg, v)
    ma, mb = ref.ab_of(v, cfg.dt, np.float64, "registers")
    assert np.array_equal(ma, a) and np.array_equal(mb, b)
    got, _ = ref.evolve_numpy(cfg, v, phi, ref.STEP_COUNTS, np.float64, np.float64)
    want, done = phi.copy(), 0
    for count in ref.STEP_COUNTS:
        wo.evolve(cfg, 0, a, b, want, [], count - done)
        done = count
        assert ref.describe_mismatch(got[count], want, ext) is None, f"after {count} steps"


@pytest.mark.parametrize("shape,ext", cases())
def test_the_numpy_step_on_float_storage_is_the_oracles(shape, ext):
    """float storage, fp64 arithmetic, both readings of a, b: the numpy step equals evolve_zwindow(storage=float32) over the whole
    array -- with a, b from the stored V ("registers"), and with the oracle's a, b of the stored V rounded to float ("stored")"""
    cfg, v, phi = ref.case_inputs(wo, shape, ext)
    for ab in ("registers", "stored"):
        a, b = wo.ab_n(cfg.dt, v)
        if ab == "stored":
            a, b = ref.r32(a), ref.r32(b)
        ma, mb = ref.ab_of(v, cfg.dt, np.float64, ab)
        assert np.array_equal(ma, a) and np.array_equal(mb, b), ab
        got, _ = ref.evolve_numpy(cfg, v, phi, ref.STEP_COUNTS, np.float64, np.float32, ab)
        through_evolve, _ = ref.evolve(wo, cfg, v, phi, ref.STEP_COUNTS, "f32", ab)
        want = phi.copy()
        wo.evolve_zwindow(cfg, 0, a, b, want, max(ref.STEP_COUNTS), storage=np.float32)
        assert np.array_equal(through_evolve[max(ref.STEP_COUNTS)], want), ab
        for count in ref.STEP_COUNTS:
            assert ref.describe_mismatch(got[count], through_evolve[count], ext) is None, f"{ab}, after {count} steps"
            assert np.array_equal(got[count], ref.r32(got[count]))           # float values only


@pytest.mark.parametrize("shape,ext", cases())
def test_gpu_inputs_stay_in_the_domain_where_the_float_model_is_a_bit_level_reference(shape, ext):
    """a condition on the INPUTS of tests/test_gpu_fp32_reference.py, not a tolerance: over every step of every case, every
    non-zero numerator x of a float division x / den has a biased exponent in 27 ... 227 and |x / den| >= 2^-100 -- the range on
    which the planned fp32 division is checked against the IEEE division for every float (DESIGN.md section 3,
    test_planned_fp32_division_on_every_float) -- and no result is subnormal or infinite in float, for either dtype.  A case that
    breaks this needs another input, never a looser comparison."""
    cfg, v, phi = ref.case_inputs(wo, shape, ext)
    for ab in ("registers", "stored"):
        fast, div = ref.evolve_numpy(cfg, v, phi, ALL_STEPS, np.float32, np.float32, ab)
        assert div.x_max > 0.0 and div.q_max > 0.0, "the run divided nothing but zeros"
        assert 2.0 ** (27 - 127) <= div.x_min and div.x_max < 2.0 ** (228 - 127), (ab, div)
        assert 2.0 ** -100 <= div.q_min and div.q_max < 2.0 ** (228 - 127), (ab, div)
        wide, _ = ref.evolve(wo, cfg, v, phi, ALL_STEPS, "f32", ab)
        for run in (fast, wide):
            for count, state in run.items():
                nz = np.abs(state[state != 0])
                assert np.isfinite(state).all() and nz.size and nz.min() >= float(np.finfo(np.float32).tiny), (ab, count)


def changed(a, b, e):
    """fraction of the work cells whose bits differ"""
    work = tuple(slice(e, -e) for _ in range(3))
    return float(np.mean(a[work] != b[work]))


@pytest.mark.parametrize("shape,ext", [c for c in cases() if np.prod(c.values[0]) > 1])
def test_a_bit_comparison_notices_each_of_three_shared_mistakes(shape, ext):
    """The three mistakes that every kernel could share and that the tolerance bars (1e-5 of the energy, 2e-5 of the largest value)
    cannot see -- each moves a cell by a few 1e-7 of the largest value -- applied to the reference on the GPU file's inputs: each
    changes bits after one step and after three, on every shape with more than one work cell.
      a, b rounded to float before use (the round-3 bug)   changes an "f32" run
      w*a + q contracted into a fused multiply-add         changes an "f32fast" run
      x * (1/den) instead of x / den                       changes an "f32fast" run
    Fractions of the work cells changed, over the 24 shape x stencil cases (min ... max; after one step / after three):
      a, b rounded    1.5 ... 73 % / 3.8 ... 83 %
      fused           2.1 ... 47 % / 3.9 ... 64 %
      reciprocal      9.8 ... 18 % / 17 ... 41 %
    (the low ends of the first two are the Cube cases: outside the well V = 0 and a = b = 1 exactly, so nothing rounds there;
    Coulomb and SimpleCornell alone give 20 ... 73 % / 58 ... 83 % and 30 ... 47 % / 60 ... 64 %)"""
    cfg, v, phi = ref.case_inputs(wo, shape, ext)
    counts = [1, 3]
    for mutation, ar in (("ab_rounded", np.float64), ("fma", np.float32), ("reciprocal", np.float32)):
        clean, _ = ref.evolve_numpy(cfg, v, phi, counts, ar, np.float32)
        mutant, _ = ref.evolve_numpy(cfg, v, phi, counts, ar, np.float32, mutation=mutation)
        for count in counts:
            frac = changed(clean[count], mutant[count], ext)
            print(f"mutation {mutation} {shape} ext {ext} steps {count}: {frac:.4f} of the work cells change")
            assert frac > 0.0, (mutation, count)


# ---- outside the normal floats: the planned division, the starts of tests/test_gpu_float_range.py, and what they can tell apart ----
@pytest.mark.parametrize("shape,ext", cases())
def test_the_planned_division_changes_nothing_that_is_already_pinned(shape, ext):
    """the all-float model with division="planned" (the kernels' three instructions restated) equals the one that divides, whole
    arrays, on every in-domain case and both readings of a, b: the restatement may change nothing the GPU file already holds"""
    cfg, v, phi = ref.case_inputs(wo, shape, ext)
    for ab in ("registers", "stored"):
        ieee, _ = ref.evolve_numpy(cfg, v, phi, ref.STEP_COUNTS, np.float32, np.float32, ab)
        planned, _ = ref.evolve_numpy(cfg, v, phi, ref.STEP_COUNTS, np.float32, np.float32, ab, division="planned")
        for count in ref.STEP_COUNTS:
            assert np.array_equal(planned[count], ieee[count]), (ab, count)
            assert ref.describe_mismatch_bits(planned[count], ieee[count], ext) is None, (ab, count)


PLANNED_DENS = (2 * 0.05 ** 2, 2 * 0.02 ** 2 * 2.35, 24 * 0.2 ** 2 * 1.3, 360 * 0.01 ** 2 * 0.7, 2 * 0.2 ** 2, 3.0, 0.06)


def test_the_planned_restatement_is_wafer_divplan_qf_on_every_binade(tmp_path):
    """planned_fma (t = x * zl in float32, x * zh + t in float64, one rounding to float32) against wafer_divplan_qf compiled for
    the host -- the function the plan itself is checked with -- on 2000 random significands of every biased exponent 0 ... 254,
    both signs, and the ends of every binade: bit for bit, subnormal operands, subnormal and overflowing quotients included.
    Divisors: those of test_planned_fp32_division_on_every_float, and the three the step tests run with.  (Zero, infinite and
    NaN operands are v_div_fixup's on the device, which the host function does not have: planned_quotient gives them x / den.)"""
    from wafer_amd import engine
    exe = str(tmp_path / "divplan_qf")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", os.path.join(root, "tests", "divplan_qf_driver.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    rng = np.random.default_rng(17)
    per = 2000
    exps = np.repeat(np.arange(255, dtype=np.uint32), per + 2)
    mant = rng.integers(0, 1 << 23, exps.size, dtype=np.uint32).reshape(255, per + 2)
    mant[:, 0], mant[:, 1] = 0, (1 << 23) - 1
    mant[0, 0] = 1                                       # (exponent 0, significand 0 is zero: the smallest subnormal instead)
    bits = (exps << np.uint32(23)) | mant.ravel()
    x = np.concatenate([bits, bits | np.uint32(1 << 31)]).view(np.float32)
    assert np.isfinite(x).all() and np.all(x != 0) and np.count_nonzero(np.abs(x) < ref.F32_TINY) == 2 * (per + 2)
    x.tofile(str(tmp_path / "x.bin"))
    dens = PLANNED_DENS + tuple(c * ref.DN * ref.DN * ref.MASS for c in (2.0, 24.0, 360.0))
    for den in dens:
        plan = engine.div_plan_f32(den)
        assert plan.checked == 1, den
        zh, zl = np.float32(plan.zh), np.float32(plan.zl)
        out = str(tmp_path / "q.bin")
        r = subprocess.run([exe, str(tmp_path / "x.bin"), out] + ["%08x" % int(np.array([z]).view(np.uint32)[0]) for z in (zh, zl)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        want = np.fromfile(out, dtype=np.float32)
        got = ref.planned_fma(x, zh, zl)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), den
        assert np.array_equal(ref.planned_quotient(x, den).view(np.uint32), want.view(np.uint32)), den
        with np.errstate(all="ignore"):
            off = got != x / np.float32(den)
        low = np.abs(x) < np.float32(2.0 ** -100)
        print(f"den {den:.6g}: planned != IEEE on {np.mean(off[low]):.4%} of the operands below 2^-100, {int(off[~low].sum())} above")
    # the operand classes v_div_fixup owns: the quotient's sign and class are those of x / den
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], dtype=np.float32)
    for den in dens:
        with np.errstate(all="ignore"):
            assert ref.differing_bits(ref.planned_quotient(special, den), special / np.float32(den)).sum() == 0, den


RANGE_CASES = [(s, e) for e in (1, 2, 3) for s in ref.RANGE_SHAPES] + [(s, e) for e in (1, 2) for s in (ref.BATCH_ONE_SHAPE, (17, 17, 17))]
BIG_RANGE_CASES = [pytest.param(s, e, id=f"{'x'.join(map(str, s))}-ext{e}") for s, e in RANGE_CASES if np.prod(s) >= 1000]


def work(p, e):
    return p[e:-e, e:-e, e:-e]


def frame_is_plus_zero(p, e):
    frame = np.ones(p.shape, dtype=bool)
    work(frame, e)[...] = False
    return bool(np.all(p[frame] == 0.0) and not np.signbit(p[frame]).any())


def counts_of(shape):
    """the step counts tests/test_gpu_float_range.py runs a shape to (a shape only batches hold: the batches' counts)"""
    return ref.RANGE_STEP_COUNTS if shape in ref.RANGE_SHAPES else ref.BATCH_STEP_COUNTS


def range_runs(shape, ext, start):
    """{label: {count: phi}} of the references tests/test_gpu_float_range.py compares with, from the named start"""
    cfg, v = ref.range_case(wo, shape, ext)
    phi = ref.named_start(cfg, start)
    counts, runs = counts_of(shape), {}
    for ab in ("registers", "stored"):
        runs["f32-" + ab] = ref.evolve(wo, cfg, v, phi, counts, "f32", ab)[0]
        if start != "top":
            runs["f32fast-" + ab] = ref.evolve(wo, cfg, v, phi, counts, "f32fast", ab, division="planned")[0]
    return cfg, v, phi, runs


@pytest.mark.parametrize("shape,ext", BIG_RANGE_CASES)
def test_the_range_starts_reach_what_they_are_for(shape, ext):
    """conditions on the inputs of tests/test_gpu_float_range.py (never tolerances; a case that breaks one gets another seed or
    ramp), on every shape of at least 1000 cells, after every step count, for every reference that file compares with:
      low     at least 25 % of the work cells subnormal; every division of the f32fast run below 2^-100
      deep    at least 5 % subnormal, and a cell that is zero where the fp64 oracle's value is not (underflow happened)
      top     an inf or NaN cell, and at least half the work cells finite and non-zero (f32 only: f32fast is not run on it)
      seeded  NaN present and not everywhere after one step
    and the frame is +0.0 in every one of them."""
    sub = lambda p: np.mean((np.abs(work(p, ext)) < ref.F32_TINY) & (work(p, ext) != 0))
    for start in ref.STARTS:
        cfg, v, phi, runs = range_runs(shape, ext, start)
        assert frame_is_plus_zero(phi, ext)
        if start == "deep":
            a, b = ref.ab_of(v, cfg.dt, np.float64, "registers")
            exact, done, oracle = phi.copy(), 0, {}
            for count in counts_of(shape):
                wo.evolve(cfg, 0, np.ascontiguousarray(a), np.ascontiguousarray(b), exact, [], count - done)
                oracle[count], done = exact.copy(), count
        for label, run in runs.items():
            for count, p in run.items():
                assert frame_is_plus_zero(p, ext), (start, label, count)
                w = work(p, ext)
                line = (f"{start} {shape} ext {ext} {label} after {count}: subnormal {sub(p):.3f} zero {np.mean(w == 0):.3f} "
                        f"inf {int(np.isinf(w).sum())} nan {np.mean(np.isnan(w)):.4f}")
                if start == "low":
                    assert sub(p) >= 0.25, line
                elif start == "deep":
                    lost = int(np.count_nonzero((w == 0) & (work(oracle[count], ext) != 0)))
                    line += f" zero-where-fp64-is-not {lost}"
                    assert sub(p) >= 0.05 and lost >= 1, line
                elif start == "top":
                    assert np.count_nonzero(~np.isfinite(w)) >= 1 and np.mean(np.isfinite(w) & (w != 0)) >= 0.5, line
                else:
                    assert np.isnan(w).any() and (count > 1 or not np.isnan(w).all()), line
                print(line)
        if start == "low":
            for ab in ("registers", "stored"):
                _, div = ref.evolve_numpy(cfg, v, phi, [max(counts_of(shape))], np.float32, np.float32, ab, division="planned")
                assert 0.0 < div.x_max and div.q_max < 2.0 ** -100, (ab, div)


def share(a, b):
    """fraction of ALL cells, frame included, whose float bits differ (the sign of zero counts, NaN equals NaN)"""
    return float(np.mean(ref.differing_bits(a, b)))


@pytest.mark.parametrize("shape,ext", BIG_RANGE_CASES)
def test_a_bit_comparison_on_the_range_starts_notices_each_of_five_mistakes(shape, ext):
    """The mistakes the in-domain inputs cannot see, applied to the reference on the new starts: each changes bits after one step
    and after three, on every shape of at least 1000 cells.
      subnormal results flushed to zero by the store    low, deep (f32 and f32fast)
      subnormal phi read as zero                        low, deep (f32 and f32fast)
      overflow saturating to the largest float          top (f32)
      the frame formed as neighbour * 0                 seeded (f32 and f32fast): NaN and -0.0 in a frame that must stay +0.0
      IEEE division in place of the planned one         low (f32fast)
    The share of ALL cells (frame included) each one changes is printed.  Over the 13 cases, min ... max, after one step / three:
      flushing store   low 25 ... 53 % / 32 ... 65 %     deep 4.4 ... 13 % / 8.3 ... 17 %
      flushing load    low 29 ... 59 % / 33 ... 68 %     deep 7.5 ... 15 % / 8.7 ... 18 %
      saturating store 0.01 ... 0.14 % / 0.03 ... 0.62 %  (the cells that hold inf: on "top" every inf descends from the upload's
                       overflow -- no finite result of a step exceeds the largest float -- so "saturating" is an inf kept as the
                       largest float by the store; the double-to-float conversion itself is pinned at the upload, GPU file)
      frame by product 6.3 ... 24 % / 6.3 ... 28 %       (after one step the frame alone: -0.0 beside negative cells, NaN beside
                       NaN and inf)
      IEEE division    0.52 ... 1.4 % / 1.5 ... 3.4 %"""
    cfg, v = ref.range_case(wo, shape, ext)
    counts = [1, 3]
    table = [(m, s, ar) for m in ("flush_store", "flush_load") for s in ("low", "deep") for ar in (np.float64, np.float32)]
    table += [("saturate", "top", np.float64), ("frame_product", "seeded", np.float64), ("frame_product", "seeded", np.float32)]
    for mutation, start, ar in table:
        phi = ref.named_start(cfg, start)
        division = "planned" if ar is np.float32 else "ieee"
        clean, _ = ref.evolve_numpy(cfg, v, phi, counts, ar, np.float32, division=division)
        mutant, _ = ref.evolve_numpy(cfg, v, phi, counts, ar, np.float32, mutation=mutation, division=division)
        for count in counts:
            frac = share(clean[count], mutant[count])
            print(f"mutation {mutation} on {start} ({ar.__name__}) {shape} ext {ext} steps {count}: {frac:.4f} of the cells change")
            assert frac > 0.0, (mutation, start, ar, count)
            if mutation == "frame_product" and count == 1:        # the frame alone: the work cells of one step do not read it
                assert not frame_is_plus_zero(mutant[1], ext) and share(work(clean[1], ext), work(mutant[1], ext)) == 0.0
    phi = ref.named_start(cfg, "low")
    planned, _ = ref.evolve_numpy(cfg, v, phi, counts, np.float32, np.float32, division="planned")
    ieee, _ = ref.evolve_numpy(cfg, v, phi, counts, np.float32, np.float32, division="ieee")
    for count in counts:
        frac = share(planned[count], ieee[count])
        print(f"IEEE division for the planned one on low {shape} ext {ext} steps {count}: {frac:.4f} of the cells change")
        assert frac > 0.0, count


def test_a_bit_comparison_tells_zeros_and_nans_apart_the_way_it_says():
    """describe_mismatch_bits: -0.0 is not +0.0, any NaN is any NaN, a double that is no float matches nothing, and the report
    names the place"""
    a = np.zeros((5, 5, 5))
    a[2, 2, 2], a[1, 1, 1] = np.nan, 2.0 ** -149
    b = a.copy()
    b[2, 2, 2] = -np.nan
    assert ref.describe_mismatch_bits(a, b, 1) is None and ref.describe_mismatch_bits(a, b, 1, storage=np.float64) is None
    b[0, 3, 3] = -0.0
    assert np.array_equal(a, b, equal_nan=True)
    assert "1 of 125 cells differ; first at (0, 3, 3) (in the frame itself)" in ref.describe_mismatch_bits(a, b, 1)
    b[0, 3, 3], b[1, 1, 1] = 0.0, 0.0
    assert "(1, 1, 1) (next to the frame)" in ref.describe_mismatch_bits(a, b, 1)
    b[1, 1, 1] = 2.0 ** -149 * (1 + 2.0 ** -30)
    assert ref.describe_mismatch_bits(b, a, 1) is not None and ref.describe_mismatch_bits(b, b, 1) is not None
    assert ref.describe_mismatch_bits(b, b, 1, storage=np.float64) is None
