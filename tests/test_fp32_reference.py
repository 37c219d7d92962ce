"""tests/fp32_reference.py held to the CPU oracle, and the inputs of tests/test_gpu_fp32_reference.py held to the domain in which
that reference is one to the bit.  No GPU: the numpy step restates oracle/wafer_oracle.c:wo_stencil_step, and everything here
compares whole arrays with np.array_equal."""
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
