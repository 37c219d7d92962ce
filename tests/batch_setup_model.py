"""The two questions the engine asks of a potential after every write of V (check_v_range, and wafer_k_batch_v_check for many members
at once), restated in numpy from a DOWNLOADED padded V -- float64 in the reference's [x][y][z] layout, the storage type's values
widened exactly.  One numpy operation per operation of the kernel's expression, so that the doubles are the same.

  range:  2^-400 < fabs(1. + dt * (double)v / 2.) < 2^400 on every cell, decided on the minimum and maximum of the BIT patterns
          (non-negative doubles order as their patterns; a NaN sorts above +inf, so one NaN makes the answer False).  The engine
          walks the whole allocation, whose cells outside the padded box hold 0, which gives 1: the model folds that 1 in.
  mirror: V[x, y, z] and V[x, ny-1-y, z] hold the same BITS on the work x and y of every padded plane (-0.0 is not 0.0; two NaNs
          with the same payload are equal)."""
import numpy as np

LOW, HIGH = 2.0 ** -400, 2.0 ** 400


def range_words(v: np.ndarray, dt: float):
    """(min, max) of the bit patterns of fabs(1. + dt * v / 2.) over v and one cell that holds 0, as Python ints"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        t = np.float64(dt) * v
        t = t / 2.0
        t = 1.0 + t
        x = np.abs(t)
    bits = np.concatenate([x.reshape(-1), np.abs(np.array([1.0 + np.float64(dt) * 0.0 / 2.0]))]).view(np.uint64)
    return int(bits.min()), int(bits.max())


def words_in_range(lo_word: int, hi_word: int) -> bool:
    """the engine's predicate on the two words: both bounds are exclusive, and a NaN in either makes it False"""
    lo, hi = (np.array([w], dtype=np.uint64).view(np.float64)[0] for w in (lo_word, hi_word))
    return bool(lo > LOW) and bool(hi < HIGH)


def in_range(v: np.ndarray, dt: float) -> bool:
    return words_in_range(*range_words(v, dt))


def y_symmetric(v: np.ndarray, ext: int) -> bool:
    """v: the padded array; the mirror on work x and y, every padded plane"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    work = np.ascontiguousarray(v[ext:v.shape[0] - ext, ext:v.shape[1] - ext, :])
    return bool(np.array_equal(work.view(np.uint64), np.ascontiguousarray(work[:, ::-1, :]).view(np.uint64)))


def stored(a: np.ndarray, dtype: str) -> np.ndarray:
    """what an array of the batch's storage type holds of these doubles, widened back"""
    if dtype == "f64":
        return np.asarray(a, dtype=np.float64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---- the adversarial sources of tests/test_gpu_batch_setup.py (about 6 x 5 x 4, resampled onto every member) -----------------------
SOURCE_SHAPE = (6, 5, 4)


def sources() -> dict:
    """name -> unpadded source.  "flat": one power of two everywhere -- every c0 * (1 - d) + c1 * d of the trilinear arithmetic is then
    that value exactly ((1 - d) + d rounds to 1), so V is finite and its own mirror image whatever the member's shape; "nan": the same
    with one NaN; "huge": with one 1e200 (dt * V / 2 beyond 2^400; +inf on float storage); "skew": random, so no mirror image.  The marked entries sit at (1, 1, 1): under the
    padded basis a member samples only the source's first (s - 1) (n - 1) / (p - 1) points per axis, 1.2 at the least here."""
    flat = np.full(SOURCE_SHAPE, -0.25)
    nan = flat.copy()
    nan[1, 1, 1] = np.nan
    huge = flat.copy()
    huge[1, 1, 1] = 1e200
    skew = np.random.default_rng(5).standard_normal(SOURCE_SHAPE)
    return dict(flat=flat, nan=nan, huge=huge, skew=skew)
