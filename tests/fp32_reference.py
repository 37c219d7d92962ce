"""A bit-level reference of the ground-state step on fp32 storage (dtype "f32": float arrays, fp64 arithmetic) and in all-fp32
arithmetic (dtype "f32fast"), for tests/test_fp32_reference.py (CPU) and tests/test_gpu_fp32_reference.py (GPU).

One step is  phi' = w*a + b*dt*S/den  over the work area (grid.rs:568-664 as oracle/wafer_oracle.c:wo_stencil_step restates it:
the bracketed sum S in the reference's association, b*dt*S/den from left to right), the frame stays zero.  Three choices fix
every bit of it:

  arithmetic type  float64 for "f32", float32 for "f32fast".  In float32 EVERY operand (dt, den, V, a, b) and every product,
                   quotient and sum is a float (the kernels' C = float: wafer_stencil.hip.h, wafer_ab_from_v).
  storage type     the result of every step is rounded to it (float32 for both dtypes; float64 pins the model to wo.evolve).
  a, b             "registers": formed from the STORED (float) V in the arithmetic type -- wafer_ab_from_v, what the LDS kernel
                   and the two- and three-step kernels do (variants 1, 2, 3);
                   "stored": the float arrays wafer_k_ab writes -- formed in fp64 from the stored V, THEN rounded to float --
                   which variant 0 and any kernel run with WAFER_ABV=0 stream.

For "f32" the C oracle expresses both a, b choices (evolve_zwindow over the whole array with storage=float32), so evolve() below
calls it; the numpy step serves "f32fast", which the oracle cannot express, and the CPU tests that hold the numpy step to the
oracle.  numpy's elementwise float32 / float64 operations are the IEEE operations (no extended precision, no contraction).

The planned fp32 division of the f32fast kernels is the IEEE division for |x / den| >= 2^-100, so with
division="ieee" (the default) this model is a bit-level reference only on inputs whose quotients stay there: the model reports
the range it divided (Divided).  division="planned" restates the kernels' three instructions themselves (planned_quotient) and
is a reference over the whole float range: the starts below (ramp_start, seeded_start) leave the normal floats on purpose --
subnormals, underflow to zero, overflow to inf, NaN -- for tests/test_gpu_float_range.py."""
from dataclasses import dataclass

import numpy as np

# ---- the inputs both test files run (one table, so the CPU file checks the domain of exactly what the GPU file uploads) -------
DN, DT, MASS, SIG = 0.2, 0.004, 1.3, 0.3
RAGGED = [(65, 33, 20), (257, 20, 11), (150, 37, 29)]
WHOLE_TILES = [(128, 16, 5), (256, 32, 11), (128, 48, 23)]        # whole 128 x 16 tiles: exact store counts, ring queues
SMALL = [(3, 2, 5), (1, 1, 1), (17, 17, 17)]                      # smaller than a tile / degenerate
SHAPES = RAGGED + WHOLE_TILES + SMALL
STEP_COUNTS = [1, 2, 3, 7, 8, 12]                                 # every remainder of the two- and three-step passes
POTENTIALS = ["Coulomb", "SimpleCornell", "Cube"]                 # algebraic (+ - * / sqrt only): V itself is bit-comparable


def potential_of(shape, ext):
    """every shape meets every one of POTENTIALS over the three stencil orders (but a grid of fewer than four cells along an
    axis: the cube's well, padded indices n/4 < i <= 3n/4, can miss its work area, and V = 0 there leaves a = b = 1 exactly)"""
    pot = POTENTIALS[(SHAPES.index(shape) + ext - 1) % len(POTENTIALS)]
    return "Coulomb" if pot == "Cube" and min(shape) < 4 else pot


def r32(x):
    """what a float array holds of x (round to nearest even), as the float64 array the oracle and the engine's downloads use"""
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64))


def case_inputs(wo, shape, ext, potential=None):
    """(cfg, stored V, start) of a case: the oracle's V and a N(0, 1) work area inside a zero frame, both rounded to float"""
    cfg = wo.Config(*shape, ext=ext, potential=potential or potential_of(shape, ext), dn=DN, dt=DT, mass=MASS, sig=SIG)
    phi = np.zeros(cfg.padded_shape)
    rng = np.random.default_rng(1000 * ext + SHAPES.index(shape) if shape in SHAPES else 7)
    phi[ext:-ext, ext:-ext, ext:-ext] = rng.standard_normal(cfg.work_shape)
    return cfg, r32(wo.potential_generate(cfg)), r32(phi)


# ---- starts that leave the normal floats (tests/test_gpu_float_range.py; conditions on them: tests/test_fp32_reference.py) ------
RANGE_SHAPES = [(65, 33, 20), (256, 32, 11), (150, 37, 29), (3, 2, 5)]
RANGE_STEP_COUNTS = [1, 2, 3, 7, 12]
# name: (hi, lo) of ramp_start on a grid of at least 1000 cells, (hi, lo) on a smaller one (a steep ramp over a handful of
# cells is mixed away within a few steps), seed.  "low": every division below 2^-100, half the cells subnormal; "deep": the
# realistic tail, from 1 down through the subnormals to zero; "top": the upload overflows, the steps overflow further and then
# meet inf - inf.
RAMPS = {"low": ((-100, -160), (-128, -149), 11), "deep": ((0, -170), (-118, -152), 12), "top": ((128, 90), (128, 122), 13)}
STARTS = ("low", "deep", "top", "seeded")
BATCH_ONE_SHAPE = (40, 24, 31)                          # the one-shape batch's members: one start each
BATCH_MIXED = [(65, 33, 20), (17, 17, 17), (3, 2, 5)]   # the mixed-shape batch's members: all of them from one start
BATCH_STEP_COUNTS = [1, 3, 7]


def range_case(wo, shape, ext):
    """(cfg, stored V) of a float-range case: case_inputs' (a shape outside SHAPES on SimpleCornell)"""
    cfg, v, _ = case_inputs(wo, shape, ext, None if shape in SHAPES else "SimpleCornell")
    return cfg, v


def ramp_start(cfg, hi, lo, seed):
    """N(0, 1) * 2^(hi + (lo - hi) t), t = (i + j + k) / max(1, nx + ny + nz - 3) over the work indices, inside a zero frame,
    rounded to float with overflow (to inf) and underflow (to subnormals and zero) allowed"""
    e = cfg.ext
    nx, ny, nz = cfg.work_shape
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    t = (i + j + k) / max(1, nx + ny + nz - 3)
    phi = np.zeros(cfg.padded_shape)
    phi[e:-e, e:-e, e:-e] = np.random.default_rng(seed).standard_normal(cfg.work_shape) * 2.0 ** (hi + (lo - hi) * t)
    with np.errstate(over="ignore", under="ignore"):
        return r32(phi)


SPECIALS = (np.nan, np.inf, -np.inf, -0.0, 2.0 ** -149, -2.0 ** -149)


def seeded_positions(work_shape):
    """work positions of seeded_start's single cells, those the grid has: the eight corners (each next to the frame on three
    sides); (127, 15, z) and (128, 16, z), either side of an x seam and a y seam of the 128 x 16 tiles; x = 63 / 64, the batch
    kernels' 64-column tiles; z = 2 / 3 and z = 5 / 6, either side of the first two chunk boundaries under WAFER_ZCHUNK=3"""
    nx, ny, nz = work_shape
    pos = [(x, y, z) for x in (0, nx - 1) for y in (0, ny - 1) for z in (0, nz - 1)]
    pos += [(127, 15, nz // 2), (128, 16, nz // 2), (63, ny // 2, nz // 3), (64, ny // 2, nz // 3)]
    pos += [(nx // 3, ny // 3, z) for z in (2, 3)] + [((2 * nx) // 3, (2 * ny) // 3, z) for z in (5, 6)]
    out = []
    for p in pos:
        if all(0 <= c < n for c, n in zip(p, work_shape)) and p not in out:
            out.append(p)
    return out


def seeded_start(cfg, seed):
    """a N(0, 1) work area (as floats) with the cells of seeded_positions set to NaN, +inf, -inf, -0.0, 2^-149, -2^-149 in turn
    (the turn starts at `seed`, so two seeds put different values at a position), inside a zero frame"""
    e = cfg.ext
    phi = np.zeros(cfg.padded_shape)
    work = phi[e:-e, e:-e, e:-e]
    work[...] = np.random.default_rng(seed).standard_normal(cfg.work_shape)
    phi = r32(phi)
    work = phi[e:-e, e:-e, e:-e]
    for n, p in enumerate(seeded_positions(cfg.work_shape)):
        work[p] = SPECIALS[(n + seed) % len(SPECIALS)]
    return phi


def named_start(cfg, name, seed=None):
    """the start `name` of STARTS on cfg's grid"""
    if name == "seeded":
        return seeded_start(cfg, 14 if seed is None else seed)
    big, small, default_seed = RAMPS[name]
    hi, lo = big if int(np.prod(cfg.work_shape)) >= 1000 else small
    return ramp_start(cfg, hi, lo, default_seed if seed is None else seed)


# ---- the step -----------------------------------------------------------------------------------------------------------------
def _shifted(p, e, axis, d):
    """the work area of the padded array p, moved by d cells along axis"""
    sl = [slice(e, n - e) for n in p.shape]
    sl[axis] = slice(e + d, p.shape[axis] - e + d)
    return p[tuple(sl)]


def stencil_sum(p, e):
    """S of oracle/wafer_oracle.c:stencil_sum over the work area of p, term by term from left to right, in p's type"""
    ar = p.dtype.type
    w = _shifted(p, e, 0, 0)
    n = lambda axis, d: _shifted(p, e, axis, d)
    if e == 1:
        return n(0, 1) + n(0, -1) + n(1, 1) + n(1, -1) + n(2, 1) + n(2, -1) - ar(6) * w
    if e == 2:
        s = -n(0, 2) + ar(16) * n(0, 1) + ar(16) * n(0, -1) - n(0, -2)
        for axis in (1, 2):
            s = s - n(axis, 2) + ar(16) * n(axis, 1) + ar(16) * n(axis, -1) - n(axis, -2)
        return s - ar(90) * w
    s = None
    for axis in (0, 1, 2):
        lead = ar(2) * n(axis, 3)
        s = lead if s is None else s + lead
        s = s - ar(27) * n(axis, 2) + ar(270) * n(axis, 1) + ar(270) * n(axis, -1) - ar(27) * n(axis, -2) + ar(2) * n(axis, -3)
    return s - ar(1470) * w


def denominator(cfg):
    """grid.rs:569 / 594 / 626 in fp64 (the float kernels are handed (float) of it)"""
    return {1: 2., 2: 24., 3: 360.}[cfg.ext] * cfg.dn * cfg.dn * cfg.mass


def ab_of(v_stored, dt, ar, source):
    """a, b (potential.rs:101-110) over the whole padded array, as arrays of the arithmetic type `ar`"""
    if source == "registers":
        v, dt = v_stored.astype(ar), ar(dt)
        b = ar(1) / (ar(1) + dt * v / ar(2))
        return (ar(1) - dt * v / ar(2)) * b, b
    assert source == "stored", source
    b = 1. / (1. + dt * v_stored / 2.)
    a = (1. - dt * v_stored / 2.) * b
    return r32(a).astype(ar), r32(b).astype(ar)


@dataclass
class Divided:
    """the non-zero |x| and |x / den| of every division x / den a run performed (inf / 0 where it divided nothing but zeros)"""
    x_min: float = np.inf
    x_max: float = 0.0
    q_min: float = np.inf
    q_max: float = 0.0

    def add(self, x, q):
        # finite operands only: the range starts divide inf and NaN on purpose.  An in-domain case cannot hide one here --
        # test_gpu_inputs_stay_in_the_domain_... asserts np.isfinite of every state of every step, so x and q are finite there
        ax, aq = (np.abs(y[(y != 0) & np.isfinite(y)]).astype(np.float64) for y in (x, q))
        if ax.size:
            self.x_min, self.x_max = min(self.x_min, float(ax.min())), max(self.x_max, float(ax.max()))
        if aq.size:
            self.q_min, self.q_max = min(self.q_min, float(aq.min())), max(self.q_max, float(aq.max()))
        if np.count_nonzero(q) != np.count_nonzero(x):     # a non-zero x whose quotient underflowed to zero
            self.q_min = 0.0


MUTATIONS = ("ab_rounded", "fma", "reciprocal")
# ... and the mistakes that show only outside the normal floats (tests/test_fp32_reference.py names the start each one needs)
RANGE_MUTATIONS = ("flush_store", "flush_load", "saturate", "frame_product")
F32_TINY, F32_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)


def _plan_f32(den):
    """(zh, zl) of the fp32 plan of x / den the f32fast kernels run with (wafer_div_plan_f32: host code, no GPU)"""
    from wafer_amd import engine
    p = engine.div_plan_f32(float(den))
    assert p.checked == 1 and np.float32(p.den) == np.float32(den), (den, p.checked)
    return np.float32(p.zh), np.float32(p.zl)


def planned_quotient(x, den):
    """the f32fast kernels' x / den on a float32 array x (wafer_div_invariant<float>, wafer_divplan_qf):
    q = fmaf(x, zh, RN(x * zl)), restated as t = x * zl in float32, s = x * zh + t in float64, q = (float) s.  The float64 product
    is exact (two 24-bit significands), and so is the sum (the operands span at most 49 bits), so the one rounding is the
    fused multiply-add's -- subnormal and overflowing results included.  v_div_fixup then gives zero, infinite and NaN
    operands what x / den gives (the sign of a zero quotient is x's, whatever the sign of zl)."""
    with np.errstate(all="ignore"):
        return np.where((x == 0) | ~np.isfinite(x), x / np.float32(den), planned_fma(x, *_plan_f32(den)))


def planned_fma(x, zh, zl):
    """fmaf(x, zh, RN(x * zl)) alone, on float32 x, zh, zl: wafer_divplan_qf"""
    assert x.dtype == np.float32 and type(zh) is np.float32 and type(zl) is np.float32
    with np.errstate(all="ignore"):
        t = x * zl
        return (x.astype(np.float64) * np.float64(zh) + t.astype(np.float64)).astype(np.float32)


def _flushed(x):
    """x with its float-subnormal values replaced by zeros of their sign"""
    return np.where(np.abs(x) < F32_TINY, np.copysign(0.0, x), x).astype(x.dtype)


def step(phi, a, b, dt, den, e, ar, storage, divided=None, mutation=None, division="ieee"):
    """one step of the float64 array phi (holding values of the storage type): a new array of the same kind.  mutation: one of
    the three mistakes the comparison has to notice -- a, b rounded to float before use; w*a + q in ONE rounding (a fused
    multiply-add; float32 arithmetic only, formed through the exact float64 product); x * (1/den) for x / den -- or one of
    RANGE_MUTATIONS: subnormal results flushed to zero by the store; subnormal phi read as zero; a store that saturates (an
    infinite result kept as the largest finite value of the storage type); the frame formed as (the nearest work cell's result) * 0 in place of +0.
    division: "ieee" (x / den) or, in float32 arithmetic, "planned" (planned_quotient).  Overflow, underflow and invalid
    operations are part of the arithmetic here and raise nothing."""
    assert division in ("ieee", "planned"), division
    with np.errstate(all="ignore"):
        p = phi.astype(ar)
        if mutation == "flush_load":
            p = _flushed(p)
        w = _shifted(p, e, 0, 0)
        wa, wb = _shifted(a, e, 0, 0), _shifted(b, e, 0, 0)
        if mutation == "ab_rounded":
            wa, wb = wa.astype(np.float32).astype(ar), wb.astype(np.float32).astype(ar)
        x = wb * ar(dt) * stencil_sum(p, e)
        if division == "planned":
            assert ar is np.float32 and mutation != "reciprocal"
            q = planned_quotient(x, den)
        else:
            q = x * (ar(1) / ar(den)) if mutation == "reciprocal" else x / ar(den)
        if divided is not None:
            divided.add(x, q)
        if mutation == "fma":
            assert ar is np.float32
            r = (w.astype(np.float64) * wa.astype(np.float64) + q.astype(np.float64)).astype(np.float32)
        else:
            r = w * wa + q
        stored = r.astype(storage).astype(np.float64)
        if mutation == "flush_store":
            stored = _flushed(stored)
        if mutation == "saturate":
            stored = np.where(np.isinf(stored), np.copysign(float(np.finfo(storage).max), stored), stored)
        if mutation == "frame_product":
            mask = np.zeros(phi.shape)
            _shifted(mask, e, 0, 0)[...] = 1.0
            return np.pad(stored, e, mode="edge") * mask
        out = np.zeros(phi.shape)
        _shifted(out, e, 0, 0)[...] = stored
        return out


def evolve_numpy(cfg, v_stored, phi, counts, ar, storage, ab="registers", mutation=None, division="ieee"):
    """the numpy step from the start `phi` up to each of the (increasing) step counts: ({count: phi}, Divided)"""
    assert mutation is None or mutation in MUTATIONS + RANGE_MUTATIONS
    a, b = ab_of(v_stored, cfg.dt, ar, ab)
    den, divided, out, done = denominator(cfg), Divided(), {}, 0
    for count in counts:
        for _ in range(count - done):
            phi = step(phi, a, b, cfg.dt, den, cfg.ext, ar, storage, divided, mutation, division)
        out[count], done = phi, count
    return out, divided


def evolve(wo, cfg, v_stored, phi, counts, dtype, ab="registers", division="ieee"):
    """the reference of `dtype` ("f32" / "f32fast") from the start `phi` (float values) on the stored V, after each of the
    (increasing) step counts: ({count: phi}, Divided or None).  "f32" is the C oracle's with V and every step's result rounded
    to float (evolve_zwindow from padded plane 0 over the whole array; an overflowing result rounds to inf); "f32fast" the
    all-float numpy model, dividing as `division` says."""
    if dtype == "f32fast":
        return evolve_numpy(cfg, v_stored, phi, counts, np.float32, np.float32, ab, division=division)
    assert dtype == "f32" and division == "ieee", (dtype, division)
    a, b = (np.ascontiguousarray(x) for x in ab_of(v_stored, cfg.dt, np.float64, ab))
    phi, out, done = phi.copy(), {}, 0
    with np.errstate(all="ignore"):
        for count in counts:
            lo, hi = wo.evolve_zwindow(cfg, 0, a, b, phi, count - done, storage=np.float32)
            assert (lo, hi) == (0, phi.shape[2])
            out[count], done = phi.copy(), count
    return out, None


def frame_mask(shape, e):
    """True on the work cells that have a frame cell among their stencil neighbours"""
    m = np.zeros(shape, dtype=bool)
    for axis in range(3):
        sl = [slice(e, n - e) for n in shape]
        for side in (slice(e, 2 * e), slice(shape[axis] - 2 * e, shape[axis] - e)):
            sl[axis] = side
            m[tuple(sl)] = True
    return m


def describe_mismatch(got, want, e):
    """None where every cell's bits agree (np.array_equal); otherwise the count of differing cells, the first one's index, both
    values there, and whether that cell touches the frame"""
    if np.array_equal(got, want):
        return None
    return _report(~((got == want) | (np.isnan(got) & np.isnan(want))), got, want, e)


def _report(bad, got, want, e):
    """the report of describe_mismatch / describe_mismatch_bits on the cells marked in `bad` (at least one)"""
    idx = tuple(int(i) for i in np.argwhere(bad)[0])
    inside = all(e <= i < n - e for i, n in zip(idx, got.shape))
    where = "in the frame itself" if not inside else "next to the frame" if frame_mask(got.shape, e)[idx] else "in the interior"
    return (f"{int(bad.sum())} of {got.size} cells differ; first at {idx} ({where}): got {got[idx]!r} ({float(got[idx]).hex()}), "
            f"want {want[idx]!r} ({float(want[idx]).hex()})")


def differing_bits(got, want, storage=np.float32):
    """True on the cells whose bit patterns in the storage type differ: the sign of a zero counts, any NaN equals any NaN, and a
    value the storage type cannot hold (a download that is not made of floats) differs from everything"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    word = np.uint32 if storage is np.float32 else np.uint64
    with np.errstate(all="ignore"):
        g, w = got.astype(storage), want.astype(storage)
    held = (g.astype(np.float64) == got) | np.isnan(got)
    return ~(((g.view(word) == w.view(word)) | (np.isnan(g) & np.isnan(w))) & held)


def describe_mismatch_bits(got, want, e, storage=np.float32):
    """describe_mismatch on the bit patterns of the storage type (differing_bits): None, or the same report"""
    bad = differing_bits(got, want, storage)
    return _report(bad, got, want, e) if bad.any() else None
