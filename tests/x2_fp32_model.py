"""A numpy model of Context.evolve(wnum, steps) on a storage type where the two-steps-per-pass kernel runs (ThreePoint, 1 <= wnum
<= 3, steps >= 4: wafer_engine_schedules.hip, x2_applies), shared by tests/test_x2_fp32_model.py (CPU) and
tests/test_gpu_excited_fp32.py (GPU).  Nothing here imports the engine.  The algebra is the one tests/test_two_step_regrouping.py
writes out in fp64; what this file adds is the pass plan and every point at which the kernels round to the storage type, each
taken from the code (the line it follows is named) and none from a result.  Every operation is an fp64 numpy operation (IEEE,
unfused -- the library is built with -ffp-contract=off) on values of the storage type; `A` is fp32_reference.step with a, b formed
in registers from the stored V (wafer_ab_from_v) and fp64 arithmetic.

Plan of one call (wafer_passes.h, wafer_next_pass):

  head     wafer_x2_head(steps) = 2 + (steps & 1) one-step passes of the transform-on-load kernel (WAFER_PASS_EXCITED, one_pass):
           step 1 under identity scalars (launch_excited: wafer_k_identity_scalars); every later one loads
               x = raw / norm - l_0 s_0 - l_1 s_1 ...        true division, unfused, storage order, ROUNDED TO STORAGE
           (wafer_stencil_lds.hip.h, xform_vec: `w[v] = (T)x`, T the storage type), norm = sqrt(sum raw^2) and
           s_j = t_j / norm - sum_{i<j} s_i G_ji from the previous step's sums (same file, the XF coefficients).  Each raw step
           result is stored, i.e. rounded to storage, and its sums sum raw^2, t_j = sum l_j raw are taken on the rounded values
           (same file: `res` is of type T before it is squared).
  images   M_j = A l_j rounded to storage (ensure_x2: wafer_entry_step_lds into c->mstates[j], an array of the storage type);
           <l_j, M_i> and G_ji = <l_j, l_i> are fp64 sums over the stored values (launch_dot).
  coeffs   wafer_k_x2_coeffs (wafer_stencil_x2.hip.h), kind 1 after the head, kind 2 after each pass: n = sqrt(sums[0]),
           W0 = 1 / n, SB = mgs(n, sum l_j Y1), t2_j = sum l_j Z / n - sum_i SB_i <l_j, M_i>, SC = mgs(1.0, t2).
  pass     x~ = Z W0 - M_0 SB_0 ... - l_0 SC_0 ...     wafer_x2_xform: reciprocal multiply, separate products and differences;
                                                     fp64, NOT rounded (the LDS tiles and z-queues of wafer_k_xstep2 are double)
           Y1 = A x~                                  fp64, NOT rounded (WaferUpdateKeep<T, T, ...> with T = double)
           Z  = A Y1                                  ROUNDED TO STORAGE (wafer_stencil_x2_iter.inc.h: as_stored(update_with(...)))
           sum Y1^2, sum l_j Y1 on the fp64 Y1; sum l_j Z on the ROUNDED Z (same file: zv = res2[r][v], after as_stored).
  final    u = Z W0 - M_0 SB_0 ...; sum u^2 on the unrounded u; (u - l_0 SC_0 ...) ROUNDED TO STORAGE (wafer_k_x2_apply:
           `rs[v] = (ST)r[v]`), then divided by sqrt(sum u^2) and ROUNDED TO STORAGE again (x2_run: launch_normalise,
           wafer_k_row_op<2>).

A second call starts a new head from the materialised phi.  Where a comment in the engine and its code disagree about a rounding
point, the code decides: the head of wafer_stencil_x2.hip.h says 128 x 8 tiles for two and three stored states, while
wafer_x2_ry(.., wide = true) gives float storage the 128 x 16 tile at every k (tile_height below).

Every scalar (the sums above, G, <l_j, M_i>) passes through `scalar(value)`: batch_fp32_model's `exact` for the model proper, its
`Perturbed` (+-1e-12 relative, the project's bar for sums) for the run that measures how far a differently partitioned sum can
move a float result.  `mutation` is one of MUTATIONS: a mistake the comparison has to notice."""
import functools
import math

import numpy as np

from tests import batch_fp32_model as chain
from tests import batch_onepass_model as onepass
from tests import fp32_reference as ref
from tests.batch_fp32_model import Perturbed, exact, spacing_u, work  # noqa: F401  (re-exported: the tests take them from here)

MUTATIONS = (
    "images_unrounded",            # M_j kept in fp64 (the transform and <l_j, M_i> read the unrounded images)
    "x_rounded_between_passes",    # x~ rounded to storage before the first step of a pass
    "y1_rounded",                  # Y1 rounded to storage (as if it left the CU)
    "sums_before_rounding",        # sum l_j Z taken on the fp64 Z
    "one_rounding_at_the_end",     # phi = storage((u - sum l_j SC_j) / n_c): one rounding where the code has two
)

# ---- the table both test files run ------------------------------------------------------------------------------------------------
DN, DT, MASS, SIG = 0.3, 0.01, 1.3, 0.4
SHAPES = [(150, 37, 29),   # ragged, crosses the x seam at 128
          (128, 32, 20),   # whole tiles: the XS instantiation
          (260, 8, 40),    # three x tiles, one row of tiles
          (24, 20, 28),    # smaller than a tile
          (3, 2, 5)]       # more cells than stored states, barely
KS = (1, 2, 3)
STEPS = (4, 5, 7, 12)      # both heads (2 and 3 one-step passes), one pass (4, 5) and several (7: two, 12: five)
SECOND = 6                 # the second call, from the materialised phi
CORRELATION = 0.4
# Cases whose model, against its perturbed self, differs in more than 0.25 % of the work cells (tests/test_x2_fp32_model.py asserts
# that cap on every case) get fewer steps, never a higher cap: {case: (steps of the first call, steps of the second; 0 = none)}.
# Measured with the full counts -- all four after the SECOND call, i.e. after 11 to 18 steps in all (a flipped cell moves its
# neighbours' next step by a fraction of an ulp, so flips breed): 0.32 %, 0.29 %, 0.46 % and 0.80 % of the cells.
FEWER_STEPS = {
    ((128, 32, 20), 3, 7): (7, 4),
    ((260, 8, 40), 2, 5): (4, 4),
    ((260, 8, 40), 3, 12): (10, 6),
    ((24, 20, 28), 2, 5): (5, 0),
}


def case_of(shape, k, steps):
    """(steps of the first call, steps of the second, correlated store?, potential): every shape and every k meets both stores
    and both potentials over the step counts (Cube's well can miss the work area of a grid of fewer than four cells along an
    axis: Coulomb there)"""
    i = SHAPES.index(shape) + STEPS.index(steps)
    pot = "Cube" if i % 2 else "Coulomb"
    if pot == "Cube" and min(shape) < 4:
        pot = "Coulomb"
    first, second = FEWER_STEPS.get((shape, k, steps), (steps, SECOND))
    return first, second, bool((i + k) // 2 % 2), pot


CASES = [(shape, k, steps) for shape in SHAPES for k in KS for steps in STEPS]


def _field(rng, cfg):
    e = cfg.ext
    w = np.zeros(cfg.padded_shape)
    w[e:-e, e:-e, e:-e] = rng.standard_normal(cfg.work_shape)
    return w


def store(x, storage):
    return np.ascontiguousarray(x.astype(storage).astype(np.float64))


def stored_states(cfg, k, correlated, storage=np.float32, seed=30):
    """k normalised states of the storage type: orthonormal (to the storage type's rounding), or each later one carrying
    CORRELATION times the first (overlaps of order one in every step)"""
    out = []
    for i in range(k):
        l = _field(np.random.default_rng([seed, i, cfg.nx, cfg.ny, cfg.nz]), cfg)
        if correlated and out:
            l = l / math.sqrt(float(np.sum(l * l))) + CORRELATION * out[0]
        else:
            for o in out:
                l = l - o * float(np.sum(o * l))
        out.append(store(l / math.sqrt(float(np.sum(l * l))), storage))
    return out


def inputs(wo, shape, potential, storage=np.float32, ext=1):
    """(cfg, stored V, start): the oracle's V and a N(0, 1) work area inside a zero frame, both rounded to storage"""
    cfg = wo.Config(*shape, ext=ext, potential=potential, dn=DN, dt=DT, mass=MASS, sig=SIG)
    return cfg, store(wo.potential_generate(cfg), storage), store(_field(np.random.default_rng([40, *shape]), cfg), storage)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def head_steps(steps):
    """wafer_passes.h: wafer_x2_head"""
    return 2 + (steps & 1)


def x2_passes(steps):
    return (steps - head_steps(steps)) // 2


def tile_height(k, ry=None):
    """rows of a tile of wafer_k_xstep2 on float storage: wafer_x2_ry(t, k, vg, wide = true) -- WAFER_X2_RY where it is 1 or 2,
    else 2 at every k"""
    return 8 * (ry if ry in (1, 2) else 2)


def _mgs(n, t, G):
    """wafer_k_x2_coeffs' mgs: s_j = t_j / n - sum_{i<j} s_i G_ji"""
    s = []
    for j, tj in enumerate(t):
        v = tj / n
        for i in range(j):
            v = v - s[i] * G[j][i]
        s.append(v)
    return s


def _xform(w, w0, sb, sc, lows, M, upto_u=False):
    """wafer_x2_xform: w * W0 - sum_j M_j SB_j (= u) - sum_j l_j SC_j"""
    x = w * w0
    for m, s in zip(M, sb):
        x = x - m * s
    if upto_u:
        return x
    for l, s in zip(lows, sc):
        x = x - l * s
    return x


class Model:
    """the constants of one (cfg, V, store): a, b, the Gram matrix, the images and <l_j, M_i>; evolve() is one call"""

    def __init__(self, cfg, v_stored, lowers, storage, scalar=exact, mutation=None):
        assert mutation is None or mutation in MUTATIONS, mutation
        assert cfg.ext == 1 and 1 <= len(lowers) <= 3
        self.cfg, self.lows, self.storage, self.scalar, self.mutation = cfg, lowers, storage, scalar, mutation
        self.a, self.b = ref.ab_of(v_stored, cfg.dt, np.float64, "registers")
        self.den = ref.denominator(cfg)
        k = len(lowers)
        dot = lambda x, y: scalar(float(np.sum(x * y)))   # noqa: E731
        self.G = [[dot(lowers[j], lowers[i]) for i in range(j)] for j in range(k)]
        self.M = [self.A(l, np.float64 if mutation == "images_unrounded" else storage) for l in lowers]
        self.amat = [[dot(lowers[j], self.M[i]) for i in range(k)] for j in range(k)]

    def A(self, x, storage):
        """one ground-state step in fp64 arithmetic, its result rounded to `storage`"""
        return ref.step(x, self.a, self.b, self.cfg.dt, self.den, 1, np.float64, storage)

    def evolve(self, phi, steps):
        """phi after Context.evolve(wnum, steps), steps >= 4; a new array"""
        assert steps >= 4, steps
        lows, M, st, scalar, mut = self.lows, self.M, self.storage, self.scalar, self.mutation
        dot = lambda x, y: scalar(float(np.sum(x * y)))   # noqa: E731
        # head: one-step passes, transform on load
        x, sums = phi, None
        for h in range(head_steps(steps)):
            if h:
                norm = math.sqrt(sums[0])
                x = raw / norm
                for l, s in zip(lows, _mgs(norm, sums[1:], self.G)):
                    x = x - l * s
                x = store(x, st)
            raw = self.A(x, st)
            sums = [dot(raw, raw)] + [dot(l, raw) for l in lows]
        # kind 1: the buffer holds a raw one-step result
        n = math.sqrt(sums[0])
        w0, sb, sc = 1.0 / n, [0.0] * len(lows), _mgs(n, sums[1:], self.G)
        buf = raw
        for _ in range(x2_passes(steps)):
            xt = _xform(buf, w0, sb, sc, lows, M)
            if mut == "x_rounded_between_passes":
                xt = store(xt, st)
            y1 = self.A(xt, st if mut == "y1_rounded" else np.float64)
            z = self.A(y1, st)
            zs = self.A(y1, np.float64) if mut == "sums_before_rounding" else z
            syy, sly, slz = dot(y1, y1), [dot(l, y1) for l in lows], [dot(l, zs) for l in lows]
            # kind 2
            n = math.sqrt(syy)
            sb = _mgs(n, sly, self.G)
            t2 = []
            for j in range(len(lows)):
                v = slz[j] / n
                for i in range(len(lows)):
                    v = v - sb[i] * self.amat[j][i]
                t2.append(v)
            sc = _mgs(1.0, t2, self.G)
            w0 = 1.0 / n
            buf = z
        # phi materialised
        u = _xform(buf, w0, sb, sc, lows, M, upto_u=True)
        su = dot(u, u)
        r = u
        for l, s in zip(lows, sc):
            r = r - l * s
        if mut != "one_rounding_at_the_end":
            r = store(r, st)
        return store(r / math.sqrt(su), st)


@functools.lru_cache(maxsize=None)
def case_models(wo, shape, k, steps):
    """a case of CASES on float storage -> (cfg, stored V, start, stored states, [(steps of the call, model with exact scalars,
    model with every scalar moved by +-1e-12 relative), ...]), one entry per call: each run continues from its OWN previous
    result, as the GPU does.  Computed once and shared; the arrays are not to be written."""
    first, second, correlated, potential = case_of(shape, k, steps)
    cfg, v, phi = inputs(wo, shape, potential)
    lowers = stored_states(cfg, k, correlated)
    me, mp = Model(cfg, v, lowers, np.float32), Model(cfg, v, lowers, np.float32, Perturbed(k))
    calls, e, p = [], phi, phi
    for n in (first, second):
        if n:
            e, p = me.evolve(e, n), mp.evolve(p, n)
            calls.append((n, e, p))
    return cfg, v, phi, lowers, calls


# ---- the one-step paths of a float Context: tables over models that exist (batch_onepass_model, batch_fp32_model) ---------------------
ONE_STEP_SHAPES = onepass.FLOAT_SHAPES + [(150, 37, 29)]
ONE_STEP_STEPS = onepass.FLOAT_STEPS                               # (1, 4)
# the transform-on-load kernel (XF): (ext, wnum, WAFER_X2) -- what never takes the two-step pass, or is kept from it
XF_CASES = [(2, 1, None), (2, 3, None), (2, 4, None), (3, 1, None), (3, 3, None), (3, 4, None), (1, 4, None), (1, 2, "0")]
# the kernel-per-projection path (launch_excited_rows): (ext, wnum, variant, a and b of fp32_reference.ab_of)
ROWS_SHAPES = chain.EXCITED_SHAPES
ROWS_CASES = [(ext, wnum, 0, "stored") for ext in (1, 2) for wnum in (1, 3)] + [(ext, 5, -1, "registers") for ext in (1, 2)]
ORTHO_WNUM = (1, 3, 5)
# the chain rounds after normalise and after every projection, so its flips breed faster: the cases whose model differs from its
# perturbed self in more than 0.25 % of the cells after 4 steps (1.7 %, 0.38 %, 0.52 %) end earlier -- {(shape, ext, wnum): last
# step count}; (33, 20, 11) with three states is over the cap after 2 steps already (0.30 %) and runs 1
ROWS_FEWER = {((33, 20, 11), 1, 3): 1, ((65, 33, 20), 1, 5): 3, ((65, 33, 20), 2, 5): 3}


def rows_steps(shape, ext, wnum):
    """the step counts (each from the start) a case of ROWS_CASES is compared after"""
    return tuple(sorted({1, ROWS_FEWER.get((shape, ext, wnum), ONE_STEP_STEPS[-1])}))


def member_of(ext, wnum):
    """which of batch_fp32_model.MEMBERS (dn, dt, mass, potential) a one-step case runs"""
    return (ext + wnum) % len(chain.MEMBERS)


def onepass_models(wo, shape, ext, wnum):
    """batch_onepass_model.float_models of the case's member: (cfg, stored states, {1: (exact, perturbed), 4: ...})"""
    return onepass.float_models(wo, member_of(ext, wnum), shape, ext, wnum)


@functools.lru_cache(maxsize=None)
def chain_models(wo, shape, ext, wnum, ab="registers"):
    """the chain model of batch_fp32_model on float storage -> (cfg, stored V, start, stored states, {"orthogonalise" | steps:
    (exact, perturbed)})"""
    m = member_of(ext, wnum)
    cfg, v, phi = chain.member_inputs(wo, m, shape, ext)
    lowers = chain.stored_states(cfg, m, wnum)
    out = {"orthogonalise": (chain.orthogonalise(phi, lowers, np.float32), chain.orthogonalise(phi, lowers, np.float32, Perturbed(m)))}
    for steps in rows_steps(shape, ext, wnum):
        out[steps] = (chain.excited_steps(cfg, v, phi, lowers, steps, np.float32, ab=ab),
                      chain.excited_steps(cfg, v, phi, lowers, steps, np.float32, Perturbed(m), ab=ab))
    return cfg, v, phi, lowers, out


# ---- the bar ------------------------------------------------------------------------------------------------------------------------
def outer_layer(cfg):
    """True on the outermost layer of the work area (work-shaped)"""
    m = np.ones(cfg.work_shape, dtype=bool)
    m[1:-1, 1:-1, 1:-1] = False
    return m


def seams(cfg, ty):
    """True on the work cells beside a tile seam: x = 127, 0 (mod 128), y = ty - 1, 0 (mod ty)"""
    x, y = np.arange(cfg.nx) % 128, np.arange(cfg.ny) % ty
    m = np.zeros(cfg.work_shape, dtype=bool)
    m[(x == 127) | (x == 0), :, :] = True
    m[:, (y == ty - 1) | (y == 0), :] = True
    return m


SUBSET_MIN = 1000


def subsets(cfg, ty):
    """{name: work-shaped mask}: the whole work area, and the outer layer / the seam cells where they hold >= SUBSET_MIN cells"""
    out = {"work": np.ones(cfg.work_shape, dtype=bool)}
    for name, m in (("outer", outer_layer(cfg)), ("seams", seams(cfg, ty) if ty else None)):
        if m is not None and int(m.sum()) >= SUBSET_MIN:
            out[name] = m
    return out


def reference_figures(cfg, model_exact, model_perturbed, ty):
    """(u, D_ref, {subset: F_ref}): the float spacing at max |phi|, the largest difference of the two model runs in units of it,
    and the number of cells of each subset in which they differ at all"""
    u = spacing_u(model_exact)
    d_ref = float(np.max(np.abs(model_exact - model_perturbed))) / u
    diff = work(cfg, model_exact) != work(cfg, model_perturbed)
    return u, d_ref, {name: int(np.count_nonzero(diff & m)) for name, m in subsets(cfg, ty).items()}


def cap(f_ref, cells):
    """the most cells of a subset of `cells` cells that may differ from the exact-scalar model"""
    return max(f_ref, -(-cells // 2000))


def measure(got, cfg, model_exact, model_perturbed, ty):
    """-> (figures, violations): figures = dict(u, d_ref, f_ref, err (max |got - model| / u), differ {subset: cells}); violations
    = the list of ways `got` misses the bar (empty: inside):
        the array holds values of the float type;
        max |got - model| <= max(1, 4 D_ref) u;
        per subset, the cells that differ from the exact-scalar model number at most max(F_ref, ceil(cells / 2000))."""
    u, d_ref, f_ref = reference_figures(cfg, model_exact, model_perturbed, ty)
    err = float(np.max(np.abs(got - model_exact))) / u
    diff = work(cfg, got) != work(cfg, model_exact)
    masks = subsets(cfg, ty)
    differ = {name: int(np.count_nonzero(diff & m)) for name, m in masks.items()}
    bad = []
    if not np.array_equal(got, ref.r32(got)):
        bad.append("not float values")
    if not err <= max(1.0, 4.0 * d_ref):
        bad.append(f"max error {err} u > max(1, 4 * {d_ref})")
    for name, m in masks.items():
        c = cap(f_ref[name], int(m.sum()))
        if differ[name] > c:
            bad.append(f"{differ[name]} cells of {name} ({int(m.sum())}) differ, cap {c}")
    return dict(u=u, d_ref=d_ref, f_ref=f_ref, err=err, differ=differ), bad
