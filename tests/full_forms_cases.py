"""Inputs that switch the step kernels' short arithmetic forms off (short_forms(c) false: the IEEE 1 / x for b and the extra
Markstein round, or x / den in fp32), shared by tests/test_full_forms_host.py (CPU: conditions on these inputs, on the oracle
alone) and tests/test_gpu_full_forms.py (GPU).  Every case starts from the algebraic potential ref.potential_of(shape, ext) and
the start of ref.case_inputs (tests/fp32_reference.py):

  unplanned    Params(unplanned_div=True), V unchanged: everything stays finite, the reference is the planned run's
  huge         fp64 only.  1 + dt V/2 = 2^600 at the centre work cell and -2^450 at the first work cell (the corner of tile 0):
               b = +-2^-600 there and a is -1 to the last place, so the run stays finite
  tiny         fp64 only.  V = (2^-500 - 1) 2 / dt at one cell: 1 + dt V/2 rounds to 0, b = inf -- a NaN front that grows by R
               cells per step, so the step counts stop at 7 (TINY_COUNTS) and the reference's non-finite share is capped (CAP)
  inf          float storage: V = inf at tiny's cell, the only way a float V leaves the range (b = 0, a = NaN): TINY_COUNTS too
  *_mirror     the base V made its own y-mirror on the bits and every altered cell (x, y, z) written at (x, ny-1-y, z) as well:
               the engine finds v_ysym = 1 and v_in_range = 0 together

The potentials are float64 arrays; "f64" keeps the oracle's doubles, "f32" rounds them to float (what a float context stores)."""
import functools

import numpy as np

from tests import fp32_reference as ref

SHAPES = ref.RANGE_SHAPES + [s for s in ref.WHOLE_TILES if s not in ref.RANGE_SHAPES]
COUNTS = ref.RANGE_STEP_COUNTS                 # unplanned, huge
TINY_COUNTS = [n for n in COUNTS if n <= 7]    # tiny, inf: 1, 2, 3, 7
CAP = 0.15                                     # the largest non-finite share of work cells a compared reference may have
KINDS = ("base", "huge", "tiny", "inf", "base_mirror", "huge_mirror", "tiny_mirror", "inf_mirror")
# the shapes and stencil orders of the excited-state / stored-state / sums tests: one ragged, one of whole tiles
STATE_SHAPES = [(65, 33, 20), (256, 32, 11)]


def counts_of(kind):
    return TINY_COUNTS if kind.startswith(("tiny", "inf")) else COUNTS


def work(p, e):
    return p[e:-e, e:-e, e:-e]


def huge_cells(work_shape):
    """[(work cell, 1 + dt V/2 there)] of "huge": the centre work cell and the first one"""
    nx, ny, nz = work_shape
    return [((nx // 2, ny // 2, nz // 2), 2.0 ** 600), ((0, 0, 0), -(2.0 ** 450))]


def tiny_cell(work_shape):
    """the one work cell of "tiny" and "inf": off the mirror line of a grid with more than two rows, away from huge's cells"""
    nx, ny, nz = work_shape
    return (nx // 3, ny // 3, nz // 2)


def altered_cells(kind, work_shape, dt):
    """[(work cell, V there)] of the kind, mirrored cells included"""
    name, _, mirror = kind.partition("_")
    if name == "huge":
        cells = [(c, (s - 1.0) * 2 / dt) for c, s in huge_cells(work_shape)]
    elif name == "tiny":
        cells = [(tiny_cell(work_shape), (2.0 ** -500 - 1.0) * 2 / dt)]
    elif name == "inf":
        cells = [(tiny_cell(work_shape), np.inf)]
    else:
        assert name == "base", kind
        cells = []
    if mirror:
        ny = work_shape[1]
        cells += [((x, ny - 1 - y, z), val) for (x, y, z), val in cells if ny - 1 - y != y]
    return cells


def y_mirrored(v, e):
    """v with the upper half of the work rows overwritten by the mirror image of the lower half, on every padded plane (the
    engine's question: V[x, y, z] and V[x, ny-1-y, z] hold the same bits on the work x and y)"""
    v = v.copy()
    w = v[e:-e, e:-e, :]
    ny = w.shape[1]
    for j in range(ny // 2):
        w[:, ny - 1 - j, :] = w[:, j, :]
    return v


@functools.lru_cache(maxsize=None)
def case(wo, shape, ext, kind="base", storage="f64"):
    """(cfg, V, start) of a case, both read-only.  storage "f64": the oracle's V in doubles; "f32": rounded to float"""
    assert kind in KINDS and storage in ("f64", "f32"), (kind, storage)
    assert storage == "f32" or not kind.startswith("inf")
    assert storage == "f64" or not kind.startswith(("huge", "tiny"))       # (on float storage those V are +-inf)
    # (a shape outside ref.SHAPES -- the one-shape batch's -- on SimpleCornell, as ref.range_case has it)
    cfg, v32, phi = ref.case_inputs(wo, shape, ext, None if shape in ref.SHAPES else "SimpleCornell")
    v = v32 if storage == "f32" else wo.potential_generate(cfg)
    if kind.endswith("_mirror"):
        v = y_mirrored(v, ext)
    else:
        v = v.copy()
    for cell, val in altered_cells(kind, cfg.work_shape, cfg.dt):
        work(v, ext)[cell] = val
    v.setflags(write=False)
    phi.setflags(write=False)
    return cfg, v, phi


def non_finite_share(p, e):
    return float(np.mean(~np.isfinite(work(p, e))))


def compared(out, e):
    """the step counts of a reference {steps: phi} at which it is compared: those whose non-finite share is within the cap"""
    return [n for n, p in out.items() if non_finite_share(p, e) <= CAP]


def shapes_of_row(shapes, spl):
    """the shapes a row of the float kernel table (tests/test_gpu_fp32_reference.py: KERNELS) is run on here: those of
    tests/test_gpu_float_range.py, and on the rows of the three-step kernel every grid of whole tiles as well"""
    out = list(ref.RANGE_SHAPES if shapes is ref.SHAPES else shapes)
    return out + [s for s in ref.WHOLE_TILES if spl == 3 and s not in out]


@functools.lru_cache(maxsize=None)
def oracle_f64(wo, shape, ext, kind):
    """{steps: phi} of wo.evolve on wo.ab(cfg, V) from the case's start, after each of counts_of(kind)"""
    cfg, v, phi = case(wo, shape, ext, kind)
    with np.errstate(all="ignore"):
        a, b = wo.ab(cfg, np.array(v))
        state, done, out = np.array(phi), 0, {}
        for steps in counts_of(kind):
            wo.evolve(cfg, 0, a, b, state, [], steps - done)
            out[steps], done = state.copy(), steps
    return out


@functools.lru_cache(maxsize=None)
def model_f32(wo, dtype, shape, ext, kind, ab, start="domain", division="ieee"):
    """{steps: phi} of ref.evolve on float storage ("f32": the C oracle rounding to float; "f32fast": the all-float model, dividing
    as `division` says) on the case's stored V, from the in-domain start or from the named start of ref.STARTS"""
    cfg, v, phi = case(wo, shape, ext, kind, "f32")
    if start != "domain":
        phi = ref.named_start(cfg, start)
    with np.errstate(all="ignore"):
        want, _ = ref.evolve(wo, cfg, np.array(v), np.array(phi), counts_of(kind), dtype, ab, division=division)
    return want


def start_of(wo, shape, ext, start):
    cfg, _, phi = case(wo, shape, ext, "base", "f32")
    return np.array(phi) if start == "domain" else ref.named_start(cfg, start)


# ---- batches: both forms in one launch ------------------------------------------------------------------------------------------------
# (kind, unplanned_div, listed) of the five members on fp64; float storage cannot hold "huge" and "tiny", so there the members are
# planned / unplanned on the base V and on V = inf
F64_MEMBERS = [("base", False, True), ("base", True, True), ("huge", False, True), ("tiny", False, True), ("base", False, False)]
F32_MEMBERS = [("base", False, True), ("base", True, True), ("inf", False, True), ("inf", True, True), ("base", False, False)]
SHORT_FORMS = [1, 0, 0, 0, 1]                  # what member_info reports for either list
BATCH_COUNTS = ref.BATCH_STEP_COUNTS           # 1, 3, 7: among COUNTS and TINY_COUNTS
ACTIVE = [1, 1, 1, 1, 0]


def batch_shapes(mixed):
    """the five members' shapes: (40, 24, 31) five times, or ref.BATCH_MIXED cycled (two shapes are shared by two members)"""
    return [ref.BATCH_MIXED[m % len(ref.BATCH_MIXED)] for m in range(5)] if mixed else [ref.BATCH_ONE_SHAPE] * 5
