"""compute_observables (grid.rs:303-445) on the device, exactly: wafer_k_step_lds<NLOW = -2> (one context, z-slabs) and
wafer_k_batch_observables (one-shape and mixed-shape batches) on the integer-valued inputs of tests/observables_reading.py, where
every per-cell term is a multiple of 1/4 and every partial sum in every order is exact (integer_case asserts it), against
math.fsum of the numpy reading's terms with ==.  No oracle call and no tolerance: a cell dropped or counted twice at a tile, chunk
or slab edge, an r2 from a neighbouring index or a pot_sub read one cell off changes an exact sum.

The shapes are the smallest at which the partition into tiles can go wrong -- the tile is 128 x 16 cells on doubles for Three- and
FivePoint, 128 x 8 for SevenPoint, twice as wide on float storage: one cell and one row more than a tile, one whole tile, two
tiles and a cell in x, less than a tile, one cell.  (The association of the integrand cannot show on such data; that is the CPU
file's part, tests/test_observables_reading.py.)"""
import dataclasses
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import observables_reading as rd  # noqa: E402
from tests.test_gpu_slab import run_slabs  # noqa: E402

DT = 0.004
F64_SHAPES = [(129, 17, 5), (128, 16, 3), (257, 9, 4), (3, 2, 5), (1, 1, 1)]
F32_SHAPES = [(257, 17, 5), (256, 16, 3), (3, 2, 5)]
# WAFER_ZCHUNK (planes per workgroup): unset, one plane, two -- with nz = 5 chunks of 2, 2, 1
CONTEXT_CASES = [(dtype, shape, zchunk)
                 for dtype, shapes in (("f64", F64_SHAPES), ("f32", F32_SHAPES))
                 for shape in shapes
                 for zchunk in ((None, "1", "2") if shape[2] >= 4 else (None,))]


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


def params_of(wa, case, dtype, **kw):
    return wa.Params(*case.shape, dn=case.dn, dt=DT, mass=case.mass, central_difference=case.ext, dtype=dtype, **kw)


def assert_exact(got, want, tag):
    for k in rd.QUANTITIES:
        assert got[k] == want[k], (tag, k, got[k], want[k])


def set_zchunk(monkeypatch, zchunk):
    if zchunk is None:
        monkeypatch.delenv("WAFER_ZCHUNK", raising=False)
    else:
        monkeypatch.setenv("WAFER_ZCHUNK", zchunk)


@pytest.mark.parametrize("ext", [1, 2, 3])
@pytest.mark.parametrize("dtype,shape,zchunk", CONTEXT_CASES)
def test_one_context(wa, monkeypatch, dtype, shape, zchunk, ext):
    set_zchunk(monkeypatch, zchunk)
    case = rd.integer_case(shape, ext, seed=17 * ext + len(shape) + shape[0], storage=dtype)
    with wa.Context(params_of(wa, case, dtype)) as ctx:
        for form in rd.POTSUB_FORMS:
            ctx.set_potential_host(case.v, *case.potsub_form(form))
            ctx.upload_phi(case.phi)
            assert_exact(ctx.observables(), case.sums(form), form)


@pytest.mark.parametrize("ext,dtype", [(1, "f64"), (3, "f64"), (2, "f32")])
def test_after_a_step_the_current_buffer_is_read(wa, monkeypatch, ext, dtype):
    """a step moves phi to the other buffer; the same phi uploaded again must give the same sums"""
    set_zchunk(monkeypatch, None)
    shape = (129, 17, 5) if dtype == "f64" else (257, 17, 5)
    case = rd.integer_case(shape, ext, seed=5, storage=dtype)
    want = case.sums("array")
    with wa.Context(params_of(wa, case, dtype)) as ctx:
        ctx.set_potential_host(case.v, *case.potsub_form("array"))
        ctx.upload_phi(case.phi)
        assert_exact(ctx.observables(), want, "before")
        ctx.evolve(0, 1)
        ctx.upload_phi(case.phi)
        assert_exact(ctx.observables(), want, "after")


# ---- z-slabs: every rank's observables() is the all-reduced sum over the GLOBAL grid; r2 and the pot_sub array depend on the
# global z index, so a slab that took its own plane number for it misses the exact sum ----------------------------------------
# (129, 17, 11) in 2 slabs (6, 5 planes) and 3 (4, 4, 3) wherever the engine makes such slabs: a slab needs 2 * ext planes
# (wafer_ctx_create), which rules out 3 slabs for FivePoint and any split of 11 planes for SevenPoint -- asserted below -- so
# those stencils get the shortest nz whose uneven split is allowed as well: 13 (5, 4, 4 and 7, 6) and 19 (7, 6, 6).
SLAB_CASES = [(1, 11, 2), (1, 11, 3), (2, 11, 2), (2, 13, 3), (3, 13, 2), (3, 19, 3)]
REFUSED_SLABS = [(2, 11, 3), (3, 11, 2), (3, 11, 3)]


def slab_sums(wa, case, dtype, world, form):
    def body(ctx, rank):
        ctx.set_overlap(0)
        ctx.set_potential_host(case.v, *case.potsub_form(form))
        ctx.upload_phi(case.phi)
        return ctx.observables()

    res, _ = run_slabs(wa, params_of(wa, case, dtype), world, body, connect=False)
    assert len(res) == world
    return res


@pytest.mark.parametrize("form", ["array", "scalar"])
@pytest.mark.parametrize("ext,nz,world", SLAB_CASES)
def test_slabs(wa, monkeypatch, ext, nz, world, form):
    set_zchunk(monkeypatch, None)
    case = rd.integer_case((129, 17, nz), ext, seed=100 + 10 * ext + world)
    want = case.sums(form)
    for rank, got in enumerate(slab_sums(wa, case, "f64", world, form)):
        assert_exact(got, want, rank)


@pytest.mark.parametrize("shape", [(129, 17, 11), (257, 17, 11)])      # (the float tile is 256 cells wide)
def test_slabs_float_storage(wa, monkeypatch, shape):
    set_zchunk(monkeypatch, None)
    case = rd.integer_case(shape, 1, seed=7, storage="f32")
    want = case.sums("array")
    for rank, got in enumerate(slab_sums(wa, case, "f32", 3, "array")):
        assert_exact(got, want, rank)


@pytest.mark.parametrize("ext,nz,world", REFUSED_SLABS)
def test_slabs_thinner_than_two_frames_are_refused(wa, ext, nz, world):
    """why SLAB_CASES has no such case: the last slab of these splits has fewer than 2 * ext planes"""
    from wafer_amd.slab import partition
    case = rd.integer_case((129, 17, nz), ext, seed=1)
    zb, zc = partition(nz, world, world - 1)
    assert zc < 2 * ext
    with pytest.raises(wa.WaferError, match="2\\*ext planes"):
        wa.Context(dataclasses.replace(params_of(wa, case, "f64"), z_begin=zb, z_count=zc))


# ---- batches --------------------------------------------------------------------------------------------------------------
ONE_SHAPE = [(129, 17, 5)] * 3
MIXED = [(129, 17, 5), (3, 2, 5), (257, 9, 4)]


def batch_members(ext, dtype, shapes, zero=None):
    """(case, pot_sub form) per member: different seeds, and none / scalar / array in turn.  zero: that member's phi is all zeros"""
    out = []
    for m, shape in enumerate(shapes):
        case = rd.integer_case(shape, ext, seed=40 + 7 * m + ext, storage=dtype)
        if m == zero:
            case.phi[...] = 0.0
        out.append((case, rd.POTSUB_FORMS[m % 3]))
    return out


def batch_observables(wa, members, dtype, mixed):
    with wa.Batch([params_of(wa, case, dtype) for case, _ in members], mixed_shapes=mixed) as b:
        assert b.num_shapes() == len({case.shape for case, _ in members})
        for m, (case, form) in enumerate(members):
            b.set_potential_host(m, case.v, *case.potsub_form(form))
            b.upload_phi(m, case.phi)
        return b.observables()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ext", [1, 3])
@pytest.mark.parametrize("shapes,mixed", [(ONE_SHAPE, False), (MIXED, True)], ids=["one_shape", "mixed"])
def test_batches(wa, shapes, mixed, ext, dtype):
    members = batch_members(ext, dtype, shapes)
    got = batch_observables(wa, members, dtype, mixed)
    assert len(got) == len(members)
    for m, (case, form) in enumerate(members):
        assert_exact(got[m], case.sums(form), (m, form))
    assert len({g["norm2"] for g in got}) == len(got)       # the members do differ


@pytest.mark.parametrize("shapes,mixed,zero", [(ONE_SHAPE, False, 1), (MIXED, True, 2)], ids=["one_shape", "mixed"])
def test_a_member_of_zeros_gives_plus_zero(wa, shapes, mixed, zero):
    """phi = 0 under a potential of both signs: the terms are +0 and -0 (v*w*w with v < 0); the sums are +0.0, not -0.0, not NaN,
    and the other members keep their exact sums"""
    members = batch_members(1, "f64", shapes, zero=zero)
    assert members[zero][1] != "none" and (members[zero][0].v < 0).any()
    got = batch_observables(wa, members, "f64", mixed)
    for k in rd.QUANTITIES:
        assert got[zero][k] == 0.0 and math.copysign(1.0, got[zero][k]) == 1.0, (k, got[zero][k])
    for m, (case, form) in enumerate(members):
        if m != zero:
            assert_exact(got[m], case.sums(form), (m, form))
