"""wafer_k_row_op (norm^2, overlap, normalise, Gram-Schmidt projection: wafer_elementwise.hip.h) where a wave walks more than
one row.  launch_row_op starts at most 8 workgroups of four waves per CU, so on rows of one 1 KiB segment a wave takes a second
row only when ny * nz exceeds 32 * CUs: every small test of these kernels stays below that, and the increment of the walk
(WAFER_ROW_WALK_END: row += stride, y += stride % ny, z += stride / ny, the wrap at y >= ny) never ran in them.  Here
ny * nz = 96 * CUs + 1, so that some wave takes a third row and one a fourth, with grids of a few million cells at the most.

The data is integer valued, so that every product and every sum is exact in the storage and arithmetic types and == holds
against numpy's int64 arithmetic whatever the order of the reduction; the host asserts that condition before it asks the
device.  The row ops compute in double on every dtype (only the step kernels of f32fast compute in float); the float dtypes
store floats.  Normalise by an arbitrary norm is a true division, held to numpy's bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.gpu_common import make_pair, random_phi  # noqa: E402


@pytest.fixture(scope="module")
def wo():
    from oracle import wafer_oracle
    wafer_oracle.build()
    return wafer_oracle


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


@pytest.fixture(scope="module")
def rows(wa):
    """rows of a walk shape: with 96 * CUs + 1 of them a wave of the 32 * CUs takes a third row, and the first a fourth"""
    with wa.Context(wa.Params(8, 8, 8, dn=0.2, dt=0.004)) as ctx:
        cus = ctx.device_info()["compute_units"]
    assert cus > 0
    return 96 * cus + 1


def walk_shape(key, rows):
    if key == "wrap":        # stride % ny != 0: the wrap branch is taken and skipped
        return (5, 97, -(-rows // 97))
    if key == "no_wrap":     # ny divides the stride of 4 * workgroups: y never moves; on f64 a second segment of two cells
        return (130, 64, -(-rows // 64))
    if key == "float_tail":  # on the float dtypes a second segment of three cells, a partial float4
        return (259, 64, -(-rows // 64))
    assert key == "small"
    return (129, 33, 7)


# ny >= 64 at depth: each plane carries 2 * (16 + 3 ext) guard rows
CASES = [("wrap", 1, "f64"), ("wrap", 3, "f32"), ("wrap", 2, "f32fast"), ("no_wrap", 2, "f64"), ("no_wrap", 1, "f32"),
         ("float_tail", 1, "f32"), ("float_tail", 1, "f32fast"), ("small", 2, "f64")]
walk_cases = pytest.mark.parametrize("key,ext,dtype", CASES)


def in_frame(work, ext):
    """the work cells inside a zero Dirichlet frame, float64"""
    out = np.zeros(tuple(s + 2 * ext for s in work.shape))
    out[ext:-ext, ext:-ext, ext:-ext] = work
    return out


def work_of(padded, ext):
    return padded[ext:-ext, ext:-ext, ext:-ext]


def test_the_walk_shapes_walk(wa, rows):
    """the premise: on each walk shape launch_row_op's grid is full (8 workgroups per CU) and has fewer waves than a third of the
    rows, and 4 * workgroups is / is not a multiple of ny as the shape's comment says"""
    cus = (rows - 1) // 96
    for key, _, dtype in CASES:
        if key == "small":
            continue
        nx, ny, nz = walk_shape(key, rows)
        per_seg = 128 if dtype == "f64" else 256
        segs = ny * nz * -(-nx // per_seg)
        blocks = max(1, min(8 * cus, (segs + 3) // 4))
        assert blocks == 8 * cus and ny * nz > 3 * 4 * blocks, (key, dtype)
        assert ((4 * blocks) % ny == 0) == (key != "wrap"), (key, dtype)
        assert nx * ny * nz < 7_000_000


@walk_cases
def test_norm2_and_normalise(wa, rows, key, ext, dtype):
    shape = walk_shape(key, rows)
    cfg, par = make_pair(shape, ext=ext, dtype=dtype)
    rng = np.random.default_rng(11)
    ints = rng.integers(-2, 3, size=shape)
    total = int(np.sum(ints * ints, dtype=np.int64))
    assert total < 2 ** 53
    # an arbitrary wavefunction and an arbitrary norm: the true division
    real = rng.standard_normal(shape)
    if dtype != "f64":
        real = real.astype(np.float32).astype(np.float64)
    n2 = float(np.sum(real * real))
    with wa.Context(par) as ctx:
        ctx.upload_phi(in_frame(ints.astype(np.float64), ext))
        assert ctx.norm2() == total                  # integer squares, integer partial sums: exact in any order
        ctx.normalise(4.0)
        got = ctx.download_phi()
        assert np.array_equal(work_of(got, ext), ints / 2.0)
        assert not got[:ext].any() and not got[:, :ext].any() and not got[:, :, :ext].any()
        assert not got[-ext:].any() and not got[:, -ext:].any() and not got[:, :, -ext:].any()
        assert ctx.norm2() * 4 == total              # quarters of integers: exact as well

        ctx.upload_phi(in_frame(real, ext))
        ctx.normalise(n2)
        want = real / np.sqrt(n2)
        if dtype != "f64":
            want = want.astype(np.float32).astype(np.float64)
        got = work_of(ctx.download_phi(), ext)
        assert np.array_equal(got, want)
        assert np.array_equal(np.signbit(got), np.signbit(want))


def integer_states(shape, rng, shared):
    """three states with values in {-1, 0, 1} on disjoint supports, (x + y + z) % 3 == j; with `shared` > 0, state j is also 1
    on that many cells of state j - 1's support, so that its overlap depends on the projection before it (modified Gram-Schmidt:
    taken with the already-projected phi)"""
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]
    colour = (x + y + z) % 3
    states = [np.where(colour == j, rng.integers(-1, 2, size=shape), 0).astype(np.int64) for j in range(3)]
    for j in range(1, 3):
        at = np.flatnonzero(states[j - 1])[:: max(1, np.count_nonzero(states[j - 1]) // max(shared, 1))][:shared]
        states[j].flat[at] = 1
    return states


def project_int64(phi, states, wnum, cell_bound, sum_bound):
    """grid.rs:477-492 in int64: for each state in order, overlap = sum l * w over the already-projected w, then
    w -= l * overlap.  Asserts the condition under which the device owes equality: every overlap (a double on the device, in
    every dtype) below sum_bound and every intermediate cell below cell_bound (the storage type's exact integers)."""
    w = phi.astype(np.int64)
    for l in states[:wnum]:
        assert int(np.abs(l * w).sum()) < sum_bound          # every partial sum, in whatever order, is exact
        overlap = int(np.sum(l * w, dtype=np.int64))
        assert abs(overlap) < sum_bound
        assert int(np.abs(l).max()) * abs(overlap) < sum_bound
        w = w - l * overlap
        assert int(np.abs(w).max()) < cell_bound
    return w


@walk_cases
def test_orthogonalise(wa, rows, key, ext, dtype):
    """wafer_k_row_op<1> (the first overlap) and <3> (projection fused with the next state's overlap), wnum = 1, 2, 3"""
    shape = walk_shape(key, rows)
    cfg, par = make_pair(shape, ext=ext, dtype=dtype)
    cell_bound = 2 ** 53 if dtype == "f64" else 2 ** 24
    rng = np.random.default_rng(12)
    phi = rng.integers(-2, 3, size=shape)
    with wa.Context(par) as ctx:
        for shared in ((0, 5) if key in ("wrap", "small") else (0,)):
            states = integer_states(shape, rng, shared)
            for j in range(1, 3):
                assert (np.count_nonzero(states[j - 1] * states[j]) == 0) == (shared == 0)
            assert shared or np.count_nonzero(states[0] * states[2]) == 0
            padded = [in_frame(l.astype(np.float64), ext) for l in states]
            for j, l in enumerate(padded):
                ctx.load_state(j, l)
            for wnum in (1, 2, 3):
                want = project_int64(phi, states, wnum, cell_bound, 2 ** 53)
                ctx.upload_phi(in_frame(phi.astype(np.float64), ext))
                ctx.orthogonalise(wnum)
                got = ctx.download_phi()
                assert np.array_equal(work_of(got, ext), want), (shared, wnum)
                assert np.count_nonzero(got) == np.count_nonzero(want), (shared, wnum)      # the frame stays zero
            for j, l in enumerate(padded):
                assert np.array_equal(ctx.download_state(j), l)


@pytest.mark.parametrize("wnum,variant", [(2, 0), (5, None)])
def test_production_path(wo, wa, rows, wnum, variant):
    """the excited-state steps that run these row ops in production: under stencil variant 0, normalise with the first overlap
    fused in and then the projection chain; with more than four stored states the same chain under the default variant.  At the
    project's excited-state bar (test_excited_state_evolve): 1e-13 per cell, rel 1e-12 on norm2."""
    shape = walk_shape("wrap", rows)
    cfg, par = make_pair(shape, ext=1, potential="Harmonic", dn=0.3, dt=0.01, max_states=5)
    v = wo.potential_generate(cfg)
    a, b = wo.ab(cfg, v)
    lowers = []
    for i in range(wnum):  # an orthonormal set, as converged states would be
        l = random_phi(cfg, seed=30 + i)
        wo.orthogonalise(i, l, lowers)
        wo.normalise(l, wo.norm2(cfg, l))
        lowers.append(l)
    phi = random_phi(cfg, seed=40)
    with wa.Context(par) as ctx:
        if variant is not None:
            ctx.set_stencil_variant(variant)
        ctx.set_potential("Harmonic")
        for i, l in enumerate(lowers):
            ctx.load_state(i, l)
        ctx.upload_phi(phi)
        ctx.evolve(wnum, 3)
        assert ctx.x2_passes() == 0
        wo.evolve(cfg, wnum, a, b, phi, lowers, 3)
        got = ctx.download_phi()
        assert np.allclose(got, phi, rtol=0, atol=1e-13)
        assert ctx.norm2() == pytest.approx(wo.norm2(cfg, phi), rel=1e-12)
