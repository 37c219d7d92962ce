"""wafer_diag_checksum against its host model (tests/checksum_model.py, a numpy restatement of the definition in
include/wafer_hip.h).  Every "same bits" claim on grids too big to download rests on this sum -- bench.py's parity checks,
slab.overlap_modes_agree, the full-size path equalities -- and those uses compare it only with itself: a kernel that left cells
out, clipped a slab's planes wrongly, read the wrong width or the wrong buffer would pass them all.  Here every value is held
to the model with ==: the whole grid, plane ranges, one bit of one cell, two cells swapped, the buffer that is current after
steps / a symmetrise / a clone, and z-slabs against the undecomposed grid.  The truth for the stored bits is download_phi()."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.checksum_model import MASK, model  # noqa: E402
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


# (65, 33, 20): the x loop's stride of 64 plus one cell; (257, 5, 3): five trips of it, ragged
SHAPES = [(1, 1, 1), (3, 2, 5), (65, 33, 20), (130, 9, 7), (257, 5, 3)]
EXTS = [1, 2, 3]
DTYPES = ["f64", "f32", "f32fast"]
grid_cases = pytest.mark.parametrize("shape,ext,dtype", [(s, e, d) for s in SHAPES for e in EXTS for d in DTYPES])
FAR = 2 ** 32 - 16      # a z_begin whose (int) is a negative plane


def bits_equal(a, b):
    """bit for bit (NaNs and signed zeros included)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def special_phi(padded_shape, ext, dtype, seed=1):
    """N(0, 1) over the WHOLE padded array -- the frame is non-zero on purpose: it must not count -- with work cells set to
    -0.0, 0.0, +-inf and the smallest normal number of the storage type; on f64 also a NaN and a subnormal; on the float dtypes
    also the smallest float subnormal, +-2^-149 (a float array must hold it, and the sum must count its bits)"""
    phi = np.random.default_rng(seed).standard_normal(padded_shape)
    work = phi[ext:-ext, ext:-ext, ext:-ext]
    specials = [-0.0, 0.0, np.inf, -np.inf, float(np.finfo(np.float64 if dtype == "f64" else np.float32).tiny)]
    if dtype == "f64":
        specials += [np.nan, 5e-324]
    else:
        specials += [2.0 ** -149, -2.0 ** -149]
    for i, v in enumerate(specials):
        work[np.unravel_index((1 + 7919 * i) % work.size, work.shape)] = v
    return phi


def work_of(padded, ext):
    return padded[ext:-ext, ext:-ext, ext:-ext]


def stored(ctx, dtype):
    """the work cells as the device holds them: download_phi(), on the float dtypes narrowed back to float32 (and widened
    again, which is exact)"""
    got = ctx.download_phi()
    if dtype != "f64":
        narrow = got.astype(np.float32).astype(np.float64)
        assert bits_equal(narrow, got)      # a float array downloads as floats
        got = narrow
    return got


def model_range(work, z_begin, z_count, dtype, own=None):
    """the model over (range ∩ grid ∩ owned planes)"""
    nz = work.shape[2]
    own = own or (0, nz)
    a, b = max(min(z_begin, nz), own[0]), min(z_begin + z_count, nz, own[1])
    return model(work[:, :, a:b], a, dtype) if b > a else 0


@grid_cases
def test_whole_grid(wa, shape, ext, dtype):
    cfg, par = make_pair(shape, ext=ext, dtype=dtype)
    phi = special_phi(cfg.padded_shape, ext, dtype)
    with wa.Context(par) as ctx:
        ctx.upload_phi(phi)
        held = stored(ctx, dtype)
        if dtype == "f64":
            assert bits_equal(held, phi)
        else:
            assert (work_of(held, ext) == -2.0 ** -149).any()      # the float array holds the subnormal (no flush to zero)
        want = model(work_of(held, ext), 0, dtype)
        assert ctx.checksum() == want
        assert ctx.checksum() == want          # the sum's device word is cleared between calls
        zero_frame = np.zeros_like(held)       # ... and the frame does not count
        work_of(zero_frame, ext)[...] = work_of(held, ext)
        ctx.upload_phi(zero_frame)
        assert ctx.checksum() == want


@grid_cases
def test_plane_ranges(wa, shape, ext, dtype):
    cfg, par = make_pair(shape, ext=ext, dtype=dtype)
    nz = shape[2]
    with wa.Context(par) as ctx:
        ctx.upload_phi(special_phi(cfg.padded_shape, ext, dtype, seed=2))
        work = work_of(stored(ctx, dtype), ext)
        whole = ctx.checksum()
        assert whole == model(work, 0, dtype)
        ranges = [(0, 1), (nz - 1, 1), (nz // 3, max(1, nz // 2)), (nz - 1, 5), (nz, 3), (0, 0), (0, nz), (0, nz + 7)]
        for z0, zc in ranges:
            assert ctx.checksum(z0, zc) == model_range(work, z0, zc, dtype), (z0, zc)
        assert ctx.checksum(nz, 3) == 0 and ctx.checksum(0, 0) == 0
        cuts = sorted({0, nz // 3, (2 * nz) // 3, nz})
        assert sum(ctx.checksum(a, b - a) for a, b in zip(cuts, cuts[1:])) & MASK == whole
        assert sum(ctx.checksum(k, 1) for k in range(nz)) & MASK == whole
        # a z_begin of 2^31 or more is past every grid: nothing to sum, with or without z_begin + z_count passing 2^32
        assert ctx.checksum(FAR, 8) == 0
        assert ctx.checksum(FAR, 32) == 0
        assert ctx.checksum(2 ** 31, nz) == 0


def flip_lowest_bit(v, dtype):
    if dtype == "f64":
        return float((np.array([v], dtype=np.float64).view(np.uint64) ^ np.uint64(1)).view(np.float64)[0])
    return float((np.array([v], dtype=np.float32).view(np.uint32) ^ np.uint32(1)).view(np.float32)[0])


@grid_cases
def test_cell_by_cell(wa, shape, ext, dtype):
    """one bit of one cell, and where a value sits: the position dependence the decomposition check needs"""
    cfg, par = make_pair(shape, ext=ext, dtype=dtype)
    nx, ny, nz = shape
    cells = [(0, 0, 0), (nx - 1, ny - 1, nz - 1), (63, ny - 1, nz - 1), (64, ny - 1, nz - 1), (nx // 2, ny // 2, nz // 2)]
    cells = [c for i, c in enumerate(cells) if c[0] < nx and c not in cells[:i]]
    with wa.Context(par) as ctx:
        ctx.upload_phi(special_phi(cfg.padded_shape, ext, dtype, seed=3))
        phi = stored(ctx, dtype)
        work = work_of(phi, ext)       # a view: the edits below go into phi
        for c in cells:                # a flipped bit must stay a plain normal number in the storage type
            if not np.isfinite(work[c]) or abs(work[c]) < 1e-30:
                work[c] = 0.75
        ctx.upload_phi(phi)
        prev = ctx.checksum()
        assert prev == model(work, 0, dtype)
        for c in cells:
            work[c] = flip_lowest_bit(work[c], dtype)
            ctx.upload_phi(phi)
            assert bits_equal(stored(ctx, dtype), phi)
            got = ctx.checksum()
            assert got != prev, c
            assert got == model(work, 0, dtype), c
            prev = got
        if nx >= 2:                    # two unequal cells of one row change places
            y, z = ny - 1, nz - 1
            xa, xb = (63, 64) if nx > 64 else (0, nx - 1)
            if work[xa, y, z] == work[xb, y, z]:
                work[xb, y, z] = 0.5 if work[xa, y, z] != 0.5 else 0.25
                ctx.upload_phi(phi)
                prev = ctx.checksum()
            work[xa, y, z], work[xb, y, z] = work[xb, y, z], work[xa, y, z]
            ctx.upload_phi(phi)
            got = ctx.checksum()
            assert got != prev
            assert got == model(work, 0, dtype)


@grid_cases
def test_the_current_buffer(wa, shape, ext, dtype):
    """the sum is taken of the buffer that is current: after odd numbers of steps, after symmetrise (which swaps buffers) and
    after clone_state_to_phi"""
    cfg, par = make_pair(shape, ext=ext, dtype=dtype, potential="Harmonic")

    def check(ctx):
        got = ctx.checksum()
        assert got == model(work_of(stored(ctx, dtype), ext), 0, dtype)
        return got

    with wa.Context(par) as ctx:
        ctx.set_potential("Harmonic")
        ctx.upload_phi(random_phi(cfg, seed=4))
        seen = [check(ctx)]
        for steps in (1, 5, 3):
            ctx.evolve(0, steps)
            seen.append(check(ctx))
        assert len(set(seen)) == len(seen)     # every step changed the wavefunction
        ctx.push_state()
        pushed = seen[-1]
        ctx.evolve(0, 1)
        assert check(ctx) != pushed
        ctx.clone_state_to_phi(0)
        assert check(ctx) == pushed
        if ext == 3:                           # (on ny = 1 the mirror leaves zeros, as the reference's does: no != here)
            ctx.symmetrise("AboutY")
            check(ctx)


SLAB_SHAPE = (21, 18, 40)
SLABS = [(0, 13), (13, 17), (30, 10)]
# each of these lies inside one slab, straddles the edge of others and misses the rest
SLAB_RANGES = [(0, 40), (0, 13), (1, 11), (5, 3), (10, 6), (13, 17), (12, 19), (28, 5), (30, 10), (33, 20), (39, 1), (40, 3),
               (0, 0), (20, 0), (FAR, 32)]


@pytest.mark.parametrize("halo_mult", [1, 3])
@pytest.mark.parametrize("ext,dtype", [(1, "f64"), (3, "f64"), (2, "f32")])
def test_slabs(wa, ext, dtype, halo_mult):
    """on a z-slab only the owned planes count (the ghost planes hold the neighbours' values: the GLOBAL array is uploaded), the
    slabs' sums add up to the undecomposed grid's range by range, and download_window serves exactly the owned + ghost planes"""
    nx, ny, nz = SLAB_SHAPE
    R, G = ext, halo_mult * ext
    full = special_phi(tuple(s + 2 * ext for s in SLAB_SHAPE), ext, dtype, seed=5)
    base = dict(dn=0.2, dt=0.004, central_difference=ext, dtype=dtype)
    with wa.Context(wa.Params(*SLAB_SHAPE, **base)) as ctx:
        ctx.upload_phi(full)
        held = stored(ctx, dtype)
        if dtype == "f64":
            assert bits_equal(held, full)
        whole = [ctx.checksum(z0, zc) for z0, zc in SLAB_RANGES]
    work = work_of(held, ext)
    assert whole == [model_range(work, z0, zc, dtype) for z0, zc in SLAB_RANGES]
    assert len(set(whole)) == len(SLAB_RANGES) - 3        # (40, 3), (0, 0), (20, 0), (FAR, 32) give 0; the rest differ
    parts = []
    for z0, zc in SLABS:
        with wa.Context(wa.Params(*SLAB_SHAPE, z_begin=z0, z_count=zc, halo_depth=G, **base)) as ctx:
            ctx.upload_phi(full)
            sums = [ctx.checksum(a, n) for a, n in SLAB_RANGES]
            assert sums == [model_range(work, a, n, dtype, own=(z0, z0 + zc)) for a, n in SLAB_RANGES], (z0, zc)
            parts.append(sums)
            # the padded planes this context holds: owned + G ghost planes per side, inside the global padded grid
            lo, hi = max(0, z0 + R - G), min(nz + 2 * R, z0 + R + zc + G)
            for zp, n in [(lo, hi - lo), (lo, 1), (hi - 1, 1), (z0 + R, zc), (z0 + R - 1, zc + 2)]:
                assert bits_equal(ctx.download_window("phi", zp, n), held[:, :, zp:zp + n]), (z0, zc, zp, n)
            outside = [(hi - 1, 2), (hi, 1), (lo, hi - lo + 1)] + ([(lo - 1, 2), (lo - 1, 1)] if lo > 0 else [])
            for zp, n in outside:
                with pytest.raises(wa.WaferError):
                    ctx.download_window("phi", zp, n)
    for i, (a, n) in enumerate(SLAB_RANGES):
        assert sum(p[i] for p in parts) & MASK == whole[i], (a, n)
