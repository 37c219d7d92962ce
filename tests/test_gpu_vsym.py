"""The three-step pass that reads a y-symmetric potential once per mirrored pair of tiles (the VS instantiation of
wafer_k_step3_fused on the folded tile order): the oracle's bits cell by cell, taken exactly when the ARRAY is its own mirror
image in y -- whatever name the potential has and however it got onto the device -- and never otherwise."""
import numpy as np
import pytest

from tests.gpu_common import make_pair, random_phi, ulp_diff

pytestmark = pytest.mark.gpu


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


def paired(ctx):
    """did the last three-step launch run the instantiation with the trailing `true` (VS)?"""
    name = ctx.stencil_kernel_instance()
    assert name.startswith("wafer_k_step3_fused<")
    return name.endswith(", 1, true>")


KW = dict(ext=1, dn=0.2, dt=0.004, mass=1.0)
# grids the three-step kernel takes by default (above its cell threshold): 8 and 9 rows of 128 x 16 tiles, 8 tiles per layer of
# 256 CUs' worth of workgroups: dozens of z-chunks per column
GRIDS = [(128, 128, 128), (128, 144, 120)]


@pytest.mark.parametrize("shape", GRIDS)
@pytest.mark.parametrize("pot", ["Coulomb", "SimpleCornell", "Harmonic", "Dodecahedron"])
def test_paired_pass_gives_the_oracles_bits(wo, wa, pot, shape):
    """3, 6 and 7 steps (7: a single-step remainder behind two paired passes), nty even and odd"""
    cfg, par = make_pair(shape, potential=pot, **KW)
    a, b = wo.ab(cfg, wo.potential_generate(cfg))
    phi0 = random_phi(cfg, seed=7)
    ref, done = phi0.copy(), 0
    for steps in (3, 6, 7):
        wo.evolve(cfg, 0, a, b, ref, [], steps - done)
        done = steps
        with wa.Context(par) as ctx:
            ctx.set_potential(pot)
            ctx.upload_phi(phi0)
            assert ctx.steps_per_launch() == 3
            ctx.evolve(0, steps)
            assert paired(ctx), ctx.stencil_kernel_instance()
            d = ulp_diff(ctx.download_phi(), ref)
            print(pot, shape, steps, "max_ulp", d)
            assert d == 0


@pytest.mark.parametrize("pot,shape", [("Periodic", (128, 128, 128)), ("Coulomb", (128, 136, 120))])
def test_asymmetric_potential_and_ragged_rows_keep_the_plain_pass(wo, wa, pot, shape):
    """(the oracle steps on the array the device generated: the device's sin of Periodic is not libm's to the last bit)"""
    cfg, par = make_pair(shape, potential=pot, **KW)
    phi = random_phi(cfg, seed=8)
    with wa.Context(par) as ctx:
        ctx.set_potential(pot)
        a, b = wo.ab(cfg, ctx.download_array("v"))
        ctx.upload_phi(phi)
        ctx.evolve(0, 7)
        assert not paired(ctx), ctx.stencil_kernel_instance()
        wo.evolve(cfg, 0, a, b, phi, [], 7)
        assert ulp_diff(ctx.download_phi(), phi) == 0


# (x, y, z) work cells of a 128^3 grid: the upper half of y, the lower half, and a row that the centre tile below the mirror
# line (rows 48 .. 63) reads as a halo row (y0 + 17)
@pytest.mark.parametrize("cell", [(40, 100, 77), (40, 20, 77), (90, 65, 3)])
def test_one_ulp_on_one_cell_of_an_uploaded_potential(wo, wa, cell):
    """the paired pass must not run, and the result is the oracle's on the CHANGED array (an implementation that trusts the
    name, or reads the lower half without comparing, fails the upper-half case)"""
    cfg, par = make_pair((128, 128, 128), potential="Coulomb", **KW)
    v = wo.potential_generate(cfg)
    phi0 = random_phi(cfg, seed=9)
    with wa.Context(par) as ctx:       # the array as generated, uploaded: symmetric, so the paired pass runs
        ctx.set_potential_host(v)
        ctx.upload_phi(phi0)
        ctx.evolve(0, 3)
        assert paired(ctx)
    e = cfg.ext
    x, y, z = cell
    v[e + x, e + y, e + z] = np.nextafter(v[e + x, e + y, e + z], np.inf)
    a, b = wo.ab(cfg, v)
    ref = phi0.copy()
    wo.evolve(cfg, 0, a, b, ref, [], 6)
    with wa.Context(par) as ctx:
        ctx.set_potential_host(v)
        ctx.upload_phi(phi0)
        ctx.evolve(0, 6)
        assert not paired(ctx), ctx.stencil_kernel_instance()
        assert ulp_diff(ctx.download_phi(), ref) == 0


def test_one_context_follows_its_potential(wo, wa):
    """symmetric -> asymmetric upload -> symmetric again: instantiation and workgroup table follow each time"""
    cfg, par = make_pair((128, 128, 128), potential="Coulomb", **KW)
    v = wo.potential_generate(cfg)
    vbad = v.copy()
    vbad[50, 111, 60] = np.nextafter(vbad[50, 111, 60], -np.inf)
    ref = random_phi(cfg, seed=10)
    with wa.Context(par) as ctx:
        ctx.upload_phi(ref)
        for arr, want in ((None, True), (vbad, False), (v, True), (vbad, False)):
            if arr is None:
                ctx.set_potential("Coulomb")
            else:
                ctx.set_potential_host(arr)
            ctx.evolve(0, 3)
            assert paired(ctx) == want, ctx.stencil_kernel_instance()
            a, b = wo.ab(cfg, v if arr is None else arr)
            wo.evolve(cfg, 0, a, b, ref, [], 3)
            assert ulp_diff(ctx.download_phi(), ref) == 0


def test_knob_on_and_off_agree_at_256_cubed(wa, monkeypatch):
    sums = {}
    for knob in ("-1", "0"):
        monkeypatch.setenv("WAFER_F3_VSYM", knob)
        with wa.Context(wa.Params(256, 256, 256, dn=0.1, dt=0.002, max_states=1)) as ctx:
            ctx.set_potential("Coulomb")
            ctx.set_initial_condition("Gaussian", seed=3)
            ctx.evolve(0, 30)
            assert paired(ctx) == (knob == "-1"), ctx.stencil_kernel_instance()
            sums[knob] = ctx.checksum()
    assert sums["-1"] == sums["0"]


@pytest.mark.parametrize("dtype,shape,steps", [("f32", (128, 32, 11), 9), ("f32", (128, 48, 23), 11), ("f32", (256, 32, 11), 10),
                                               ("f32fast", (256, 32, 11), 10), ("f32fast", (256, 48, 23), 11)])
def test_fp32_storage_paired_pass_gives_the_single_step_kernels_bits(wa, dtype, shape, steps, monkeypatch):
    """fp32 storage (fp64 and fp32 arithmetic): the comparison runs on the float array; WAFER_F3_VSYM=1 runs the paired pass
    there (the default keeps these dtypes on the plain pass)"""
    monkeypatch.setenv("WAFER_FUSE3_MIN_NY", "1")
    monkeypatch.setenv("WAFER_F3_VSYM", "1")
    out = {}
    for variant, zchunk in ((3, ""), (3, "5"), (1, "")):
        if zchunk:
            monkeypatch.setenv("WAFER_ZCHUNK", zchunk)
        else:
            monkeypatch.delenv("WAFER_ZCHUNK", raising=False)
        par = wa.Params(*shape, dn=0.2, dt=0.004, mass=1.3, central_difference=1, dtype=dtype)
        with wa.Context(par) as ctx:
            ctx.set_stencil_variant(variant)
            ctx.set_potential("Coulomb")
            ctx.set_initial_condition("Gaussian", seed=5)
            ctx.evolve(0, steps)
            if variant == 3:
                assert paired(ctx), ctx.stencil_kernel_instance()
            out[(variant, zchunk)] = ctx.download_phi()
    assert np.array_equal(out[(3, "")], out[(1, "")])
    assert np.array_equal(out[(3, "5")], out[(1, "")])


def test_fp32_storage_keeps_the_plain_pass_by_default(wa, monkeypatch):
    monkeypatch.setenv("WAFER_FUSE3_MIN_NY", "1")
    monkeypatch.delenv("WAFER_F3_VSYM", raising=False)
    with wa.Context(wa.Params(128, 32, 11, dn=0.2, dt=0.004, central_difference=1, dtype="f32")) as ctx:
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Gaussian", seed=5)
        ctx.evolve(0, 3)
        assert not paired(ctx)
