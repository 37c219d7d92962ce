"""The finding the paired three-step pass rests on, kept as a test: which of the reference's potentials equal their own
mirror image in y, V[x, y, z] == V[x, ny-1-y, z] bit for bit over the work area.

ThreePoint (ext = 1): every centred built-in potential, Dodecahedron included; Cube and QuadWell on some shapes only (integer
division in their bounds); Periodic never.  FivePoint / SevenPoint: none but the all-zero NoPotential -- the reference centres
on (n + 1) / 2 in the PADDED index (potential.rs:366-371), which is the work area's centre only when the frame is one cell wide.
That second half is why the engine compares the array's bits after every write of V and never trusts a potential's name."""
import numpy as np
import pytest


SHAPES = [(64, 64, 64), (48, 96, 40), (33, 47, 20)]
ALWAYS = ["NoPotential", "Coulomb", "ComplexCoulomb", "ElipticalCoulomb", "SimpleCornell", "FullCornell", "Harmonic",
          "ComplexHarmonic", "Dodecahedron"]
BY_SHAPE = ["Cube", "QuadWell"]      # symmetric at the first two shapes, not at (33, 47, 20)
BUILTIN = ALWAYS + BY_SHAPE + ["Periodic"]


def y_symmetric(cfg, v):
    e = cfg.ext
    w = np.ascontiguousarray(v[e:-e, e:-e, e:-e]).view(np.int64)
    return bool(np.array_equal(w, w[:, ::-1, :]))


def generate(oracle, shape, ext, pot, **kw):
    cfg = oracle.Config(*shape, ext=ext, potential=pot, **kw)
    return cfg, oracle.potential_generate(cfg)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pot", BUILTIN)
def test_three_point_potentials_mirror_in_y(oracle, pot, shape):
    cfg, v = generate(oracle, shape, 1, pot, dn=0.1, dt=0.002, mass=1.0, sig=1.0)
    expected = pot in ALWAYS or (pot in BY_SHAPE and shape != (33, 47, 20))
    assert y_symmetric(cfg, v) == expected


@pytest.mark.parametrize("ext", [2, 3])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pot", BUILTIN)
def test_wider_frames_have_no_mirror_but_the_zero_potential(oracle, pot, shape, ext):
    cfg, v = generate(oracle, shape, ext, pot, dn=0.1, dt=0.002, mass=1.0, sig=1.0)
    assert y_symmetric(cfg, v) == (pot == "NoPotential")


@pytest.mark.parametrize("pot,shape,kw", [("Coulomb", (128, 128, 96), dict(dn=0.05, dt=0.0005, mass=1.0, sig=1.0)),
                                          ("SimpleCornell", (256, 128, 64), dict(dn=0.02, dt=0.0001, mass=2.35, sig=1.0))])
def test_benchmark_settings_mirror_in_y(oracle, pot, shape, kw):
    """the grid spacings and the mass of the two benchmark configurations (smaller grids: the property is per cell)"""
    cfg, v = generate(oracle, shape, 1, pot, **kw)
    assert y_symmetric(cfg, v)
    # one ulp on one work cell breaks it: what the device's comparison has to see
    v[5, 7, 9] = np.nextafter(v[5, 7, 9], np.inf)
    assert not y_symmetric(cfg, v)
