"""Moment matrices of the stored states, on the device: wafer_k_moment_sums through Context.moments, against the context's own
observables and ritz_matrices (==), the numpy model of tests/moments_model.py (a tolerance on N(0, 1) states, == on integer
states), a Ritz step on box states, the calls that must not notice it, and the wafer-hip driver's `gpu.moments` section.

Cases are those of tests/test_gpu_ritz.py: smaller than a tile, odd sizes, and one shape whose observables launch has several tiles
in x and y and several z-chunks.  The stored states are random on the frame too: the kernel never reads a frame cell."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import moments_model as mm  # noqa: E402
from tests import ritz_model as rm  # noqa: E402
from tests import test_gpu_ritz as gr  # noqa: E402  (its cases, its box states and its driver case)

KS, CASES = gr.KS, gr.CASES
bits, params_of, storage_of, seed_of = gr.bits, gr.params_of, gr.storage_of, gr.seed_of


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


@functools.lru_cache(maxsize=None)
def measured(dtype, shape, ext):
    """one context per case: eight N(0, 1) stored states with a random frame -- moments and ritz_matrices for every k of KS,
    observables of every state, the states and phi before and after -- then eight integer states and their moments; with the
    model's matrices of both sets.  Computed once, shared by the tests below."""
    import wafer_amd as wa
    states = rm.random_states(shape, ext, 9, seed_of(dtype, shape, ext), frame=True, storage=storage_of(dtype))
    ints = mm.integer_states(shape, ext, 8, seed_of(dtype, shape, ext) + 1, storage=storage_of(dtype))
    with wa.Context(params_of(wa, shape, ext, dtype)) as ctx:
        for j in range(8):
            ctx.load_state(j, states[j])
        ctx.upload_phi(states[8])
        before_v = ctx.moments(8)                       # no potential yet: V is not read
        ctx.set_potential("Harmonic")
        moms = {k: ctx.moments(k) for k in KS}
        down = [ctx.download_state(j) for j in range(8)]
        phi = ctx.download_phi()
        smat = {k: ctx.ritz_matrices(k)[1] for k in KS}
        obs = []
        for j in range(8):
            ctx.clone_state_to_phi(j)
            obs.append(ctx.observables())
        for j in range(8):
            ctx.load_state(j, ints[j])
        int_moms = {k: ctx.moments(k) for k in KS}
    return dict(moms=moms, before_v=before_v, smat=smat, obs=obs, states=states, down=down, phi=phi, int_moms=int_moms,
                model=mm.matrices(shape, ext, states[:8], scales=True), int_model=mm.matrices(shape, ext, ints))


# ---- M1: the bit ties ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,shape,ext", CASES)
def test_bit_ties(dtype, shape, ext):
    m = measured(dtype, shape, ext)
    for k in KS:
        got = m["moms"][k]
        for j in range(k):
            print(k, j, repr(got["r2"][j, j]), repr(m["obs"][j]["r2"]), repr(got["s"][j, j]), repr(m["obs"][j]["norm2"]))
    for k in KS:
        got = m["moms"][k]
        assert got["origin"] == mm.centres(shape)
        for j in range(k):
            assert got["r2"][j, j] == m["obs"][j]["r2"], (k, j)
            assert got["s"][j, j] == m["obs"][j]["norm2"], (k, j)
        assert np.array_equal(bits(got["s"]), bits(m["smat"][k])), k
        for name in mm.NAMES:
            assert got[name].shape == (k, k)
            assert np.array_equal(bits(got[name]), bits(got[name].T)), (k, name)
            assert np.array_equal(bits(got[name]), bits(m["moms"][8][name][:k, :k])), (k, name)
            assert np.array_equal(bits(m["before_v"][name]), bits(m["moms"][8][name])), name     # the potential changes nothing


# ---- M2: all five matrices against the model -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,shape,ext", CASES)
def test_matrices_against_the_model(dtype, shape, ext):
    m = measured(dtype, shape, ext)
    want, scale = m["model"]
    for k in KS:
        for name in mm.NAMES:
            err = np.abs(m["moms"][k][name] - want[name][:k, :k])
            print(k, name, float(np.max(err / scale[name][:k, :k])))
    for k in KS:
        for name in mm.NAMES:
            err = np.abs(m["moms"][k][name] - want[name][:k, :k])
            assert np.all(err <= 1e-12 * scale[name][:k, :k]), (k, name, float(np.max(err / scale[name][:k, :k])))


# ---- M3: integer states, exactly ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,shape,ext", CASES)
def test_integer_states_are_exact(dtype, shape, ext):
    m = measured(dtype, shape, ext)
    for k in KS:
        for name in mm.NAMES:
            assert np.array_equal(m["int_moms"][k][name], m["int_model"][name][:k, :k]), (k, name)


# ---- M4: read-only --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,shape,ext", CASES)
def test_states_and_phi_keep_their_bits(dtype, shape, ext):
    m = measured(dtype, shape, ext)
    for j in range(8):
        assert np.array_equal(bits(m["down"][j]), bits(m["states"][j])), j
    assert np.array_equal(bits(m["phi"]), bits(m["states"][8]))


@pytest.mark.parametrize("variant", [None, 0, 2])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_evolve_does_not_notice_the_call(wa, dtype, variant):
    """evolve(2, 8); moments(2); evolve(2, 6) equals the same sequence without the call, with the two-step pass armed: the Gram
    matrix and the pass's images survive"""
    shape, ext = (12, 10, 9), 1
    start = rm.random_states(shape, ext, 3, 78, frame=False, storage=storage_of(dtype))
    out = []
    for call in (True, False):
        with wa.Context(params_of(wa, shape, ext, dtype)) as ctx:
            ctx.set_potential("Harmonic")
            if variant is not None:
                ctx.set_stencil_variant(variant)
            for j in range(2):
                ctx.load_state(j, start[j])
            ctx.upload_phi(start[2])
            ctx.evolve(2, 8)
            if variant != 0:
                assert ctx.x2_passes() > 0
            if call:
                ctx.moments(2)
            ctx.evolve(2, 6)
            out.append(ctx.download_phi())
    assert np.array_equal(bits(out[0]), bits(out[1]))


# ---- M5: after a Ritz step on box states --------------------------------------------------------------------------------------------------------
def test_moments_of_rotated_box_states(wa):
    shape = (12, 10, 9)
    sines = [rm.sine_state(shape, 1, p) for p in gr.LEVELS]
    mixed = [sum(gr.MIX[a, b] * sines[b] for b in range(4)) for a in range(4)]
    with wa.Context(wa.Params(*shape, dn=gr.DN, dt=gr.DT, mass=gr.MASS, central_difference=1, max_states=4)) as ctx:
        ctx.set_potential("NoPotential")
        for j, l in enumerate(mixed):
            ctx.load_state(j, l)
        ctx.ritz(4)
        got = ctx.moments()
        down = [ctx.download_state(j) for j in range(4)]
    want, scale = mm.matrices(shape, 1, down, scales=True)
    for name in mm.NAMES:
        assert np.all(np.abs(got[name] - want[name]) <= 1e-12 * scale[name]), name
    assert np.max(np.abs(got["s"] - np.eye(4))) <= 1e-12
    # The rotated states are the box levels, each within 1e-12 per cell of its sine (tests/test_gpu_ritz.py), lowest first: (1,1,1),
    # then (2,1,1) -- x is the longest axis.  (1,1,1) is even about the box centre (n - 1) / 2 in every axis, so about the call's
    # origin, one cell above, its dipole is -1 per axis; (2,1,1) is odd in x, so <111|x|211> is large (-16 L / 9 pi^2 of a box of
    # length L = 13) and <111|y|211>, <111|z|211> vanish.  Bound: a state error d <= 1e-12 per cell moves an entry by at most
    # 2 sum |dx| |l| |d| <= 2 * 6.5 * sqrt(1080) * 1e-12 = 4.3e-10.
    assert np.max(np.abs(np.array([got[a][0, 0] for a in "xyz"]) + 1.0)) <= 1e-9
    assert abs(got["x"][0, 1]) > 1.0 and abs(got["y"][0, 1]) <= 1e-9 and abs(got["z"][0, 1]) <= 1e-9


# ---- M6: refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(wa):
    from wafer_amd.engine import WAFER_ERR_INVALID, WAFER_ERR_STATE
    shape, ext = (12, 10, 9), 1
    states = rm.random_states(shape, ext, 3, 9)
    with wa.Context(params_of(wa, shape, ext, "f64", max_states=10)) as ctx:
        for j in range(2):
            ctx.load_state(j, states[j])
        ctx.upload_phi(states[2])
        for k, code in ((0, WAFER_ERR_INVALID), (9, WAFER_ERR_INVALID), (3, WAFER_ERR_STATE)):
            with pytest.raises(wa.WaferError) as e:
                ctx.moments(k)
            assert e.value.code == code, (k, e.value.code)
        sentinel = np.full(5 * 9, np.nan)
        L = wa.load_library()
        import ctypes as C
        assert L.wafer_moment_matrices(ctx._h, 3, sentinel.ctypes.data_as(C.POINTER(C.c_double))) == WAFER_ERR_STATE
        assert L.wafer_moment_matrices(ctx._h, 2, None) == WAFER_ERR_INVALID
        assert np.all(np.isnan(sentinel))                                    # a refused call writes nothing
        for j in range(2):
            assert np.array_equal(bits(ctx.download_state(j)), bits(states[j])), j
        assert np.array_equal(bits(ctx.download_phi()), bits(states[2]))
        assert ctx.moments()["s"].shape == (2, 2)                            # k = None: both


def test_a_slab_context_is_refused(wa):
    from wafer_amd.engine import WAFER_ERR_INVALID
    shape, ext = (12, 10, 9), 1
    states = rm.random_states(shape, ext, 2, 4, frame=False)
    with wa.Context(params_of(wa, shape, ext, "f64", z_begin=0, z_count=shape[2])) as ctx:
        for j in range(2):
            ctx.load_state(j, states[j])
        with pytest.raises(wa.WaferError, match="z-slab") as e:
            ctx.moments(2)
        assert e.value.code == WAFER_ERR_INVALID
        for j in range(2):
            assert np.array_equal(bits(ctx.download_state(j)), bits(states[j]))


# ---- M7: wafer-hip --------------------------------------------------------------------------------------------------------------------------------
def moment_lines(mom, fmt):
    k = len(mom["s"])
    return ["%3d %3d" % (i, j) + "".join(" " + fmt(mom[name][j, i], 10).rjust(19) for name in mm.NAMES) for j in range(k) for i in range(j + 1)]


def test_driver_moments_section(wa, tmp_path):
    plain, _ = gr.run_cli(tmp_path, "plain", "")
    off, _ = gr.run_cli(tmp_path, "off", "gpu:\n    moments: false\n")
    on, _ = gr.run_cli(tmp_path, "on", "gpu:\n    moments: true\n")
    assert gr.table_of(plain.stdout) == gr.table_of(off.stdout)
    assert "Moments" not in plain.stdout
    lines = gr.table_of(on.stdout)
    at = lines.index("Moments")
    assert lines[:at] == gr.table_of(plain.stdout)                 # everything printed without the key is a prefix
    ctx, fmt = gr.solve_like_the_driver(wa)
    with ctx:
        want = moment_lines(ctx.moments(), fmt)
    assert len(want) == 6
    assert lines[at + 1:] == want + [""], (lines[at + 1:], want)
