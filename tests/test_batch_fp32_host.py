"""Float-storage batches (dtype "f32" / "f32fast" in wafer_amd.Batch) on the host: what wafer_batch_create accepts and rejects
before any HIP call, the inputs of tests/test_gpu_batch_fp32.py held to the domain in which the f32fast reference is one to the
bit, and the chain model of the excited-state step (tests/batch_fp32_model.py) held to the oracle."""
import numpy as np
import pytest

from tests import batch_fp32_model as model
from tests import fp32_reference as ref


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


@pytest.fixture(scope="module")
def wo():
    from oracle import wafer_oracle
    wafer_oracle.build()
    return wafer_oracle


def _params(wa, **kw):
    base = dict(nx=16, ny=16, nz=16, dn=0.2, dt=0.004)
    base.update(kw)
    return wa.Params(**base)


# ---- 1. uniform float batches pass validation ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f32fast"])
def test_uniform_float_batch_passes_validation(wa, dtype):
    """every member f32 (or every member f32fast): validation lets the batch through, and creation then needs the device --
    code -2 (HIP) on a machine without one, never -1 (INVALID)"""
    import torch
    members = [_params(wa, dtype=dtype), _params(wa, dtype=dtype, dt=0.002, mass=2.0), _params(wa, dtype=dtype, dn=0.3)]
    if torch.cuda.is_available():
        with wa.Batch(members) as b:
            assert len(b) == 3 and b.dispatch()["dtype"] == dtype
        return
    with pytest.raises(wa.WaferError) as e:
        wa.Batch(members)
    assert e.value.code == -2, str(e.value)


# ---- 2. one dtype per batch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,other", [("f64", "f32"), ("f32", "f64"), ("f32", "f32fast"), ("f32fast", "f32"), ("f64", "f32fast")])
def test_mixed_dtypes_are_rejected_naming_the_member(wa, first, other):
    members = [_params(wa, dtype=first), _params(wa, dtype=first, dt=0.002), _params(wa, dtype=other)]
    with pytest.raises(wa.WaferError) as e:
        wa.Batch(members)
    assert e.value.code == -1
    assert "member 2" in str(e.value) and "dtype" in str(e.value)


@pytest.mark.parametrize("where", [0, 1])
def test_a_dtype_outside_the_enum_is_rejected(wa, where):
    """through the C ABI: Params cannot express it"""
    import ctypes as C
    from wafer_amd import engine
    L = wa.load_library()
    arr = (engine._Params * 2)(_params(wa).c(), _params(wa).c())
    arr[where].dtype = 3
    h = C.c_void_p()
    assert L.wafer_batch_create(arr, 2, C.byref(h)) == -1
    msg = L.wafer_last_error().decode()
    assert "member %d" % where in msg and "dtype" in msg


# ---- 3. the GPU file's members stay inside the planned fp32 division's checked domain --------------------------------------------
def _domain_cases():
    out = []
    for ext in (1, 2, 3):
        for shape in model.SHAPES:
            out.append((shape, ext, model.STEP_COUNTS))
    for ext in (1, 2):
        out.append((model.VARIANT_SHAPES[1], ext, list(model.VARIANT_STEPS)))   # ((65, 33, 20) runs more steps above)
    return out


def test_member_table_has_distinct_parameters():
    for key in ("dn", "dt", "mass", "potential"):
        assert len({m[key] for m in model.MEMBERS}) == len(model.MEMBERS) == 3, key
    assert all(m["potential"] in ref.POTENTIALS and m["dt"] <= m["dn"] ** 2 / 3 for m in model.MEMBERS)


@pytest.mark.parametrize("shape,ext,counts", _domain_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_member_inputs_stay_in_the_checked_fp32_division_domain(wo, shape, ext, counts):
    """the all-float model is the IEEE division, the kernels' planned one agrees with it for 2^-100 <= |x|, |x / den| < 2^101
    (tests/test_fp32_reference.py asserts the same bounds): every member x shape x ext of the GPU file divides inside it.  A
    member that leaves it is replaced in batch_fp32_model.MEMBERS; the bound stays."""
    for k in range(len(model.MEMBERS)):
        cfg, v, phi = model.member_inputs(wo, k, shape, ext)
        _, div = ref.evolve_numpy(cfg, v, phi, counts, np.float32, np.float32, "registers")
        print(k, shape, ext, div)
        assert div.x_max > 0.0 and div.q_max > 0.0, "the run divided nothing but zeros"
        assert 2.0 ** -100 <= div.x_min and div.x_max < 2.0 ** 101, (k, div)
        assert 2.0 ** -100 <= div.q_min and div.q_max < 2.0 ** 101, (k, div)


# ---- 4. the chain model is the oracle's excited-state evolve ---------------------------------------------------------------------
@pytest.mark.parametrize("wnum", [1, 2, 3])
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_chain_model_with_double_storage_is_the_oracle(wo, ext, wnum):
    """storage = float64: step, norm2, phi / sqrt(norm2), modified Gram-Schmidt in storage order -- 1e-13 per cell against
    wo.evolve (the project's excited-state bar), for every member; orthogonalise alone as well"""
    shape, steps = model.EXCITED_SHAPES[0], 4
    for k in range(len(model.MEMBERS)):
        cfg, v, phi = model.member_inputs(wo, k, shape, ext)
        lowers = model.stored_states(cfg, k, wnum, storage=np.float64)
        got = model.excited_steps(cfg, v, phi, lowers, steps, np.float64)
        a, b = wo.ab(cfg, v)
        want = phi.copy()
        wo.evolve(cfg, wnum, a, b, want, lowers, steps)
        err = float(np.max(np.abs(got - want)))
        print("member", k, "ext", ext, "wnum", wnum, "max|dphi|", err)
        assert err <= 1e-13, (k, err)
        only = phi.copy()
        wo.orthogonalise(wnum, only, lowers)
        assert float(np.max(np.abs(model.orthogonalise(phi, lowers, np.float64) - only))) <= 1e-13, k


def test_chain_model_rounds_where_it_says(wo):
    """float storage: every result of the chain is a float, and it is not the double chain rounded once at the end"""
    cfg, v, phi = model.member_inputs(wo, 0, model.EXCITED_SHAPES[0], 1)
    lowers = model.stored_states(cfg, 0, 2)
    f = model.excited_steps(cfg, v, phi, lowers, 2, np.float32)
    d = model.excited_steps(cfg, v, phi, lowers, 2, np.float64)
    assert np.array_equal(f, ref.r32(f))
    assert not np.array_equal(f, ref.r32(d))
    assert float(np.max(np.abs(f - d))) < 8 * model.spacing_u(f)
