"""The one-pass form of the batched excited step (wafer_batch_set_gs_variant) on the host: the three new calls across the header,
the library, the ctypes mirror and the Rust source, and the numpy model of tests/batch_onepass_model.py held to the oracle (double
storage) and to its own perturbed self (float storage: the bar tests/test_gpu_batch_onepass.py applies to the GPU)."""
import os
import re

import numpy as np
import pytest

from tests import batch_fp32_model as chain
from tests import batch_onepass_model as onepass
from tests import fp32_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["wafer_batch_set_gs_variant", "wafer_batch_diag_gs", "wafer_batch_diag_gs_steps"]
FLOAT_SHAPES = onepass.FLOAT_SHAPES     # of tests/test_gpu_batch_onepass.py
NM = len(chain.MEMBERS)


@pytest.fixture(scope="module")
def wo():
    from oracle import wafer_oracle
    wafer_oracle.build()
    return wafer_oracle


# ---- 1. the surface ---------------------------------------------------------------------------------------------------------------
def test_the_three_calls_are_declared_exported_and_bound():
    import wafer_amd
    from wafer_amd import engine
    lib = wafer_amd.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wafer_hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in engine.EXPORTS and getattr(lib, name).argtypes is not None, name
        assert re.search(r"pub fn %s\s*\(" % name, rust), name
    for method in ("set_gs_variant", "gs_dispatch", "gs_steps"):
        assert callable(getattr(wafer_amd.Batch, method, None)), method


# ---- 2. double storage: the model is the oracle's excited-state evolve -----------------------------------------------------------------
def correlated_states(cfg, k, wnum):
    """each random state normalised, 0.4 x the first added, normalised again: pairwise overlaps of about 0.4"""
    out = []
    for l in chain.stored_states(cfg, k, wnum, storage=np.float64):
        l = l + (0.4 * out[0] if out else 0.0)
        out.append(np.ascontiguousarray(l / np.sqrt(np.sum(l * l))))
    return out


@pytest.mark.parametrize("store", ["random", "correlated"])
@pytest.mark.parametrize("wnum", [1, 2, 3, 4])
@pytest.mark.parametrize("ext", [1, 2, 3])
def test_model_with_double_storage_is_the_oracle(wo, ext, wnum, store):
    shape, steps = (33, 20, 11), 4
    for k in range(NM):
        cfg, v, phi = chain.member_inputs(wo, k, shape, ext)
        lowers = chain.stored_states(cfg, k, wnum, storage=np.float64) if store == "random" else correlated_states(cfg, k, wnum)
        if store == "correlated" and wnum > 1:
            assert 0.3 < float(np.sum(lowers[1] * lowers[0])) < 0.45
        got = onepass.excited_steps(cfg, v, phi, lowers, steps, np.float64)
        a, b = wo.ab(cfg, v)
        want = phi.copy()
        wo.evolve(cfg, wnum, a, b, want, lowers, steps)
        err = float(np.max(np.abs(got - want)))
        print("member", k, "ext", ext, "wnum", wnum, store, "max|dphi|", err)
        assert err <= 1e-13, (k, err)
        only = phi.copy()
        wo.orthogonalise(wnum, only, lowers)
        assert float(np.max(np.abs(onepass.orthogonalise(phi, lowers, np.float64) - only))) <= 1e-13, k


# ---- 3. float storage: the model against its perturbed self ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FLOAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("ext", [1, 2, 3])
@pytest.mark.parametrize("wnum", [1, 2, 3])
def test_float_model_moves_little_under_perturbed_scalars(wo, wnum, ext, shape):
    """D_ref <= 1 float spacing at max |phi| and at most 1 % of the work cells differing: the GPU file's bar,
    max(1, 4 D_ref) spacings and 1 % of the cells, then asks of the kernels what the model's own sensitivity allows"""
    for k in range(NM):
        cfg, _, out = onepass.float_models(wo, k, shape, ext, wnum)
        for what, (x, p) in out.items():
            u = chain.spacing_u(x)
            d_ref = float(np.max(np.abs(x - p))) / u
            flips = int(np.count_nonzero(chain.work(cfg, x) != chain.work(cfg, p)))
            print(shape, ext, wnum, "member", k, what, "D_ref", d_ref, "cells differing", flips, "of", cfg.nx * cfg.ny * cfg.nz)
            assert np.array_equal(x, ref.r32(x)), (k, what)
            assert d_ref <= 1.0, (k, what, d_ref)
            assert flips <= 0.01 * cfg.nx * cfg.ny * cfg.nz, (k, what, flips)


# ---- 4. a form of its own ----------------------------------------------------------------------------------------------------------------
def test_float_onepass_model_is_not_the_chain_model(wo):
    """it rounds phi once per step where the chain rounds it 1 + wnum times: some cell differs, by a few float spacings at most"""
    cfg, v, phi = chain.member_inputs(wo, 0, (33, 20, 11), 1)
    lowers = chain.stored_states(cfg, 0, 2)
    one = onepass.excited_steps(cfg, v, phi, lowers, 4, np.float32)
    seq = chain.excited_steps(cfg, v, phi, lowers, 4, np.float32)
    assert not np.array_equal(one, seq)
    assert float(np.max(np.abs(one - seq))) <= 8 * chain.spacing_u(seq)
