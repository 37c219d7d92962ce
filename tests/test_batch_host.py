"""Batched ensembles (wafer_batch_*) on the host: the declarations are exported and mirrored, and wafer_batch_create
validates every member -- naming it -- before any HIP call, so these run without a GPU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


def _batch_decls():
    header = open(os.path.join(ROOT, "include", "wafer_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    return re.findall(r"\b(?:int|const char \*)\s*(wafer_batch_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header)


def test_batch_entry_points_are_declared_exported_and_bound(wa):
    from wafer_amd import engine
    decls = _batch_decls()
    names = {n for n, _ in decls}
    assert {"wafer_batch_create", "wafer_batch_destroy", "wafer_batch_evolve", "wafer_batch_observables",
            "wafer_batch_normalise", "wafer_batch_solve", "wafer_batch_kernel_name"} <= names
    lib = wa.load_library()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name, args in decls:
        assert hasattr(lib, name), name
        assert name in engine.EXPORTS, name
        m = re.search(r"pub fn %s\s*\((.*?)\)\s*->" % name, rust, flags=re.S)
        assert m, name
        n_c = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        n_rs = len([a for a in m.group(1).split(",") if a.strip()])
        assert n_c == n_rs, (name, n_c, n_rs)


def _params(wa, **kw):
    base = dict(nx=16, ny=16, nz=16, dn=0.2, dt=0.004)
    base.update(kw)
    return wa.Params(**base)


@pytest.mark.parametrize("bad,needle", [
    (dict(nx=17), "nx"),
    (dict(central_difference=2), "central_difference"),
    (dict(device=1), "device"),
    (dict(dtype="f32"), "dtype"),
    (dict(z_count=8), "z_count"),
    (dict(dt=0.1), "LargeDt"),
    (dict(halo_depth=2), "halo_depth"),
])
def test_batch_rejects_a_bad_member_naming_it(wa, bad, needle):
    members = [_params(wa), _params(wa, dt=0.002), _params(wa, **bad)]
    with pytest.raises(wa.WaferError) as e:
        wa.Batch(members)
    assert e.value.code == -1   # WAFER_ERR_INVALID
    assert "member 2" in str(e.value) and needle in str(e.value)


def test_batch_rejects_an_empty_list(wa):
    with pytest.raises(wa.WaferError) as e:
        wa.Batch([])
    assert e.value.code == -1


def test_batch_dt_rule_can_be_skipped_per_member(wa):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    # the skip flag lets the member through validation; creation then needs the device
    with pytest.raises(wa.WaferError) as e:
        wa.Batch([_params(wa), _params(wa, dt=0.1, skip_dt_check=True)])
    assert e.value.code == -2


def test_valid_batch_fails_loudly_without_gpu(wa):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(wa.WaferError) as e:
        wa.Batch([_params(wa), _params(wa, dt=0.002, mass=2.0)])
    assert e.value.code == -2   # WAFER_ERR_HIP: there is no CPU path
