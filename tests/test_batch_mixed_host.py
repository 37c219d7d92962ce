"""Mixed-shape batches (wafer_batch_create_mixed, Batch(members, mixed_shapes=True)) on the host: the entry points are declared,
exported and mirrored, and validation -- which runs before any HIP call, so without a GPU -- lets nx, ny, nz differ and still
names the member and the field for everything else."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wafer_batch_create_mixed", "wafer_batch_num_shapes")


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_mixed_entry_points_are_declared_exported_and_bound(wa):
    from wafer_amd import engine
    header = open(os.path.join(ROOT, "include", "wafer_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = dict(re.findall(r"\bint\s*(wafer_batch_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header))
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    lib = wa.load_library()
    for name in NEW:
        assert name in decls, name
        assert hasattr(lib, name), name
        assert name in engine.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
        m = re.search(r"pub fn %s\s*\((.*?)\)\s*->" % name, rust, flags=re.S)
        assert m, name
        n_c = len([a for a in decls[name].split(",") if a.strip()])
        n_rs = len([a for a in m.group(1).split(",") if a.strip()])
        assert n_c == n_rs == len(getattr(lib, name).argtypes), (name, n_c, n_rs)
    # the ABI is extended, not changed
    assert re.search(r"#define\s+WAFER_ABI_VERSION\s+1\b", header)


def P(wa, nx=16, ny=16, nz=16, **kw):
    base = dict(dn=0.2, dt=0.004)
    base.update(kw)
    return wa.Params(nx, ny, nz, **base)


def test_mixed_shapes_pass_validation(wa):
    members = [P(wa, 16, 16, 16), P(wa, 17, 16, 16), P(wa, 16, 20, 12)]
    if _has_gpu():
        with wa.Batch(members, mixed_shapes=True) as b:
            assert b.num_shapes() == 3 and len(b) == 3
        return
    with pytest.raises(wa.WaferError) as e:
        wa.Batch(members, mixed_shapes=True)
    assert e.value.code == -2, str(e.value)   # WAFER_ERR_HIP: validation passed, creation then needs the device


@pytest.mark.parametrize("bad,needle", [
    (dict(central_difference=2), "central_difference"),
    (dict(dtype="f32"), "dtype"),
    (dict(device=1), "device"),
    (dict(halo_depth=2), "halo_depth"),
    (dict(z_count=8), "z_count"),
    (dict(dt=0.1), "LargeDt"),
])
def test_mixed_batch_still_rejects_a_bad_member_naming_it(wa, bad, needle):
    members = [P(wa, 16, 16, 16), P(wa, 17, 16, 16, dt=0.002), P(wa, 16, 20, 12, **bad)]
    with pytest.raises(wa.WaferError) as e:
        wa.Batch(members, mixed_shapes=True)
    assert e.value.code == -1   # WAFER_ERR_INVALID
    assert "member 2" in str(e.value) and needle in str(e.value), str(e.value)


def test_mixed_batch_rejects_an_empty_list(wa):
    with pytest.raises(wa.WaferError) as e:
        wa.Batch([], mixed_shapes=True)
    assert e.value.code == -1


def test_plain_batch_still_rejects_a_differing_shape(wa):
    members = [P(wa), P(wa, dt=0.002), P(wa, nx=17)]
    for kw in ({}, dict(mixed_shapes=False)):
        with pytest.raises(wa.WaferError) as e:
            wa.Batch(members, **kw)
        assert e.value.code == -1
        assert "member 2" in str(e.value) and "nx" in str(e.value)
