"""Batched excited states on the host: the new wafer_batch_* calls are declared, exported, bound and mirrored in the Rust
source with matching argument counts, and wafer_amd.Batch checks its arguments before any device call."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_CALLS = {
    "wafer_batch_load_state": 4, "wafer_batch_download_state": 4, "wafer_batch_push_state": 2, "wafer_batch_num_states": 2,
    "wafer_batch_clear_states": 2, "wafer_batch_clone_state_to_phi": 3, "wafer_batch_orthogonalise": 3, "wafer_batch_norm2": 2,
    "wafer_batch_evolve_state": 4, "wafer_batch_solve_state": 11,
}
NEW_METHODS = ["load_state", "download_state", "push_state", "num_states", "clear_states", "clone_state_to_phi", "orthogonalise",
               "norm2", "solve_state"]


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


def _count(args):
    return len([a for a in args.split(",") if a.strip() and a.strip() != "void"])


def test_state_calls_are_declared_exported_bound_and_mirrored(wa):
    from wafer_amd import engine
    header = open(os.path.join(ROOT, "include", "wafer_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = dict(re.findall(r"\bint\s*(wafer_batch_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header))
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    lib = wa.load_library()
    for name, nargs in NEW_CALLS.items():
        assert name in decls, name
        assert _count(decls[name]) == nargs, (name, decls[name])
        assert name in engine.EXPORTS, name
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
        m = re.search(r"pub fn %s\s*\((.*?)\)\s*->" % name, rust, flags=re.S)
        assert m, name
        assert _count(m.group(1)) == nargs, (name, m.group(1))
    # wafer_batch_solve_state is wafer_batch_solve with wnum after the batch
    assert _count(decls["wafer_batch_solve"]) + 1 == NEW_CALLS["wafer_batch_solve_state"]
    assert re.search(r"#define\s+WAFER_ABI_VERSION\s+1\b", header)


def test_batch_has_the_state_methods(wa):
    import inspect
    for name in NEW_METHODS:
        assert callable(getattr(wa.Batch, name, None)), name
    ev = inspect.signature(wa.Batch.evolve).parameters
    assert list(ev)[:4] == ["self", "steps", "active", "wnum"]
    assert ev["wnum"].default == 0 and ev["active"].default is None   # the default is today's ground-state call
    assert list(inspect.signature(wa.Batch.solve_state).parameters)[:4] == ["self", "wnum", "tolerance", "screen_update"]


@pytest.fixture
def unbound(wa):
    """a Batch that never reached the device: what the argument checks see is the member list alone"""
    b = object.__new__(wa.Batch)
    b.members = [wa.Params(16, 16, 16, dn=0.2, dt=0.004, max_states=2), wa.Params(16, 16, 16, dn=0.2, dt=0.002, max_states=3)]

    class _NoDevice:
        def __getattr__(self, name):
            raise AssertionError("argument check missing: %s reached the library" % name)
    b._L = _NoDevice()
    b._h = None
    return b


def test_batch_state_arguments_are_checked_before_the_device(unbound):
    b = unbound
    with pytest.raises(ValueError, match="shape"):
        b.load_state(0, 0, np.zeros((16, 16, 16)))       # the work shape, not the padded one
    with pytest.raises(ValueError, match="member"):
        b.load_state(2, 0, np.zeros((18, 18, 18)))
    with pytest.raises(ValueError, match="member"):
        b.download_state(-1, 0)
    for call in (lambda w: b.evolve(5, wnum=w), lambda w: b.orthogonalise(w), lambda w: b.solve_state(w, 1e-9, 100)):
        with pytest.raises(ValueError, match="wnum"):
            call(4)                                      # no member can hold four states
        with pytest.raises(ValueError, match="wnum"):
            call(-1)
    for call in (lambda a: b.evolve(5, active=a, wnum=1), lambda a: b.orthogonalise(1, active=a), lambda a: b.push_state(a),
                 lambda a: b.clear_states(a), lambda a: b.clone_state_to_phi(0, active=a)):
        with pytest.raises(ValueError, match="one entry per member"):
            call([1, 0, 1])
