"""Set-up of many batch members at once, without a GPU: the six entry points are declared, exported and mirrored and refuse a null
batch; the name-to-enum helper of Batch.set_potentials / set_initial_conditions; the numpy model of the range check
(tests/batch_setup_model.py) on hand-made arrays; and wafer_amd.sweep's batched=True against a batch that only records calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import batch_setup_model as model
from tests.test_sweep_inputs_plan import Recorder, make_runs, save

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"wafer_batch_set_potentials_builtin": 3, "wafer_batch_set_initial_conditions": 4, "wafer_batch_download_array": 4,
         "wafer_batch_get_potsub": 4, "wafer_batch_diag_member": 4, "wafer_batch_diag_setup_counts": 3}


@pytest.fixture(scope="module")
def lib():
    import wafer_amd
    return wafer_amd.load_library()


# ---- the ABI --------------------------------------------------------------------------------------------------------------------
def test_the_six_entry_points_are_declared_exported_and_bound(lib):
    from wafer_amd import engine
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wafer_hip.h")).read(), flags=re.S)
    decls = dict(re.findall(r"\bint\s*(wafer_batch_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header))
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name, arity in NAMES.items():
        assert name in decls, name
        assert decls[name].count(",") + 1 == arity, name
        assert hasattr(lib, name), name
        assert name in engine.EXPORTS and len(getattr(lib, name).argtypes) == arity, name
        m = re.search(r"pub fn %s\s*\((.*?)\)\s*->" % name, rust, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == arity, name
    assert lib.wafer_abi_version() == 1


def test_a_null_batch_is_refused(lib):
    one, buf = (C.c_int * 1)(0), C.create_string_buffer(64)
    seeds, out, k, s = (C.c_uint64 * 1)(0), (C.c_double * 1)(0), C.c_int(0), C.c_double(0)
    n, r = C.c_uint64(0), C.c_uint64(0)
    calls = [lambda: lib.wafer_batch_set_potentials_builtin(None, None, one),
             lambda: lib.wafer_batch_set_initial_conditions(None, None, one, seeds),
             lambda: lib.wafer_batch_download_array(None, 0, 0, out),
             lambda: lib.wafer_batch_get_potsub(None, 0, C.byref(k), C.byref(s)),
             lambda: lib.wafer_batch_diag_member(None, 0, buf, len(buf)),
             lambda: lib.wafer_batch_diag_setup_counts(None, C.byref(n), C.byref(r))]
    for call in calls:
        assert call() == -1   # WAFER_ERR_INVALID
        assert b"null" in lib.wafer_last_error()


# ---- names to enums ---------------------------------------------------------------------------------------------------------------
def test_names_become_enums_and_unlisted_entries_are_not_looked_at():
    from wafer_amd.engine import INITIAL_CONDITIONS, POTENTIALS, _enum_entries
    assert _enum_entries(["Harmonic", "Coulomb", 7], POTENTIALS, 3, None, "potential") == [9, 4, 7]
    assert _enum_entries(["Gaussian", "Boolean"], INITIAL_CONDITIONS, 2, None, "initial condition") == [1, 4]
    # an entry the mask leaves out may be anything: it is not read
    assert _enum_entries(["Harmonic", "no such thing", None, 77], POTENTIALS, 4, np.array([1, 0, 0, 0], dtype=np.uint8), "potential") == [9, 0, 0, 77]
    assert _enum_entries([99, "FromFile"], POTENTIALS, 2, None, "potential") == [99, 12]   # ints go through: the library checks them
    with pytest.raises(ValueError, match="member 1: unknown potential 'Harmonik'"):
        _enum_entries(["Harmonic", "Harmonik"], POTENTIALS, 2, None, "potential")
    with pytest.raises(ValueError, match="one entry per member"):
        _enum_entries(["Harmonic"], POTENTIALS, 2, None, "potential")
    with pytest.raises(ValueError, match="one entry per member"):
        _enum_entries(["Harmonic"] * 3, POTENTIALS, 2, None, "potential")


# ---- the model ------------------------------------------------------------------------------------------------------------------
def bits(x: float) -> int:
    return int(np.array([x]).view(np.uint64)[0])


def test_model_range_words_and_their_bounds():
    v = np.zeros((5, 4, 3))
    assert model.range_words(v, 0.01) == (bits(1.0), bits(1.0)) and model.in_range(v, 0.01)
    v[1, 2, 1] = -50.0                                         # 1 + 0.01 * -50 / 2 = 0.75
    assert model.range_words(v, 0.01) == (bits(0.75), bits(1.0))
    v[2, 2, 2] = np.nan
    lo, hi = model.range_words(v, 0.01)
    assert lo == bits(0.75) and hi > bits(np.inf) and not model.in_range(v, 0.01)      # a NaN sorts above +inf
    v[2, 2, 2] = -np.nan
    assert not model.in_range(v, 0.01)                         # fabs clears its sign: still above +inf, not below the minimum
    # the upper bound is exclusive: dt = 2 makes dt * v / 2 == v exactly, and 1 + 2^400 rounds to 2^400
    v = np.zeros((3, 3, 3))
    v[1, 1, 1] = 2.0 ** 400
    assert model.range_words(v, 2.0) == (bits(1.0), bits(2.0 ** 400)) and not model.in_range(v, 2.0)
    v[1, 1, 1] = np.nextafter(2.0 ** 400, 0.0)
    assert model.in_range(v, 2.0)
    v[1, 1, 1] = -(2.0 ** 400)                                 # fabs: the same word
    assert model.range_words(v, 2.0)[1] == bits(2.0 ** 400) and not model.in_range(v, 2.0)
    # the lower bound is exclusive too.  Through V the value 2^-400 itself cannot arise (1 + t is a multiple of 2^-53 for t near -1:
    # the smallest results are 0 and 2^-53), so it is tested on the words, and through V its nearest neighbours are
    assert not model.words_in_range(bits(2.0 ** -400), bits(1.0))
    assert model.words_in_range(bits(np.nextafter(2.0 ** -400, 1.0)), bits(1.0))
    assert not model.words_in_range(bits(1.0), bits(2.0 ** 400)) and not model.words_in_range(bits(1.0), bits(np.nan))
    v[1, 1, 1] = -1.0                                          # 1 + -1 = 0
    assert model.range_words(v, 2.0)[0] == bits(0.0) and not model.in_range(v, 2.0)
    v[1, 1, 1] = np.nextafter(-1.0, 0.0)                       # 2^-53
    assert model.range_words(v, 2.0)[0] == bits(2.0 ** -53) and model.in_range(v, 2.0)


def test_model_mirror_compares_bits_on_work_cells_only():
    ext = 1
    v = np.zeros((6, 7, 5))                                    # work 4 x 5 x 3: a middle row in y
    v[1:-1, 1:-1, :] = np.random.default_rng(0).standard_normal((4, 1, 5)) * np.ones((1, 5, 1))
    assert model.y_symmetric(v, ext)
    w = v.copy()
    w[2, 0, 1] = 9.0                                           # the frame is not compared
    w[0, 3, 1] = 9.0
    assert model.y_symmetric(w, ext)
    w = v.copy()
    w[2, 3, 0] = 7.0                                           # the middle row mirrors onto itself, on a frame PLANE too
    assert model.y_symmetric(w, ext)
    w[2, 2, 0] = 7.0                                           # ... but its neighbour does not
    assert not model.y_symmetric(w, ext)
    w = v.copy()
    w[3, 1, 2], w[3, 5, 2] = 0.0, -0.0                         # -0.0 against 0.0 in mirrored cells: different bits
    assert w[3, 1, 2] == w[3, 5, 2] and not model.y_symmetric(w, ext)
    w[3, 1, 2] = -0.0
    assert model.y_symmetric(w, ext)
    w[3, 1, 2] = w[3, 5, 2] = np.nan                           # the same NaN on both sides: the same bits
    assert model.y_symmetric(w, ext)
    # the SevenPoint frame is three cells wide
    v3 = np.zeros((10, 12, 9))
    v3[3:-3, 3:-3, :] = 1.5
    v3[1, 2, 4] = 3.0
    assert model.y_symmetric(v3, 3) and not model.y_symmetric(v3, 1)


def test_model_sources_alone_yield_every_outcome():
    """the sources of tests/test_gpu_batch_setup.py through the oracle's trilerp_resize onto that file's shapes: the model must say
    in-range and out-of-range, symmetric and not, on every stencil and storage type -- before any GPU is asked"""
    from oracle import wafer_oracle as wo
    wo.build()
    src = model.sources()
    for ext in (1, 3):
        for dtype in ("f64", "f32"):
            seen_range, seen_sym = set(), set()
            for shape, dt in (((70, 9, 5), 0.004), ((12, 10, 7), 0.01), ((33, 6, 12), 0.003)):
                padded = tuple(n + 2 * ext for n in shape)
                for name, s in src.items():
                    v = np.zeros(padded)
                    with np.errstate(all="ignore"):
                        v[ext:-ext, ext:-ext, ext:-ext] = wo.trilerp_resize(s, shape, basis=padded)
                    v = model.stored(v, dtype)
                    r, y = model.in_range(v, dt), model.y_symmetric(v, ext)
                    seen_range.add(r)
                    seen_sym.add(y)
                    if name == "flat":
                        assert r and y, (ext, dtype, shape)
                    if name in ("nan", "huge"):
                        assert not r, (name, ext, dtype, shape)
                    if name == "skew":
                        assert r and not y, (ext, dtype, shape)
            assert seen_range == {True, False} and seen_sym == {True, False}


# ---- the sweep's calls ------------------------------------------------------------------------------------------------------------
def specs():
    return [dict(potential="Harmonic", wavemax=1), dict(n=(16, 20, 28)), dict(potential="FullCornell", init_condition="Gaussian"),
            dict(n=(12, 10, 14), potential="Coulomb", init_condition="Constant"), dict(n=(9, 9, 9))]


def test_batched_set_up_is_one_call_with_names_and_mask(tmp_path):
    from wafer_amd import sweep
    d = tmp_path / "in"
    save(d, "potential", (16, 20, 28))
    runs = make_runs(specs(), [d] * 5)
    b = Recorder()
    sweep.set_up_batch(b, runs, batched=True)
    assert [(c[1], c[2]) for c in b.named("set_potentials")] == \
        [((["Harmonic", "NoPotential", "FullCornell", "Coulomb", "NoPotential"],), (1, 0, 1, 1, 0))]
    assert not b.named("set_potential")
    # file-borne inputs are grouped as before: run 1 has the file's size, run 4 is resampled
    assert [c[1][0] for c in b.named("set_potential_host")] == [1]
    assert [(c[1], c[2], c[3]) for c in b.named("resample_potential")] == [(((16, 20, 28),), (0, 0, 0, 0, 1), dict(basis="padded"))]
    names = [c[0] for c in b.calls]
    assert names.index("set_potentials") < min(names.index("set_potential_host"), names.index("resample_potential"))
    # batched=False: today's calls, and the same file-borne calls
    old, dflt = Recorder(), Recorder()
    sweep.set_up_batch(old, runs, batched=False)
    sweep.set_up_batch(dflt, runs)
    assert old.calls == dflt.calls
    assert [c[1] for c in old.named("set_potential")] == [(0, "Harmonic"), (2, "FullCornell"), (3, "Coulomb")] and not old.named("set_potentials")
    assert [c for c in old.calls if c[0] != "set_potential"] == [c for c in b.calls if c[0] != "set_potentials"]
    # every potential from a file: no call at all
    only_files = make_runs([dict(), dict(n=(16, 20, 28))], [d] * 2)
    b = Recorder()
    sweep.set_up_batch(b, only_files, batched=True)
    assert not b.named("set_potentials") and not b.named("set_potential")


def test_batched_start_of_a_phase_is_one_call_with_names_seeds_and_mask(tmp_path):
    from wafer_amd import sweep
    d = tmp_path / "in"
    save(d, "wavefunction_0", (9, 9, 9))
    sp = specs()
    sp[4] = dict(n=(9, 9, 9), init_condition="FromFile")      # its start comes from the file, copied
    runs = make_runs(sp, [tmp_path / "none"] * 4 + [d])
    b = Recorder()
    sweep.start_phase(b, runs, None, 0, seed=3, batched=True)
    calls = b.named("set_initial_conditions")
    assert [(c[1], c[2], c[3]) for c in calls] == \
        [((["Boolean", "Boolean", "Gaussian", "Constant", "Boolean"],), (1, 1, 1, 1, 0), dict(seeds=[3, 3, 3, 3, 3]))]
    assert not b.named("set_initial_condition")
    assert [c[1] for c in b.named("upload_phi")] == [(4, (11, 11, 11))] and len(b.named("symmetrise")) == 1
    names = [c[0] for c in b.calls]
    assert names.index("set_initial_conditions") < names.index("upload_phi") < names.index("symmetrise")
    old, dflt = Recorder(), Recorder()
    sweep.start_phase(old, runs, None, 0, seed=3, batched=False)
    sweep.start_phase(dflt, runs, None, 0, seed=3)
    assert old.calls == dflt.calls
    assert [(c[1], c[3]) for c in old.named("set_initial_condition")] == \
        [((0, "Boolean"), dict(seed=3)), ((1, "Boolean"), dict(seed=3)), ((2, "Gaussian"), dict(seed=3)), ((3, "Constant"), dict(seed=3))]
    assert not old.named("set_initial_conditions")
    assert [c for c in old.calls if c[0] != "set_initial_condition"] == [c for c in b.calls if c[0] != "set_initial_conditions"]
    # phase 1: only run 0 takes part and it clones its state 0 -- nothing is generated, so no call
    b = Recorder()
    sweep.start_phase(b, runs, None, 1, seed=3, batched=True)
    assert not b.named("set_initial_conditions") and [(c[1], c[2]) for c in b.named("clone_state_to_phi")] == [((0,), (1, 0, 0, 0, 0))]


def test_the_flag_reaches_run_batch(monkeypatch, tmp_path, capsys):
    from wafer_amd import sweep
    seen = []
    monkeypatch.setattr(sweep, "run_batch", lambda plan, runs, seed, progress, batched=False: seen.append(batched) or (0, 0))
    monkeypatch.setattr(sweep, "load_config", lambda p: make_runs([dict(potential="Harmonic")], ["x"])[0].cfg)
    (tmp_path / "a.yaml").write_text("project_name: p\n")
    for k, extra in enumerate(([], ["--batched-setup"])):
        sweep.main(["-c", str(tmp_path / "a.yaml"), "--output-dir", str(tmp_path / f"out{k}"), "--seed", "1", *extra])
    capsys.readouterr()
    assert seen == [False, True]
