"""The generated Batch programs of tests/batch_sequences.py, checked on the CPU so that tests/test_gpu_batch_sequences.py cannot pass
vacuously: over the very seed list the GPU file runs, every program is valid against the generator's bookkeeping, HostModel runs it
end to end, every op kind occurs, refusals stay rare, and the transitions at which a Batch's kept state (Gram matrices, the member
table on the device, the workgroup tables, the views' flags, buffers made at first use) can go stale are all reached.  HostModel
itself is held to straight-line oracle calls on two hand-written programs."""
import functools

import numpy as np
import pytest

from tests import batch_sequences as bs
from tests.batch_sequences import KINDS, SEEDS, mk


@pytest.fixture(scope="module")
def wo():
    from oracle import wafer_oracle
    wafer_oracle.build()
    return wafer_oracle


def cases(kind):
    """the (seed, kind, ext) of tests/test_gpu_batch_sequences.py's cases (there each with every dtype: the program is the same)"""
    return [(seed, kind, ext) for seed in SEEDS[kind] for ext in bs.EXTS]


@functools.lru_cache(maxsize=None)
def prog_of(seed, kind, ext):
    return tuple(bs.program(seed, kind, ext)), tuple(bs.members(seed, kind, ext))


@functools.lru_cache(maxsize=None)
def trace_of(seed, kind, ext):
    from oracle import wafer_oracle
    prog, mems = prog_of(seed, kind, ext)
    return bs.run_model(wafer_oracle, list(prog), list(mems), ext)


def annotated(seed, kind, ext):
    """per op: (op, the members it concerns, the bookkeeping's copy of nst / step variant / gs variant BEFORE it); refused ops concern
    nobody"""
    prog, mems = prog_of(seed, kind, ext)
    book, out = bs.Book(list(mems), kind, ext), []
    for op in prog:
        out.append((op, [] if op.refused is not None else bs.touched(op, len(mems)), list(book.nst), book.step_variant, book.gs_variant))
        if op.refused is None:
            book.commit(op)
    return out


# ---- the programs themselves -----------------------------------------------------------------------------------------------------------
def test_the_same_arguments_give_the_same_program():
    for kind in KINDS:
        a, b = bs.program(3, kind, 2), bs.program(3, kind, 2, dtype="f32")
        assert repr(a) == repr(b) and a == b
        assert repr(a) != repr(bs.program(4, kind, 2))


@pytest.mark.parametrize("kind", KINDS)
def test_every_program_is_valid_and_the_model_runs_it(wo, kind):
    for seed, _, ext in cases(kind):
        prog, mems = prog_of(seed, kind, ext)
        assert bs.N_OPS <= len(prog) <= 1.6 * bs.N_OPS, (seed, len(prog))   # a program's agenda of motifs may run past N_OPS
        bs.check_valid(list(prog), list(mems), kind, ext)
        trace = trace_of(seed, kind, ext)
        assert len(trace) == len(prog)
        for (snaps, ret), op in zip(trace, prog):
            for m, snap in enumerate(snaps):   # nothing a later comparison would choke on: finite arrays, stores within capacity
                assert snap["nst"] <= mems[m].max_states
                assert snap["phi"] is None or np.all(np.isfinite(snap["phi"])), (seed, op, m)
                assert all(np.all(np.isfinite(s)) for s in snap["states"]), (seed, op, m)
        # the tiers the GPU file gives a program follow from its content: ground-only programs are the ones held to Contexts
        excited = any((op.name in ("evolve", "solve_state") and op.get("wnum")) or op.name == "orthogonalise" for op in prog if op.refused is None)
        assert excited == (not bs.ground_only(seed, kind)), seed
        # no stored state has a large norm (Gram-Schmidt against one would amplify rounding): the absolute bars were set for unit stores
        for snaps, _ in trace:
            for snap in snaps:
                for s in snap["states"]:
                    assert 1e-4 < float(np.sum(s * s)) < 20.0, (seed, float(np.sum(s * s)))


def test_programs_hold_about_forty_ops():
    for kind in KINDS:
        lengths = [len(prog_of(seed, kind, ext)[0]) for seed, _, ext in cases(kind)]
        assert bs.N_OPS <= np.mean(lengths) <= 1.2 * bs.N_OPS, (kind, np.mean(lengths))


def allowed_ops(kind):
    if kind != "mixed":
        return set(bs.OP_NAMES)
    return set(bs.OP_NAMES) - set(bs.STATE_CALLS) - {"ritz_matrices", "rotate_states", "ritz", "set_gs_variant"}


@pytest.mark.parametrize("kind", KINDS)
def test_every_op_kind_occurs(kind):
    count = {name: 0 for name in allowed_ops(kind)}
    for seed, _, ext in cases(kind):
        for op in prog_of(seed, kind, ext)[0]:
            if op.refused is None:
                assert op.name in count, (seed, op)
                count[op.name] += 1
    assert all(c >= 3 for c in count.values()), {k: c for k, c in count.items() if c < 3}


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_are_rare_and_present(kind):
    total = 0
    for seed, _, ext in cases(kind):
        prog = prog_of(seed, kind, ext)[0]
        refused = [op for op in prog if op.refused is not None]
        assert 10 * len(refused) <= len(prog), (seed, len(refused), len(prog))
        assert all(op.refused in (bs.WAFER_ERR_INVALID, bs.WAFER_ERR_STATE) for op in refused)
        total += len(refused)
    assert total >= 3   # transition k; tests/batch_sequences.run_batch compares every member's whole state around each of them


def test_the_masks_vary():
    """None, one member only, and several"""
    for kind in KINDS:
        seen = set()
        for seed, _, ext in cases(kind):
            for op in prog_of(seed, kind, ext)[0]:
                if op.name in bs.MASKED:
                    seen.add("none" if op.active is None else "one" if sum(op.active) == 1 else "some")
        assert seen == {"none", "one", "some"}, (kind, seen)


def test_wnum_five_takes_the_sequential_form_under_the_one_pass_variant():
    hits = [(seed, kind) for kind in KINDS for seed, _, ext in cases(kind) for op, act, nst, sv, gv in annotated(seed, kind, ext)
            if op.name == "evolve" and op["wnum"] == 5 and gv == 1]
    assert hits


# ---- the transitions -----------------------------------------------------------------------------------------------------------------------
def excited_call(op):
    return op.refused is None and ((op.name == "evolve" and op["wnum"] > 0) or op.name == "orthogonalise")


def transitions(seed, kind, ext):
    """the tags of the transitions (a .. j) one program reaches"""
    an = annotated(seed, kind, ext)
    prog = [x[0] for x in an]
    B = len(prog_of(seed, kind, ext)[1])
    K = bs.fused_steps(ext)
    tags = set()
    everyone = lambda op: op.active is None  # noqa: E731
    for i in range(len(an) - 1):
        op, act, nst, sv, gv = an[i]
        nxt, nact, nnst, nsv, ngv = an[i + 1]
        if op.refused is not None or nxt.refused is not None:
            continue
        # a: a store change directly before a one-pass excited evolve or orthogonalise of a member it changed
        # (the Gram matrix holds products of pairs of states: but after clear_states and one push, the call has wnum >= 2 and reads
        # the state that changed)
        both = set(act) & set(nact)
        if excited_call(nxt) and ngv == 1 and nxt["wnum"] <= 4 and both:
            w = nxt["wnum"]
            if op.name == "push_state":
                if i > 0 and an[i - 1][0].name == "clear_states" and an[i - 1][0].refused is None and set(an[i - 1][1]) & both:
                    tags.add("a:clear_push")
                elif w >= 2 and any(nst[m] < w for m in both):
                    tags.add("a:push")
            elif op.name == "load_state" and op["idx"] < nst[op["i"]] and w >= 2 and op["idx"] < w:
                tags.add("a:overwrite")
            elif op.name == "resample_state" and w >= 2 and op["idx"] < w:
                tags.add("a:resample_state")
            elif op.name == "rotate_states" and w >= 2:
                tags.add("a:rotate_states")
        # b: some members' current buffer flipped (an odd number of launches under a mask, or a masked symmetrise), then a call over all
        flipped = (op.name == "evolve" and op["wnum"] == 0 and op.active is not None and sum(op.active) < B and op["steps"] % 2 == 1 and sv != 1) or \
                  (op.name == "symmetrise" and op.active is not None and sum(op.active) < B and any(op["constraints"][m] != "NotConstrained" for m in act))
        if flipped and everyone(nxt) and (nxt.name in ("observables", "norm2", "ritz_matrices") or (nxt.name == "evolve" and nxt["wnum"] == 0)):
            tags.add("b:" + nxt.name)
        # e: a pot_sub kind change directly before observables / ritz_matrices
        if op.name == "set_potsub" and i > 0 and an[i - 1][0].name == "set_potsub" and an[i - 1][0]["i"] == op["i"] and an[i - 1][0]["kind"] != op["kind"]:
            if nxt.name == "observables" or (nxt.name == "ritz_matrices" and op["i"] in nact):
                tags.add("e:" + nxt.name)
        # h: phi written by another call directly before a fused pass over it
        if op.name in bs.PHI_WRITERS and nxt.name == "evolve" and nxt["wnum"] == 0 and nsv == 1 and nxt["steps"] >= K and set(act) & set(nact):
            if op.name != "symmetrise" or any(op["constraints"][m] != "NotConstrained" for m in set(act) & set(nact)):
                tags.add("h:" + op.name)
    # c: evolve under A, under B != A, under A; and A under K = 1, then under the fused K
    ground = [(i, x) for i, x in enumerate(an) if x[0].name == "evolve" and x[0].refused is None and x[0]["wnum"] == 0]
    key = lambda op: tuple(1 if (op.active is None or op.active[m]) else 0 for m in range(B))  # noqa: E731
    for (i, a), (j, b), (k, c) in zip(ground, ground[1:], ground[2:]):
        if j == i + 1 and k == j + 1 and key(a[0]) == key(c[0]) != key(b[0]):
            tags.add("c:aba")
    for (i, a), (j, b) in zip(ground, ground[1:]):
        between = prog[i + 1:j]
        if key(a[0]) == key(b[0]) and a[3] != 1 and b[3] == 1 and b[0]["steps"] >= K and all(o.name == "set_step_variant" for o in between):
            tags.add("c:k1_then_fused")
    # d: per member: a closed-form V, an excited evolve, a V from the host, an excited evolve -- nothing else setting that V in between
    for m in range(B):
        stage = 0
        for op, act, *_ in an:
            if op.refused is not None or m not in act:
                continue
            if op.name in ("set_potential", "set_potentials"):
                name = op["pot"] if op.name == "set_potential" else op["names"][m]
                stage = 1 if name in bs.CLOSED_FORM else 0
            elif op.name in ("set_potential_host", "resample_potential"):
                stage = 3 if stage == 2 else 0
            elif op.name == "evolve" and op["wnum"] > 0:
                if stage == 1:
                    stage = 2
                elif stage == 3:
                    tags.add("d")
    # f: norm2, the first one-pass call, norm2 -- among the calls that use gs_partials
    users = [(op, gv) for op, act, nst, sv, gv in an if op.refused is None and (op.name in ("norm2", "orthogonalise", "solve_state") or (op.name == "evolve" and op["wnum"]))]
    first = next((k for k, (op, gv) in enumerate(users) if gv == 1 and op.name in ("evolve", "orthogonalise") and op["wnum"] <= 4), None)
    if first is not None and 0 < first < len(users) - 1 and users[first - 1][0].name == "norm2" and users[first + 1][0].name == "norm2":
        tags.add("f")
    # g: every store emptied, then filled, an excited evolve, ritz
    stage = 0
    for op, act, nst, sv, gv in an:
        if op.refused is not None:
            continue
        after = [0 if (op.name == "clear_states" and m in act) else n for m, n in enumerate(nst)]
        if op.name == "clear_states" and max(nst) > 0 and max(after) == 0:
            stage = 1
        elif stage == 1 and op.name in ("push_state", "load_state", "resample_state"):
            stage = 2
        elif stage == 2 and op.name == "evolve" and op["wnum"] > 0:
            stage = 3
        elif stage == 3 and op.name == "ritz":
            tags.add("g")
    # i: a ritz* call, then a later one with a larger k for the same member
    last = [0] * B
    for op, act, *_ in an:
        if op.refused is None and op.name in ("ritz_matrices", "ritz"):
            for m in act:
                if last[m] and op["ks"][m] > last[m]:
                    tags.add("i")
                last[m] = op["ks"][m]
    # j: a solve whose members stop at different blocks, directly before an evolve of all members
    trace = trace_of(seed, kind, ext)
    for i in range(len(prog) - 1):
        if prog[i].name == "solve" and prog[i + 1].name == "evolve" and prog[i + 1].active is None and prog[i + 1].refused is None:
            if len({len(r[0]) for r in trace[i][1]}) > 1:
                tags.add("j")
    if any(op.refused is not None for op in prog):
        tags.add("k")
    return tags


GROUND = {"b:observables", "b:norm2", "b:evolve", "c:aba", "c:k1_then_fused", "e:observables", "h:upload_phi", "h:resample_phi", "j", "k"}
STATES = GROUND | {"a:push", "a:clear_push", "a:overwrite", "a:resample_state", "a:rotate_states", "b:ritz_matrices", "d", "e:ritz_matrices", "f",
                   "g", "h:clone_state_to_phi", "i"}
REQUIRED = {"one_shape": STATES, "mixed": GROUND, "mixed_states": STATES}


@pytest.mark.parametrize("kind", KINDS)
def test_every_transition_is_reached(wo, kind):
    reached = set()
    exts = set()
    for seed, _, ext in cases(kind):
        reached |= transitions(seed, kind, ext)
        exts.add(ext)
    assert exts == {1, 2, 3}
    need = REQUIRED[kind] | {"h:symmetrise"}   # ext 3 is among the exts of every kind
    assert need <= reached, sorted(need - reached)


# ---- HostModel against straight-line oracle calls -----------------------------------------------------------------------------------------
def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_model_against_the_oracle_ground_state(wo):
    mem, ext = bs.Member((12, 16, 7), 0.25, 0.006, 1.5, 4), 3
    prog = [mk("set_potentials", names=("Coulomb",)), mk("upload_phi", i=0, phi=("frame0", 11, mem.shape, ext, 1.0)),
            mk("symmetrise", constraints=("AntisymAboutY",)), mk("evolve", steps=5, wnum=0), mk("norm2"), mk("normalise"),
            mk("set_potsub", i=0, kind=2, scalar=0.5, potsub=("normal", 12, mem.shape, 1.0)), mk("observables"),
            mk("resample_potential", src=("normal", 13, (5, 4, 3), 1.0), basis="work"), mk("evolve", steps=2, wnum=0), mk("observables")]
    trace = bs.run_model(wo, prog, [mem], ext)
    cfg = wo.Config(*mem.shape, ext=ext, potential="Coulomb", dn=mem.dn, dt=mem.dt, mass=mem.mass)
    v = wo.potential_generate(cfg)
    phi = bs.materialise(("frame0", 11, mem.shape, ext, 1.0))
    wo.symmetrise(cfg, "AntisymAboutY", phi)
    wo.evolve(cfg, 0, *wo.ab(cfg, v), phi, [], 5)
    n2 = wo.norm2(cfg, phi)
    assert trace[4][1][0] == n2
    wo.normalise(phi, n2)
    assert same(trace[5][0][0]["phi"], phi) and same(trace[5][0][0]["v"], v)
    sub = bs.materialise(("normal", 12, mem.shape, 1.0))
    assert trace[7][1][0] == wo.observables(cfg, v, phi, (2, 0.0, sub)) and trace[7][0][0]["potsub"] == (2, 0.0)
    v2 = np.zeros(cfg.padded_shape)
    v2[ext:-ext, ext:-ext, ext:-ext] = wo.trilerp_resize(bs.materialise(("normal", 13, (5, 4, 3), 1.0)), mem.shape, basis=mem.shape)
    wo.evolve(cfg, 0, *wo.ab(cfg, v2), phi, [], 2)
    assert same(trace[9][0][0]["phi"], phi) and same(trace[9][0][0]["v"], v2)
    assert trace[10][1][0] == wo.observables(cfg, v2, phi, (0, 0.0, None)) and trace[10][0][0]["potsub"] == (0, 0.0)


def test_model_against_the_oracle_states(wo):
    from tests import ritz_model
    mem, ext = bs.Member((20, 13, 9), 0.2, 0.004, 1.0, 4), 1
    s0, s1 = ("frame0", 21, mem.shape, ext, 0.02), ("frame0", 22, mem.shape, ext, 0.02)
    prog = [mk("set_potential", i=0, pot="Harmonic"), mk("set_initial_conditions", names=("Boolean",), seeds=(3,)),
            mk("load_state", i=0, idx=0, state=s0), mk("load_state", i=0, idx=1, state=s1), mk("evolve", steps=4, wnum=2),
            mk("push_state"), mk("rotate_states", coefs=(("rot", 5, 3),)), mk("clone_state_to_phi", idx=2),
            mk("resample_phi", src=("state", 0, 0), basis="padded"), mk("orthogonalise", wnum=1), mk("ritz_matrices", ks=(2,)),
            mk("clear_states"), mk("solve_state", wnum=0, tolerance=1e-2, screen_update=2, max_steps=6)]
    trace = bs.run_model(wo, prog, [mem], ext)
    cfg = wo.Config(*mem.shape, ext=ext, potential="Harmonic", dn=mem.dn, dt=mem.dt, mass=mem.mass)
    v = wo.potential_generate(cfg)
    a, b = wo.ab(cfg, v)
    phi = wo.initial_condition(cfg, "Boolean", 3)
    store = [bs.materialise(s0), bs.materialise(s1)]
    wo.evolve(cfg, 2, a, b, phi, store, 4)
    assert same(trace[4][0][0]["phi"], phi)
    store = ritz_model.rotate(store + [phi.copy()], bs.materialise(("rot", 5, 3)))
    assert trace[6][0][0]["nst"] == 3 and all(same(g, w) for g, w in zip(trace[6][0][0]["states"], store))
    assert same(trace[7][0][0]["phi"], store[2])
    phi = np.zeros(cfg.padded_shape)
    phi[ext:-ext, ext:-ext, ext:-ext] = wo.trilerp_resize(np.ascontiguousarray(store[0][ext:-ext, ext:-ext, ext:-ext]), mem.shape, basis=cfg.padded_shape)
    wo.orthogonalise(1, phi, store)
    assert same(trace[9][0][0]["phi"], phi)
    h, s = ritz_model.matrices(cfg, v, store[:2])
    assert same(trace[10][1][0][0], h) and same(trace[10][1][0][1], s)
    rows, conv = wo.solve(cfg, 0, v, a, b, phi, [], 1e-2, 2, max_steps=6)
    assert trace[12][1][0][0] == rows and trace[12][1][0][2] == conv
    assert same(trace[12][0][0]["phi"], phi) and trace[12][0][0]["nst"] == (1 if conv else 0)


def test_the_numpy_ritz_solve_diagonalises(wo):
    rng = np.random.default_rng(3)
    a = rng.standard_normal((4, 4))
    s = a @ a.T + 4 * np.eye(4)
    h = rng.standard_normal((4, 4))
    h = h + h.T
    evals, c = bs.ritz_solve(h, s)
    assert np.all(np.diff(evals) >= 0)
    assert np.allclose(c.T @ s @ c, np.eye(4), atol=1e-12) and np.allclose(c.T @ h @ c, np.diag(evals), atol=1e-12)


def test_a_failure_names_the_case_and_the_cell():
    prog = [mk("norm2"), mk("evolve", active=(1, 0), steps=3, wnum=0)]
    a = {"nst": 0, "potsub": (0, 0.0), "phi": np.zeros((2, 3, 4)), "v": None, "potsub_arr": None, "states": []}
    b = dict(a, phi=a["phi"].copy())
    b["phi"][1, 2, 3] = 1e-300
    msg = bs.describe((7, "mixed", 2, "f32"), prog, 1, 0, "T1", bs.compare_exact(b, a))
    for part in ("seed 7", "kind mixed", "ext 2", "dtype f32", "op 1", "evolve(steps=3, wnum=0, active=[1, 0])", "member 0", "phi", "(1, 2, 3)", "1e-300",
                 "norm2()", "--seed 7 --kind mixed"):
        assert part in msg, (part, msg)
    assert bs.compare_exact(a, dict(a, phi=a["phi"].copy())) is None
    assert bs.first_difference(0.0, -0.0) is not None   # bytes, not values
