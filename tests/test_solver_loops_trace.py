"""wafer_amd.engine.block_solve_loop and filtered_solve_loop replayed on scripted callables: every call they make on their callables
(its `going` list and arguments, in order) and every field of the dicts they return, against tests/golden/solver_loop_traces.json.

The fixture was recorded from the two loops as they stood BEFORE they became callers of one driver (the commit "Chebyshev-filtered
subspace iteration on the stored states"), with trace() below.  To reproduce it, put a checkout of that commit first on PYTHONPATH
and run this file with the output path as its argument: it imports wafer_amd.engine from there and hands its two loops to trace().
The loops only subtract, take abs and max of the tabulated doubles, so the comparison is on float.hex strings and exact.

The members of the scenarios reach every status of both loops: converged at different blocks, max_blocks, dependent at the first
Ritz step (block 0 of the filter, block 1 of the plain loop) and at a later block, both no-interval cases, members with k = 0 and
None, guard 1 and 2 -- and every refusal of the arguments."""
import json
import os
import sys

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_loop_traces.json")
OK, DEPENDENT = 0, -4   # WAFER_OK, WAFER_ERR_STATE: what a ritz callable answers


def hexes(a):
    return None if a is None else [float(x).hex() for x in np.asarray(a, dtype=np.float64).ravel()]


def evals_of(base, amp, n):
    """the n-th Ritz step's values of a member: base_j + amp_j 2^-n (exact doubles for the bases and amplitudes below)"""
    return [b + a * 0.5 ** n for b, a in zip(base, amp)]


# A member: k, the Ritz values' (base, amp), `dep`: the Ritz step (counted from 0 per member) that fails, `ub`, and rho_j = floor_j +
# 2^-(rate n) at the member's n-th residual call, n = 1, 2, ...  Ritz steps return RITZ_MAX-long rows (the loops cut them to k), as Batch.ritz does not
# but a backend may.
def member(k, base=(), amp=(), dep=None, ub=100.0, floor=(), rate=9):
    return dict(k=k, base=list(base), amp=list(amp), dep=dep, ub=ub, floor=list(floor), rate=rate)


BLOCK_MEMBERS = [
    member(2, (1.0, 2.5), (0.0, 0.0)),                       # converged at block 2: the values stand still
    member(3, (0.5, 1.5, 3.25), (0.0, 0.015625, 0.03125)),   # converged at block 3 (tolerance 2^-6: the diffs are 2^-6, then 2^-7)
    member(2, (1.0, 2.0), (0.0, 64.0)),                      # max_blocks
    member(2, (1.0, 2.0), (0.0, 0.0), dep=0),                # dependent at block 1
    member(3, (1.0, 2.0, 3.0), (8.0, 8.0, 8.0), dep=2),      # dependent at block 3
    member(0),
    member(None),
    member(1, (7.0,), (0.0625,)),                            # converged at block 4, the last one: the diffs are 2^-5, 2^-6, 2^-7
]
FILTER_MEMBERS = [
    member(3, (1.0, 2.0, 3.0), (0.0, 0.0, 0.0), floor=(0.0, 0.0, 0.5)),                 # converged at block 1 (guard 1 and 2)
    member(4, (0.5, 1.0, 1.5, 2.0), (0.25, 0.25, 0.25, 0.25), floor=(0.0, 0.0, 2.0 ** -9, 1.0), rate=3),   # guard 1: block 4; guard 2: block 3
    member(3, (1.0, 2.0, 3.0), (1.0, 1.0, 1.0), floor=(0.0, 1.0, 1.0)),                 # max_blocks (guard 1); guard 2: block 1
    member(3, (1.0, 2.0, 3.0), (0.0, 0.0, 0.0), dep=0, floor=(0.0, 0.0, 0.0)),          # dependent at block 0
    member(3, (1.0, 2.0, 3.0), (0.5, 0.5, 0.5), dep=2, floor=(1.0, 1.0, 1.0)),          # dependent at block 2
    member(3, (4.0, 4.0, 4.0), (0.0, 0.0, 0.0), floor=(1.0, 1.0, 1.0)),                 # evals[k - 1] <= evals[0] at block 1
    member(4, (1.0, 2.0, 3.0, 4.0), (0.0, 0.0, 0.0, 64.0), ub=30.0, floor=(1.0, 1.0, 1.0, 1.0)),   # 4 + 64 >= 30 at block 1
    member(4, (1.0, 2.0, 3.0, 28.0), (0.0, 0.0, 0.0, -16.0), ub=21.0, floor=(1.0, 1.0, 1.0, 1.0)),  # 12, 20, then 24 >= 21 at block 3
    member(0),
    member(None),
]


class Script:
    """the callables of both loops on a list of members, with the log of what they were called with"""

    def __init__(self, members):
        self.members, self.log = members, []
        self.n_ritz = [0] * len(members)
        self.n_resid = [0] * len(members)

    def step(self, going, n):
        self.log.append(["step", type(going).__name__, list(going), n])

    def bound(self, going):
        self.log.append(["bound", type(going).__name__, list(going)])
        return {m: self.members[m]["ub"] for m in going}

    def filt(self, going, degree, iv):
        self.log.append(["filt", type(going).__name__, list(going), degree, {str(m): hexes(iv[m]) for m in sorted(iv)}])

    def ritz(self, going):
        self.log.append(["ritz", type(going).__name__, list(going)])
        out = {}
        for m in going:
            e, n = self.members[m], self.n_ritz[m]
            self.n_ritz[m] += 1
            out[m] = (DEPENDENT, None) if e["dep"] == n else (OK, evals_of(e["base"], e["amp"], n) + [-1.0] * (8 - e["k"]))
        return out

    def residuals(self, going, theta):
        self.log.append(["residuals", type(going).__name__, list(going), {str(m): hexes(theta[m]) for m in sorted(theta)}])
        out = {}
        for m in going:
            e, n = self.members[m], self.n_resid[m]
            self.n_resid[m] += 1
            out[m] = [f + 0.5 ** (e["rate"] * (n + 1)) for f in e["floor"]] if e["floor"] else [0.5 ** (n + 1)] * e["k"]
        return out


def plain(o):
    """a member's result with every float as float.hex"""
    if o is None:
        return None
    d = {key: o[key] for key in ("status", "message", "blocks", "steps")}
    d.update({key: hexes(o[key]) for key in ("evals", "diff", "rho")})
    d["rows"] = [dict(block=r["block"], steps=r["steps"], evals=hexes(r["evals"]), diff=hexes(r["diff"]), rho=hexes(r["rho"])) for r in o["rows"]]
    assert sorted(o) == sorted(d), sorted(o)
    return d


def run(loop, which, members, *args):
    s = Script(members)
    ks = [e["k"] for e in members]
    try:
        out = loop(s.step, s.ritz, s.residuals, ks, *args) if which == "block" else loop(s.bound, s.filt, s.ritz, s.residuals, ks, *args)
        return dict(loop=which, args=[repr(a) for a in args], calls=s.log, result=[plain(o) for o in out])
    except ValueError as e:
        return dict(loop=which, args=[repr(a) for a in args], calls=s.log, raises=str(e))


def trace(block_solve_loop, filtered_solve_loop):
    """every scenario on the two loops -> what the fixture holds"""
    nobody = [member(0), member(None)]
    return [
        run(block_solve_loop, "block", BLOCK_MEMBERS, 2.0 ** -6, 3, 4),            # tolerance, steps_per_block, max_blocks
        run(block_solve_loop, "block", BLOCK_MEMBERS, 2.0 ** -6, 1, 1),
        run(block_solve_loop, "block", nobody, 1e-3, 2, 5),
        run(block_solve_loop, "block", BLOCK_MEMBERS, 1e-3, 0, 4),
        run(block_solve_loop, "block", BLOCK_MEMBERS, 1e-3, 2, 0),
        run(block_solve_loop, "block", BLOCK_MEMBERS, 0.0, 2, 4),
        run(block_solve_loop, "block", BLOCK_MEMBERS, float("nan"), 2, 4),
        run(filtered_solve_loop, "filter", FILTER_MEMBERS, 2.0 ** -8, 5, 4),       # tolerance, degree, max_blocks (guard 1)
        run(filtered_solve_loop, "filter", FILTER_MEMBERS, 2.0 ** -8, 5, 4, 1),
        run(filtered_solve_loop, "filter", FILTER_MEMBERS, 2.0 ** -8, 4, 4, 2),
        run(filtered_solve_loop, "filter", FILTER_MEMBERS, 2.0 ** -8, 256, 1, 2),
        run(filtered_solve_loop, "filter", nobody, 1e-3, 5, 4),
        run(filtered_solve_loop, "filter", FILTER_MEMBERS, 1e-3, 0, 4),
        run(filtered_solve_loop, "filter", FILTER_MEMBERS, 1e-3, 257, 4),
        run(filtered_solve_loop, "filter", FILTER_MEMBERS, 1e-3, 5, 0),
        run(filtered_solve_loop, "filter", FILTER_MEMBERS, -1.0, 5, 4),
        run(filtered_solve_loop, "filter", FILTER_MEMBERS, 1e-3, 5, 4, 0),
        run(filtered_solve_loop, "filter", FILTER_MEMBERS, 1e-3, 5, 4, 3),         # a member with k = 3: k - guard < 1
    ]


def test_the_scenarios_reach_every_status():
    """the fixture itself: every status of both loops, at the blocks the member tables say"""
    want = {"block": {(0, 2), (0, 3), (0, 4), (-5, 4), (-4, 1), (-4, 3)},                    # (status, blocks)
            "filter": {(0, 1), (0, 3), (0, 4), (-5, 4), (-4, 0), (-4, 2), (-1, 0), (-1, 2)}}  # -1: WAFER_ERR_INVALID, no interval
    got = {"block": set(), "filter": set()}
    for sc in json.load(open(FIXTURE)):
        for o in sc.get("result", []):
            if o is not None:
                got[sc["loop"]].add((o["status"], o["blocks"]))
        if "raises" in sc:
            assert sc["calls"] == []   # a refused call has called nothing
    for loop in want:
        assert want[loop] <= got[loop], (loop, sorted(want[loop] - got[loop]))
    messages = [o["message"] for sc in json.load(open(FIXTURE)) for o in sc.get("result", []) if o]
    for part in ("<= evals[0]", ">= the spectral bound", "linearly dependent: every state", "non-finite or linearly", "with max diff", "with max rho"):
        assert any(part in msg for msg in messages), part
    assert sum("raises" in sc for sc in json.load(open(FIXTURE))) == 10


def test_the_loops_make_the_recorded_calls_and_results():
    from wafer_amd import engine
    want = json.load(open(FIXTURE))
    got = json.loads(json.dumps(trace(engine.block_solve_loop, engine.filtered_solve_loop)))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g["loop"] == w["loop"] and g["args"] == w["args"]
        assert g.get("raises") == w.get("raises"), (g["loop"], g["args"])
        assert len(g["calls"]) == len(w["calls"]), (g["loop"], g["args"])
        for i, (a, b) in enumerate(zip(g["calls"], w["calls"])):
            assert a == b, (g["loop"], g["args"], i, a, b)
        for m, (a, b) in enumerate(zip(g.get("result", []), w.get("result", []))):
            assert a == b, (g["loop"], g["args"], m, a, b)
        assert g == w


if __name__ == "__main__":
    from wafer_amd import engine
    print("recording from", engine.__file__)
    with open(sys.argv[1], "w") as f:
        json.dump(trace(engine.block_solve_loop, engine.filtered_solve_loop), f, indent=1, sort_keys=True)
        f.write("\n")
