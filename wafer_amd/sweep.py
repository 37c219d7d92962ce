"""Sweeps: many `wafer.yaml` runs as batches on one GPU -- a convergence study over N and dn, a scan over potentials or masses --
every time step ONE launch for all runs of a batch that are still going (wafer_amd.Batch), instead of one process and one tiny
context per run.

    python -m wafer_amd.sweep -c a.yaml -c b.yaml ... [--output-dir DIR] [--input-dir DIR] [--max-batch N] [--seed S]
                              [--progress] [--plan] [--mix-states] [--batched-setup] [--ritz] [--residuals] [--moments]

Configuration reading and validation are the native driver's (`wafer-hip --check-config`, through wafer_amd.run.load_config), the
input files, the directory names and the table are wafer_amd.run's, and every run computes what `wafer-hip` computes for its file:
the loop of wafer_cli.cpp per run (observables, normalise, Gram-Schmidt, the symmetry constraint at the start and at every
snapshot block, the convergence and max_steps tests), each run with its own tolerance, screen_update, snap_update, max_steps and dt.

Grouping (plan_batches): runs are partitioned by (central_difference, dtype); within a partition the runs that need state stores
(wavenum > 0 or wavemax > 0) are split by grid shape, and the ground-state-only runs of all shapes share one mixed-shape batch.
With --mix-states the state runs of a partition form ONE group of all shapes instead: a mixed-shape batch with state stores
(wafer_amd.Batch(members, mixed_shapes=True, state_stores=True)), every run with the bits it has in a batch of its own shape.  It is
opt-in: the default grouping is unchanged.  Each group is cut in input order into batches of at most --max-batch members, which
run one after another.

Scheduling (run_phase): one phase per state number w = 0, 1, ...; in phase w the runs with wavenum <= w <= wavemax that have not
failed take part.  A run is at a block boundary when its own step counter is a multiple of its screen_update.  Every batched call
at a boundary -- normalise, orthogonalise, symmetrise, push_state -- covers all runs that are at a boundary at that moment, with an
active mask; between boundaries one evolve advances ALL running runs by next_chunk steps, the distance to the nearest boundary of
any of them.  A run that converges is pushed and sits out the rest of the phase; one that passes max_steps or whose energy is not
finite has failed and takes no further part, and the others go on.

Output: <output-dir>/<index:03d>_<project name>_<timestamp>/ per run with a copy of the config, table.txt (what wafer_amd.run prints
for that run up to its "Simulation complete" line; every block's row with --progress), observables_N.json / .csv and, with
save_wavefns, wavefunction_N.npy (wavefunction_N_partial.npy for a state that did not converge): the work area in the reference's
axis order.  Stdout: one JSON line per run, then the elapsed time.  The exit code is 0 only if every run converged in every state
it asked for.  Not in a sweep: script potentials.

Inputs (plan_inputs, set_up_batch): `potential` (FromFile), a `potential_sub` array, `wavefunction_N` (lower states and starts) and
`wavefunction_N_partial` may have another resolution than the run.  A file of the run's own size is copied; anything else is
trilinearly resampled on the device as `wafer-hip` resamples it (basis: the padded size; for potential_sub the work size), and the
runs of one batch that name the same file (real path and modification time) for the same role are set by ONE Batch.resample_* call
with their mask -- with --input-dir, one upload and one launch per file however many runs read it.  The five text / binary formats
are staged without a frame (pad 0); a ready-made `<stem>.npy` counts as framed for a run whose padded size it has and as plain data
for every other run.  --plan lists the groups under "inputs" without converting or writing anything: the shape of a .npy or .csv is
read from the file, for the other formats "shape", "copy" and "resample" are null.

--batched-setup: the built-in potentials of a batch's runs are ONE Batch.set_potentials call with their mask and the generated starts
of a phase ONE Batch.set_initial_conditions call with the same seeds, instead of one call per run: the same bits, one range check and
one read-back per batch instead of one per run.  Opt-in; the default stays the per-member calls.

--ritz: every batch that has state stores ends with ritz_phase -- wafer-hip's `gpu.ritz` step for all of its runs in ONE Batch.ritz call
(three launches and one read-back whatever the runs and shapes), each run with its own number of stored states.  A run takes part if
every state it asked for converged and it holds 2 .. 8 states; its table.txt gains wafer-hip's "Ritz" block, its observables_N files
and saved wavefunctions are rewritten from the rotated states, and its JSON line gains "ritz": {"evals": [...]} (null for a run that
did not take part).  The `gpu.ritz` key of a wafer.yaml stays refused: the step is asked for per sweep, not per file.  Off by default;
without it nothing changes.

--residuals: every batch ends with residual_phase -- ONE Batch.residuals call in Rayleigh mode for all of its runs, on the stored states
where the batch has state stores (after the --ritz step), on phi in a ground-state batch -- and a run's JSON line gains
"residuals": {"theta": [...], "rho": [...]}: some eigenvalue of the run's discrete H lies within rho[j] of theta[j] (null for a run that
did not take part).  The `gpu.residual` key of a wafer.yaml stays refused like `gpu.ritz`.  Off by default; without it nothing changes.

--moments: every batch that has state stores then ends with moment_phase -- ONE Batch.moments call for all of its runs that hold
1 .. 8 stored states, each with its own state count (after the --ritz and --residuals steps) -- and a run's JSON line gains
"moments": {"s": [[...]], "x": ..., "y": ..., "z": ..., "r2": ...}, the matrices wafer-hip prints under `gpu.moments`, in index units
from observables' origin (null for a run that did not take part, and in ground-state batches).  The `gpu.moments` key of a wafer.yaml
stays refused like `gpu.ritz`.  Off by default; without it nothing changes.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np

from wafer_amd.run import find_input, load_config, measurement_row, observable_header, sanitize, staged_array, summary

DEFAULT_MAX_BATCH = 64


# ---- grouping -------------------------------------------------------------------------------------------------------------------
def needs_states(cfg: dict) -> bool:
    return cfg["wavenum"] > 0 or cfg["wavemax"] > 0


def plan_batches(cfgs: list, max_batch: int = DEFAULT_MAX_BATCH, mix_states: bool = False) -> list:
    """-> the batches in running order, each dict(members=[input indices], central_difference, dtype, needs_states, mixed_shapes,
    shapes=[distinct (nx, ny, nz)]).  Groups appear in the order of their first member; every input index appears exactly once.
    mix_states: the state runs of a (stencil, dtype) partition are one group whatever their shapes (needs_states and mixed_shapes
    both True: a mixed-shape batch with state stores) instead of one group per shape."""
    if max_batch < 1:
        raise ValueError("max_batch must be >= 1")
    groups: dict = {}
    for i, c in enumerate(cfgs):
        key = (c["central_difference"], c["dtype"])
        if not needs_states(c):
            key += ("ground",)
        else:
            key += ("states",) if mix_states else ("states", c["nx"], c["ny"], c["nz"])
        groups.setdefault(key, []).append(i)
    out = []
    for key, idx in groups.items():
        for at in range(0, len(idx), max_batch):
            members = idx[at:at + max_batch]
            shapes = []
            for i in members:
                s = (cfgs[i]["nx"], cfgs[i]["ny"], cfgs[i]["nz"])
                if s not in shapes:
                    shapes.append(s)
            out.append(dict(members=members, central_difference=key[0], dtype=key[1], needs_states=key[2] == "states",
                            mixed_shapes=key[2] == "ground" or len(key) == 3, shapes=[list(s) for s in shapes]))
    return out


def next_chunk(remaining) -> int:
    """steps of the next evolve: the smallest distance (> 0) of any running run to its next block boundary"""
    d = min(remaining)
    if d < 1:
        raise ValueError("a running member is at a boundary: it has to be handled before the next evolve")
    return int(d)


# ---- one run ----------------------------------------------------------------------------------------------------------------------
class Run:
    """one wafer.yaml in a batch: its configuration, its place (slot), its step counter and what it has printed so far"""

    def __init__(self, index: int, cfg: dict, config_path: str | None = None, input_dir: str | None = None, out_dir: str | None = None):
        self.index, self.cfg, self.config_path, self.input_dir, self.out_dir = index, cfg, config_path, input_dir, out_dir
        self.slot = 0
        self.batch = 0
        self.lines: list = []        # table.txt, line by line
        self.states: list = []       # per state: dict(state, status, steps, energy)
        self.failed = False
        self.ritz = None             # --ritz: dict(evals=[...]) once the run's states have been rotated
        self.moments = None          # --moments: dict(s=[[...]], x=..., y=..., z=..., r2=...) once the run has taken part in moment_phase
        self.residuals = None        # --residuals: dict(theta=[...], rho=[...]) once the run has taken part in residual_phase
        self.boundaries: list = []   # the steps of this phase's block boundaries
        # the phase's loop variables (grid.rs:122-125)
        self.step, self.remaining, self.last_energy, self.cloned, self.running = 0, 0, sys.float_info.max, False, False

    def say(self, text: str) -> None:
        self.lines.append(text)

    def path(self, name: str) -> str | None:
        return None if self.out_dir is None else os.path.join(self.out_dir, name)

    def write_table(self) -> None:
        if self.out_dir is not None:
            with open(self.path("table.txt"), "w") as f:
                f.write("".join(l + "\n" for l in self.lines))

    def save_phi(self, batch, name: str) -> None:
        if self.out_dir is None:
            return
        e = self.cfg["central_difference"]
        work = np.ascontiguousarray(batch.download_phi(self.slot)[e:-e, e:-e, e:-e])
        tmp = self.path(name + ".tmp.npy")
        np.save(tmp, work)
        os.replace(tmp, self.path(name + ".npy"))

    def takes_part(self, w: int) -> bool:
        return not self.failed and self.cfg["wavenum"] <= w <= self.cfg["wavemax"]


def _mask(runs, chosen) -> list:
    on = {r.slot for r in chosen}
    return [1 if r.slot in on else 0 for r in runs]


def _norm_energy(o: dict) -> float:
    return o["energy"] / o["norm2"] if o["norm2"] != 0.0 else math.nan


def final_measurement(w: int, obs: dict, nx: int) -> dict:
    """output::finalise_measurement's record of state w from the raw sums (output.rs:540-547)"""
    r_norm = math.sqrt(obs["r2"] / obs["norm2"])
    return dict(state=w, energy=obs["energy"] / obs["norm2"], binding_energy=(obs["energy"] - obs["v_infinity"]) / obs["norm2"],
                r=r_norm, l_r=nx / r_norm)


def write_observables(r, w: int, fin: dict) -> None:
    """observables_w.json and .csv of run r"""
    if r.out_dir is None:
        return
    with open(r.path(f"observables_{w}.json"), "w") as f:
        json.dump(fin, f, indent=2)
    with open(r.path(f"observables_{w}.csv"), "w") as f:
        f.write("state,energy,binding_energy,r,l_r\n%d,%r,%r,%r,%r\n" % (w, fin["energy"], fin["binding_energy"], fin["r"], fin["l_r"]))


def run_phase(batch, runs: list, w: int, progress: bool = False, push: bool = False, log=sys.stderr) -> None:
    """State w of every run of `runs` (the batch's members in slot order) that takes part, from the starts already in the batch:
    the loop of wafer_cli.cpp:666-753 per run, the batched calls shared as the module docstring says.  push: converged runs go to
    their state stores (a batch that holds runs with excited states)."""
    part = [r for r in runs if r.takes_part(w)]
    for r in part:
        r.step, r.remaining, r.last_energy, r.running, r.boundaries = 0, 0, sys.float_info.max, True, []
        r.say(observable_header(w))
    n = len(runs)

    def finish(r, obs, converged, status):
        r.running = False
        fin = final_measurement(w, obs, r.cfg["nx"])
        r.states.append(dict(state=w, status=status, steps=r.step, energy=fin["energy"]))
        if converged:                                                     # output.rs:533-558
            r.say(summary(fin))
            write_observables(r, w, fin)
            if r.out_dir is not None:
                if r.cfg["snap_update"] is not None and os.path.exists(r.path(f"wavefunction_{w}_partial.npy")):
                    os.remove(r.path(f"wavefunction_{w}_partial.npy"))
        if r.cfg["save_wavefns"]:                                         # grid.rs:223-237: saved whether converged or not
            r.save_phi(batch, f"wavefunction_{w}{'' if converged else '_partial'}")
        if not converged:                                                 # grid.rs:243-245
            print(f"run {r.index}: Error: MaxStep: maximum step limit reached for state {w}", file=log, flush=True)
            r.failed = True
        r.write_table()

    while True:
        running = [r for r in part if r.running]
        if not running:
            break
        at = [r for r in running if r.remaining == 0]
        if not at:                                                        # between boundaries: one evolve for every running run
            d = next_chunk([r.remaining for r in running])
            batch.evolve(d, active=_mask(runs, running), wnum=w)
            for r in running:
                r.step += d
                r.remaining -= d
            continue
        for r in at:
            r.boundaries.append(r.step)
        obs = batch.observables()                                         # wafer_cli.cpp:671
        finite = [r for r in at if math.isfinite(_norm_energy(obs[r.slot]))]
        for r in at:
            if r not in finite:
                print(f"run {r.index}: Error: state {w}: energy is not finite at step {r.step}", file=log, flush=True)
                r.running, r.failed = False, True
                r.states.append(dict(state=w, status="NotFinite", steps=r.step, energy=None))
                r.write_table()
        at = finite
        if not at:
            continue
        norm2s = [1.0] * n
        for r in at:
            norm2s[r.slot] = obs[r.slot]["norm2"]
        batch.normalise(norm2s, active=_mask(runs, at))                   # :674
        if w > 0:
            batch.orthogonalise(w, active=_mask(runs, at))                # :675
        clones = [r for r in at if r.cloned and r.step == 0]
        if clones:                                                        # :676-692: a clone annihilated to exactly zero
            n2 = batch.norm2()
            for r in clones:
                if not (n2[r.slot] > 0.0) or not math.isfinite(n2[r.slot]):
                    print(f"run {r.index}: Warning: the clone of state {w - 1} was annihilated exactly by Gram-Schmidt; "
                          f"starting state {w} from Gaussian noise instead.", file=log, flush=True)
                    batch.set_initial_condition(r.slot, "Gaussian", seed=0x5EED + w)
                    r.cloned, r.last_energy = False, sys.float_info.max
                    r.boundaries.pop()
                    at.remove(r)                                          # (it meets this boundary again, before any evolve)
        snaps = [r for r in at if r.cfg["snap_update"] is not None and r.step % r.cfg["snap_update"] == 0]
        if snaps:                                                         # :693-707
            cons = ["NotConstrained"] * n
            for r in snaps:
                cons[r.slot] = r.cfg["init_symmetry"]
            batch.symmetrise(cons, active=_mask(runs, snaps))             # grid.rs:138
            for r in snaps:
                r.save_phi(batch, f"wavefunction_{w}_partial")
        done = []
        for r in at:
            o = obs[r.slot]
            norm_energy = _norm_energy(o)
            tau = r.step * r.cfg["dt"]
            diff = abs(norm_energy - r.last_energy)                       # :708
            if diff < r.cfg["tolerance"]:                                 # :710-714
                r.say(measurement_row(tau, diff, o))
                done.append(r)
                continue
            if progress:
                r.say(measurement_row(tau, diff, o))
            r.last_energy = norm_energy
            if r.cfg["max_steps"] is not None and r.step > r.cfg["max_steps"]:   # :717
                finish(r, o, False, "MaxStep")
                continue
            r.remaining = r.cfg["screen_update"]
        for r in done:
            finish(r, obs[r.slot], True, "Converged")
        if push and done:
            batch.push_state(active=_mask(runs, done))                    # grid.rs:241


# ---- Rayleigh-Ritz on the converged sets (--ritz) ----------------------------------------------------------------------------------
def ritz_phase(batch, runs: list, log=sys.stderr) -> None:
    """wafer-hip's `gpu.ritz` step (wafer_cli.cpp:764-791) for every run of a batch with state stores, after its last phase: ONE
    Batch.ritz call for the eligible runs, each with its own state count -- a run is eligible if it has not failed, every state it
    asked for converged and it holds 2 .. RITZ_MAX states; any other run that holds states gets wafer-hip's line on `log`.  A rotated
    run's table gains the block wafer-hip prints, and its observables_a files (and, with save_wavefns, wavefunction_a.npy) are
    rewritten from the rotated states: per state number one clone_state_to_phi and one Batch.observables for all runs that have it.
    A run whose solve fails (status != 0) keeps its files."""
    from wafer_amd.engine import RITZ_MAX, WAFER_OK
    from wafer_amd.run import rust_lower_exp

    held = batch.num_states()
    eligible = []
    for r in runs:
        r.ritz = None
        ns = held[r.slot]
        asked = r.cfg["wavemax"] - r.cfg["wavenum"] + 1
        if r.failed or len(r.states) != asked or any(s["status"] != "Converged" for s in r.states):
            if ns > 0:
                print(f"run {r.index}: Ritz: skipped, not every state converged", file=log, flush=True)
        elif ns < 2 or ns > RITZ_MAX:
            if ns > 0:
                print(f"run {r.index}: Ritz: skipped, {ns} stored states (the step takes 2 .. {RITZ_MAX})", file=log, flush=True)
        else:
            eligible.append(r)
    if not eligible:
        return
    ks = [0] * len(runs)
    for r in eligible:
        ks[r.slot] = held[r.slot]
    res = batch.ritz(k=ks, active=_mask(runs, eligible))
    rotated = []
    for r in eligible:
        out = res[r.slot]
        if out["status"] != WAFER_OK:
            print(f"run {r.index}: Ritz: skipped, the overlap matrix is not positive definite", file=log, flush=True)
            continue
        rotated.append(r)
        k = ks[r.slot]
        r.ritz = dict(evals=[float(x) for x in out["evals"]])
        r.say("Ritz")                                                     # state, its energy before the step (H_aa / S_aa), the Ritz value
        for a in range(k):
            r.say(f"{a:3d} {rust_lower_exp(out['h'][a][a] / out['s'][a][a], 10):>19} {rust_lower_exp(out['evals'][a], 10):>19}")
        r.say("")
    for a in range(max((ks[r.slot] for r in rotated), default=0)):
        have = [r for r in rotated if ks[r.slot] > a]
        batch.clone_state_to_phi(a, active=_mask(runs, have))
        obs = batch.observables()
        for r in have:
            write_observables(r, a, final_measurement(a, obs[r.slot], r.cfg["nx"]))
            if r.cfg["save_wavefns"]:
                r.save_phi(batch, f"wavefunction_{a}")
    for r in rotated:
        r.write_table()


# ---- residuals of the results (--residuals) ---------------------------------------------------------------------------------------
def residual_phase(batch, runs: list, states: bool) -> None:
    """theta and rho = |H l - theta l| / |l| of every run's results after the batch's last phase, in ONE Batch.residuals call in
    Rayleigh mode.  states: the batch has state stores -- every run that holds at least one stored state takes part with its first
    min(held, RITZ_MAX); else a ground-state batch -- every run that has not failed takes part with its phi.  A run that took part
    gets r.residuals = dict(theta=[...], rho=[...]); the others, and a run whose state has no Rayleigh quotient, None."""
    from wafer_amd.engine import RITZ_MAX, WAFER_OK

    for r in runs:
        r.residuals = None
    if states:
        held = batch.num_states()
        part = [r for r in runs if held[r.slot] > 0]
        ks = [0] * len(runs)
        for r in part:
            ks[r.slot] = min(held[r.slot], RITZ_MAX)
    else:
        part = [r for r in runs if not r.failed]
        ks = [1 if r in part else 0 for r in runs]
    if not part:
        return
    res = batch.residuals(k=ks, active=_mask(runs, part), source="states" if states else "phi")
    for r in part:
        out = res[r.slot]
        if out["status"] == WAFER_OK:
            r.residuals = dict(theta=[float(x) for x in out["theta"]], rho=[float(x) for x in out["rho"]])


# ---- moment matrices of the results (--moments) -----------------------------------------------------------------------------------
def moment_phase(batch, runs: list) -> None:
    """wafer-hip's `gpu.moments` read-out for every run of a batch with state stores, after ritz_phase and residual_phase: ONE
    Batch.moments call for all runs that hold 1 .. RITZ_MAX stored states, each with its own state count.  A run that took part gets
    r.moments = dict(s=..., x=..., y=..., z=..., r2=...), (k, k) nested lists; the others None."""
    from wafer_amd.engine import MOMENT_NAMES, RITZ_MAX

    for r in runs:
        r.moments = None
    held = batch.num_states()
    part = [r for r in runs if 1 <= held[r.slot] <= RITZ_MAX]
    if not part:
        return
    ks = [0] * len(runs)
    for r in part:
        ks[r.slot] = held[r.slot]
    res = batch.moments(k=ks, active=_mask(runs, part))
    for r in part:
        r.moments = {name: [[float(v) for v in row] for row in res[r.slot][name]] for name in MOMENT_NAMES}


# ---- set-up ---------------------------------------------------------------------------------------------------------------------
def input_file(input_dir: str, stem: str, file_type: str):
    """the file a run reads for `stem` (a ready-made <stem>.npy first, as staged_array takes it) -> (real path, mtime) or None"""
    ready = os.path.join(input_dir, stem + ".npy")
    path = ready if os.path.exists(ready) else find_input(input_dir, stem, file_type)
    if path is None:
        return None
    path = os.path.realpath(path)
    return path, os.path.getmtime(path)


def _shapes(cfg: dict) -> tuple:
    e, work = cfg["central_difference"], (cfg["nx"], cfg["ny"], cfg["nz"])
    return work, tuple(n + 2 * e for n in work)


def _load(run: Run, stem: str) -> np.ndarray:
    """the array of stem.* without a frame (a ready-made .npy as it is)"""
    return staged_array(run.input_dir, stem, run.cfg["file_type"], 0, 0)


def peek_shape(path: str):
    """the shape of an input file without converting it (what --plan may do: no driver binary, nothing written): a .npy from its header,
    a .csv (i,j,k,data rows in C order, output.rs:148-165) from its last row; None for the formats that have to be parsed whole"""
    if path.endswith(".npy"):
        return list(np.load(path, mmap_mode="r").shape)
    if path.endswith(".csv"):
        with open(path, "rb") as f:
            f.seek(0, os.SEEK_END)
            f.seek(max(0, f.tell() - 4096))
            rows = [l for l in f.read().decode(errors="replace").splitlines() if l.strip()]
        try:
            cells = rows[-1].split(",")
            return [int(c) + 1 for c in cells[:-1]] if len(cells) == 4 else ([] if len(cells) == 1 else None)
        except (IndexError, ValueError):
            return None
    return None


def how_to_set(cfg: dict, role: str, path: str, shape) -> str:
    """"framed": a ready-made .npy of the run's padded size, used as it is; "copy": the run's own work size (a scalar too);
    "resample": anything else"""
    work, padded = _shapes(cfg)
    shape = tuple(shape)
    if role != "potential_sub" and path.endswith(".npy") and shape == padded:
        return "framed"
    return "copy" if shape == work or shape == () else "resample"


def _starts(cfg: dict, w: int) -> bool:
    """does state w of this run start from a file if there is one?  (grid.rs:60-100)"""
    return cfg["wavenum"] <= w <= cfg["wavemax"] and (w > 0 or cfg["init_condition"] == "FromFile")


def plan_inputs(runs: list, load=_load, roles=None) -> list:
    """The input files of the runs of ONE batch, grouped: -> [dict(role, state, stem, path, mtime, shape, members, copy, resample)] in
    the order potential, potential_sub, state (lower states from disk, by number), start (by number), then first appearance.  Two runs
    share a group when they read the same file -- the same real path and modification time -- for the same role and state number.
    members: the runs' input indices; copy: those of them whose own size the file has (set per member, as before), resample: the rest
    (set by one Batch.resample_* call).  Touches no GPU.  load(run, stem) -> array reads a file, once per group; the array stays in
    the group as "array" for apply_inputs.  load=None only looks (--plan): the shape comes from peek_shape, and where that cannot tell
    without converting the file, shape, copy and resample are None.
    roles: only these (start_phase asks for one phase's starts)."""
    wanted = []
    for r in runs:
        c = r.cfg
        if c["potential"] == "FromFile":
            wanted.append((0, "potential", 0, "potential", r))
        wanted.append((1, "potential_sub", 0, "potential_sub", r))
        for w in range(c["wavenum"]):
            wanted.append((2, "state", w, f"wavefunction_{w}", r))
        for w in range(c["wavenum"], c["wavemax"] + 1):
            if _starts(c, w):
                stem = f"wavefunction_{w}"
                if input_file(r.input_dir, stem, c["file_type"]) is None:     # input.rs:513-523
                    stem += "_partial"
                wanted.append((3, "start", w, stem, r))
    groups: dict = {}
    for order, role, w, stem, r in sorted(wanted, key=lambda t: (t[0], t[2])):
        if roles is not None and (role, w) not in roles:
            continue
        f = input_file(r.input_dir, stem, r.cfg["file_type"])
        if f is None:
            continue
        key = (role, w) + f
        g = groups.get(key)
        if g is None:
            g = groups[key] = dict(role=role, state=w, stem=stem, path=f[0], mtime=f[1], members=[], copy=[], resample=[])
            if load is None:
                g["shape"] = peek_shape(f[0])
                if g["shape"] is None:
                    g["copy"] = g["resample"] = None
            else:
                g["array"] = load(r, stem)
                g["shape"] = list(np.shape(g["array"]))
        g["members"].append(r.index)
        if g["shape"] is not None:
            g["resample" if how_to_set(r.cfg, role, g["path"], g["shape"]) == "resample" else "copy"].append(r.index)
    return list(groups.values())


def _framed(run: Run, role: str, path: str, a: np.ndarray) -> np.ndarray:
    """a copied array in the run's zero frame (a ready-made framed .npy as it is)"""
    if how_to_set(run.cfg, role, path, a.shape) == "framed":
        return np.ascontiguousarray(a, dtype=np.float64)
    e = run.cfg["central_difference"]
    out = np.zeros(_shapes(run.cfg)[1])
    out[e:-e, e:-e, e:-e] = a
    return out


def apply_inputs(batch, runs: list, groups: list, load=_load) -> None:
    """the groups of plan_inputs onto the batch: the copies per member, the rest of a group in one resample call with its mask"""
    by_index = {r.index: r for r in runs}
    for g in groups:
        first = by_index[g["members"][0]]
        a = g["array"] if "array" in g else load(first, g["stem"])       # (read once, by plan_inputs)
        role, w = g["role"], g["state"]
        if role == "potential_sub":                                       # potential.rs:113-131
            for i in g["members"]:
                r = by_index[i]
                if (a.ndim == 0) == (r.cfg["potential"] == "FullCornell"):
                    raise SystemExit(f"{r.config_path}: Error: WrongPotentialSubDims: potential_sub input file does not suit the potential type")
            for i in g["copy"]:
                if a.ndim == 0:
                    batch.set_potsub(by_index[i].slot, 1, float(a))
                else:
                    batch.set_potsub(by_index[i].slot, 2, 0.0, np.ascontiguousarray(a, dtype=np.float64))
        else:
            if a.ndim != 3:
                raise SystemExit(f"{first.config_path}: {g['path']} holds {a.ndim} dimensions, not 3")
            for i in g["copy"]:
                r = by_index[i]
                full = _framed(r, role, g["path"], a)
                if role == "potential":
                    batch.set_potential_host(r.slot, full)
                elif role == "state":
                    batch.load_state(r.slot, w, full)
                else:
                    batch.upload_phi(r.slot, full)
        if g["resample"]:
            src = np.ascontiguousarray(a, dtype=np.float64)
            mask = _mask(runs, [by_index[i] for i in g["resample"]])
            if role == "potential":
                batch.resample_potential(src, active=mask, basis="padded")
            elif role == "potential_sub":
                batch.resample_potsub(src, active=mask, basis="work")     # input.rs:472
            elif role == "state":
                batch.resample_state(w, src, active=mask, basis="padded")
            else:
                batch.resample_phi(src, active=mask, basis="padded")


def set_up_batch(batch, runs: list, load=_load, batched: bool = False) -> None:
    """potentials, pot_sub overrides and the lower states from disk for every run of the batch, as wafer_amd.run sets a context up:
    built-in potentials per member -- or, with batched=True, in ONE Batch.set_potentials call with their mask (--batched-setup: the
    same bits) -- everything that comes from a file through plan_inputs' groups"""
    builtin = []
    for r in runs:
        c = r.cfg
        if c["potential"] == "FromFile":                                  # potential.rs:80-86
            if input_file(r.input_dir, "potential", c["file_type"]) is None:
                raise SystemExit(f"{r.config_path}: Error: LoadPotential: FileNotFound: {r.input_dir}/potential.*")
        elif batched:
            builtin.append(r)
        else:
            batch.set_potential(r.slot, c["potential"])
        for w in range(c["wavenum"]):                                     # grid.rs:35-39: converged lower states from disk
            if input_file(r.input_dir, f"wavefunction_{w}", c["file_type"]) is None:
                raise SystemExit(f"{r.config_path}: Error: LoadWavefunction({w}): FileNotFound: {r.input_dir}/wavefunction_{w}.*")
    if builtin:
        names = ["NoPotential"] * len(runs)
        for r in builtin:
            names[r.slot] = r.cfg["potential"]
        batch.set_potentials(names, active=_mask(runs, builtin))
    roles = {("potential", 0), ("potential_sub", 0)} | {("state", w) for r in runs for w in range(r.cfg["wavenum"])}
    groups = plan_inputs(runs, load, roles=roles)                          # (the starts are read by start_phase, phase by phase)
    apply_inputs(batch, runs, groups, load)


def start_phase(batch, runs: list, pars: list, w: int, seed: int, load=_load, batched: bool = False) -> None:
    """the start of state w for every run that takes part (grid.rs:60-100), then, for w = 0, one symmetrise with every run's
    init_symmetry (config.rs:625).  batched=True: the generated starts are ONE Batch.set_initial_conditions call with their mask and
    the same seeds, instead of one call per member."""
    part = [r for r in runs if r.takes_part(w)]
    groups = plan_inputs(part, load, roles={("start", w)})
    from_file = {i for g in groups for i in g["members"]}
    clones, generated = [], []
    for r in part:
        r.cloned = False
        if r.index in from_file:
            continue
        if w > 0:                                                         # grid.rs:95
            clones.append(r)
            r.cloned = True
        elif r.cfg["init_condition"] == "FromFile":
            raise SystemExit(f"{r.config_path}: Error: SetInitialConditions: LoadWavefunction(0): FileNotFound: {r.input_dir}/wavefunction_0*.*")
        elif batched:
            generated.append(r)
        else:                                                             # grid.rs:99, config.rs:577-627
            batch.set_initial_condition(r.slot, r.cfg["init_condition"], seed=seed)
    if generated:
        names = ["Boolean"] * len(runs)
        for r in generated:
            names[r.slot] = r.cfg["init_condition"]
        batch.set_initial_conditions(names, seeds=[seed] * len(runs), active=_mask(runs, generated))
    apply_inputs(batch, runs, groups, load)
    if clones:
        batch.clone_state_to_phi(w - 1, active=_mask(runs, clones))
    if w == 0 and part:
        cons = ["NotConstrained"] * len(runs)
        for r in part:
            cons[r.slot] = r.cfg["init_symmetry"]
        batch.symmetrise(cons, active=_mask(runs, part))


def run_batch(plan: dict, runs: list, seed: int, progress: bool, batched: bool = False, ritz: bool = False, residuals: bool = False,
              moments: bool = False) -> tuple:
    """one batch of the plan from creation to its last phase -> (fused passes, one-step launches).  batched: set_up_batch's and
    start_phase's (--batched-setup).  ritz: a batch that has state stores ends with ritz_phase (--ritz).  residuals: every batch ends
    with residual_phase, after ritz_phase (--residuals).  moments: a batch that has state stores then ends with moment_phase (--moments)"""
    import wafer_amd

    pars = []
    for slot, r in enumerate(runs):
        r.slot = slot
        c = r.cfg
        pars.append(wafer_amd.Params(c["nx"], c["ny"], c["nz"], dn=c["dn"], dt=c["dt"], mass=c["mass"], sig=c["sig"],
                                     central_difference=c["central_difference"], dtype=c["dtype"], max_states=c["wavemax"] + 1))
    # (a state group of plan_batches(mix_states=True): the mixed-shape batch that has state stores)
    kind = dict(mixed_shapes=True, state_stores=True) if plan["needs_states"] and plan["mixed_shapes"] else dict(mixed_shapes=plan["mixed_shapes"])
    with wafer_amd.Batch(pars, **kind) as batch:
        set_up_batch(batch, runs, batched=batched)
        late = [r for r in runs if r.cfg["wavenum"] > 0]
        if late:   # observables run over every member: a run that starts at a later state waits with its state 0 as phi
            batch.clone_state_to_phi(0, active=_mask(runs, late))
        for w in range(min(r.cfg["wavenum"] for r in runs), max(r.cfg["wavemax"] for r in runs) + 1):
            start_phase(batch, runs, pars, w, seed, batched=batched)
            run_phase(batch, runs, w, progress=progress, push=plan["needs_states"])
        if ritz and plan["needs_states"]:
            ritz_phase(batch, runs)
        if residuals:
            residual_phase(batch, runs, states=plan["needs_states"])
        if moments and plan["needs_states"]:
            moment_phase(batch, runs)
        return batch.passes()


# ---- command line ---------------------------------------------------------------------------------------------------------------
def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m wafer_amd.sweep")
    ap.add_argument("-c", "--config", action="append", required=True, help="a wafer.yaml; give it once per run")
    ap.add_argument("--output-dir", default="./output")
    ap.add_argument("--input-dir", default=None, help="one input directory for all runs (default: input/ next to each config file)")
    ap.add_argument("--max-batch", type=int, default=DEFAULT_MAX_BATCH)
    ap.add_argument("--seed", type=int, default=None, help="seed of Gaussian starts (default: the time)")
    ap.add_argument("--progress", action="store_true", help="a table row per screen_update block in every table.txt")
    ap.add_argument("--plan", action="store_true", help="print the grouping as JSON and exit; touches no GPU")
    ap.add_argument("--mix-states", action="store_true",
                    help="runs with excited states share one mixed-shape batch per (stencil, dtype) instead of one batch per grid shape")
    ap.add_argument("--batched-setup", action="store_true",
                    help="built-in potentials and generated starts of a batch in one Batch.set_potentials / set_initial_conditions call "
                         "instead of one call per run (the same results)")
    ap.add_argument("--ritz", action="store_true",
                    help="after the last phase of every batch with state stores, one Rayleigh-Ritz step on the converged states of its runs "
                         "(what gpu.ritz: true does in wafer-hip), all runs of the batch in one Batch.ritz call")
    ap.add_argument("--residuals", action="store_true",
                    help="after the last phase of every batch (after the --ritz step), theta and rho = |H l - theta l| / |l| of every run's "
                         "stored states -- of its phi in a ground-state batch -- in one Batch.residuals call; a JSON line gains \"residuals\"")
    ap.add_argument("--moments", action="store_true",
                    help="after the last phase of every batch with state stores (after the --ritz and --residuals steps), the matrices "
                         "<i|1|j>, <i|x|j>, <i|y|j>, <i|z|j>, <i|r^2|j> of every run's stored states (what gpu.moments: true prints in wafer-hip) "
                         "in one Batch.moments call; a JSON line gains \"moments\"")
    args = ap.parse_args(argv)
    if args.max_batch < 1:
        raise SystemExit("--max-batch must be >= 1")

    cfgs = [load_config(p) for p in args.config]
    for p, c in zip(args.config, cfgs):
        if c["potential"] == "FromScript":
            raise SystemExit(f"{p}: wafer_amd.sweep: script potentials are a single-GPU feature (wafer-hip -s); "
                             "save the potential there and use potential: FromFile")
        if c["init_symmetry"] != "NotConstrained" and c["central_difference"] != 3:
            raise SystemExit(f"{p}: Error: init_symmetry {c['init_symmetry']} needs central_difference: SevenPoint "
                             "(config.rs:702-725 indexes the 3-cell frame)")
        if c["screen_update"] < 1:
            raise SystemExit(f"{p}: a sweep needs screen_update >= 1")
        if c.get("ritz"):
            raise SystemExit(f"{p}: wafer_amd.sweep: gpu.ritz: true (the Rayleigh-Ritz step on the stored states) is a wafer-hip key; "
                             "a sweep takes the step for all of its runs with the command-line flag --ritz")
        if c.get("residual"):
            raise SystemExit(f"{p}: wafer_amd.sweep: gpu.residual: true (the residuals of the stored states) is a wafer-hip key; "
                             "a sweep computes them for all of its runs with the command-line flag --residuals")
        if c.get("moments"):
            raise SystemExit(f"{p}: wafer_amd.sweep: gpu.moments: true (the moment matrices of the stored states) is a wafer-hip key; "
                             "a sweep computes them for all of its runs with the command-line flag --moments")
    plan = plan_batches(cfgs, args.max_batch, mix_states=args.mix_states)
    if args.plan:
        inputs = []
        for k, b in enumerate(plan):
            members = [Run(i, cfgs[i], args.config[i], args.input_dir or os.path.join(os.path.dirname(os.path.abspath(args.config[i])), "input"))
                       for i in b["members"]]
            for g in plan_inputs(members, load=None):                     # (looks only: converts nothing, writes nothing)
                inputs.append(dict(batch=k, role=g["role"], state=g["state"], path=g["path"], shape=g["shape"], members=g["members"],
                                   copy=g["copy"], resample=g["resample"]))
        print(json.dumps(dict(configs=args.config, batches=plan, inputs=inputs)))
        return 0

    seed = int(time.time()) if args.seed is None else args.seed
    print(f"seed of Gaussian starts: {seed}", file=sys.stderr, flush=True)
    os.makedirs(args.output_dir, exist_ok=True)
    stamp = time.strftime("%Y-%m-%d_%H:%M:%S")
    runs = []
    for i, (p, c) in enumerate(zip(args.config, cfgs)):
        out_dir = os.path.join(args.output_dir, f"{i:03d}_{sanitize(c['project_name'])}_{stamp}")
        os.makedirs(out_dir)
        with open(p) as src, open(os.path.join(out_dir, os.path.basename(p)), "w") as dst:
            dst.write(src.read())
        runs.append(Run(i, c, p, args.input_dir or os.path.join(os.path.dirname(os.path.abspath(p)), "input"), out_dir))

    t0 = time.perf_counter()
    launches = []
    for k, b in enumerate(plan):
        members = [runs[i] for i in b["members"]]
        for r in members:
            r.batch = k
        more = dict(ritz=True) if args.ritz else {}   # (without the flags the call is what it has always been)
        if args.residuals:
            more["residuals"] = True
        if args.moments:
            more["moments"] = True
        launches.append(run_batch(b, members, seed, args.progress, batched=args.batched_setup, **more))
    ok = True
    for r in runs:
        asked = r.cfg["wavemax"] - r.cfg["wavenum"] + 1
        converged = len(r.states) == asked and all(s["status"] == "Converged" for s in r.states)
        ok = ok and converged
        b = plan[r.batch]
        line = dict(index=r.index, config=r.config_path, directory=r.out_dir, converged=converged, states=r.states, batch=r.batch,
                    batch_members=b["members"], mixed_shapes=b["mixed_shapes"], fused_passes=launches[r.batch][0],
                    single_steps=launches[r.batch][1])
        if args.ritz:
            line["ritz"] = r.ritz
        if args.residuals:
            line["residuals"] = r.residuals
        if args.moments:
            line["moments"] = r.moments
        print(json.dumps(line), flush=True)
    print(f"Sweep complete. Elapsed time: {time.perf_counter() - t0:.3f} seconds.\nOutput directory: {args.output_dir}", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
