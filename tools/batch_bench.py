#!/usr/bin/env python3
"""Batched ensembles against what a user does today: B members of one shape (Harmonic, ThreePoint, members differing in
dt) advanced by one wafer_batch_evolve, by B Contexts one after another from one thread, and by B Contexts on B Python threads
(ctypes releases the GIL).  One JSON line per (shape, B):
  batch_us_per_step / batch_gups  HIP events around the batch's step launches, after warm-up
  batch_host_us_per_step / _gups  host clock around the batch's evolve call until its last step has finished (host work, launches
                                  and the wait included: timed like the two baselines; the speedups are taken from these)
  seq_us_per_step / seq_gups      host clock around B x (evolve + synchronise), one context after another
  thr_us_per_step / thr_gups      host clock around B threads, each evolve + synchronise on its own context
  parity                          member 0 of the batch bit-identical to a single context after the same steps
gups: grid-point updates per second (members x work cells x steps / time), 1e9.
--wnum K: excited-state steps instead -- every member gets an orthonormal store of K states (seeded random, orthonormalised on
the host), the batch runs evolve(steps, wnum=K), the contexts evolve(K, steps); the same columns and clocks plus "wnum", and
parity becomes max |batch - context| <= 1e-13 over member 0's cells, the value itself in "parity_max_abs".
--variant V: Batch.set_step_variant(V) before the first step (-1 default dispatch, 0 one step per launch, 1 fused passes); the
row records "variant", "steps_per_launch", the dispatch line and the launch counts of the timed call.
--dtype D: f64 (default), f32 (float storage, fp64 arithmetic) or f32fast (float arithmetic in the ground-state step) for the
batch and the contexts alike; the row records "dtype".  On the float dtypes the excited-state parity bar is 4 float spacings at
max |phi| (the two partition their sums differently, and a last-bit difference of a scalar can flip a float rounding), the
ground-state parity stays bit for bit.
--gs-variant V: Batch.set_gs_variant(V) before the first step (-1 default dispatch, 0 the sequential normalise / Gram-Schmidt chain,
1 the one-pass form for wnum <= 4); the row records "gs_variant", the gs_dispatch line for its wnum and the excited steps the timed
call ran in each form ("gs_onepass_steps", "gs_sequential_steps").
--mixed "64,50,37x50x23": one line per B instead -- the members cycle through these shapes (N is N x N x N) in ONE mixed-shape batch
(Batch(members, mixed_shapes=True)), timed as above ("mixed_*"), and the same members run as one uniform batch per shape, one
batch after another ("uniform": a row per shape; "uniform_sum_*": their times added).  "ratio_host" / "ratio_events": the uniform
batches' summed time over the mixed batch's; "parity": every member's phi bit-identical in both.
With --wnum K (and --gs-variant V) the --mixed line times excited-state steps: the mixed batch is made with state stores
(Batch(members, mixed_shapes=True, state_stores=True)), every member gets an orthonormal store of K states, both sides run
evolve(steps, wnum=K) under the same gs variant; the same "ratio_*" and "parity" fields, plus "wnum", "gs_variant", the mixed batch's
gs_dispatch line and the excited steps each form ran.
--resample SX: a mode of its own -- one SX^3 source (seeded random) onto the potential of every member.  One line per B: the members are
--sizes' first size, or cycle through --mixed's shapes in one mixed-shape batch.  "batch_host_ms": host clock around
Batch.resample_potential(source) (one upload, one transpose, one launch, then every member's potential bookkeeping; the call returns
when it is done), "batch_events_ms": HIP events around the upload, transpose and launch alone (Batch.last_resample_ms), "ctx_host_ms":
host clock around B Contexts each calling set_potential_resampled(source) one after another -- what a user does without the batched
call.  --reps repetitions after one warm-up, every one listed; "ratio_host": ctx over batch, per repetition.  "parity": phi of the
first and the last member after Batch.resample_phi(source) bit-identical to a Context's upload_phi_resampled.
The lines are appended to profiles/batch_resample_rows.jsonl unless --out names another file.
--resample-contexts-only times the contexts alone (it runs on a tree without the batched call) and writes "ctx_host_ms" only.
--setup B: a mode of its own -- B members (--sizes' first size, or cycling through --mixed's shapes) set up from nothing: "batched_ms":
host clock around Batch.set_initial_conditions + Batch.set_potentials (one launch each, one range check and one read-back; the call
returns when the device has finished), "per_member_ms": around the loops of set_initial_condition and set_potential over the members
of the same batch -- the code path a batch has without the batched calls, unchanged.  Both write the same potentials (Harmonic, Coulomb,
SimpleCornell, Cube in turn) and starts (Boolean, Gaussian, Constant, Coulomb).  The parts are listed too ("*_potentials_ms",
"*_starts_ms": the starts alone do not wait for the device).  --reps repetitions after one warm-up of each, every one listed; "ratio":
per_member over batched, per repetition; "parity": V and phi of the first and the last member bit-identical after either; "setup_counts":
the launches and read-backs one batched repetition adds.  Appended to profiles/batch_setup_rows.jsonl unless --out names another file.
--ritz K: a mode of its own -- Rayleigh-Ritz on K stored states per member (orthonormal, seeded random; Harmonic).  One line per B: the
members are --sizes' first size, or cycle through --mixed's shapes in one mixed-shape batch with state stores.  "batch_matrices_ms": host
clock around Batch.ritz_matrices(K) (two launches and one read-back for all members: it returns with the sums), "ctx_matrices_ms": around
B Contexts holding the same states calling ritz_matrices(K) one after another -- what a user does without the batched call;
"batch_ritz_ms" / "ctx_ritz_ms": the same for Batch.ritz(K) and the contexts' ritz(K), each side followed by a download of the last
member's state 0, which waits for the rotation.  --reps repetitions after one warm-up of each, every one listed, with "*_spread" =
(max - min) / median; "ratio_*": ctx over batch, per repetition.  "parity": every member's h, s and every rotated state bit-identical on
both sides after the last repetition; "ritz_counts": the launches and read-backs one Batch.ritz adds.  Appended to
profiles/batch_ritz_rows.jsonl unless --out names another file.

--moments K: a mode of its own -- Batch.moments on K stored states per member (the stores of --ritz).  One line per B: "batch_moments_ms",
"batch_ritz_matrices_ms" (the same stores, for scale: that call also reads V and the neighbours) and "ctx_moments_ms" (B Contexts calling
moments one after another), `--reps` repetitions after one warm-up, all listed; "parity": every member's five matrices == on both sides.

--residuals K: a mode of its own -- Batch.residuals on K stored states per member (the stores of --ritz).  One line per B:
"batch_given_ms" / "ctx_given_ms": the wall clock around Batch.residuals(K, theta) (two launches and one read-back for all members) and
around B Contexts calling residuals(K, theta) one after another; "batch_rayleigh_ms" / "ctx_rayleigh_ms": the same with theta=None (two
passes); one warm-up, then --reps repetitions, all listed; "parity": every member's theta, r2 and norm2 compared == on both sides in both
modes; "residual_counts_*": the launches and read-backs one call adds.  Appended to profiles/batch_residual_rows.jsonl unless --out names
another file.

--store-step K: a mode of its own -- Batch.evolve_states on K stored states per member (the stores of --ritz; every size of --sizes, Harmonic).
One line per B, HIP events around the launches of --steps steps (an even number: no trailing copy), one warm-up call of --warmup steps,
then --reps repetitions, all listed: "store_us_per_step" and "store_gups" (B x K x cells x steps / time) for Batch.evolve_states(steps, K);
"dup_us_per_step" / "dup_gups" for Batch.evolve(steps) on a batch of B x K members (the same cells stepped, with V and a, b duplicated per
state; one step per launch, the default dispatch); "gs_us_per_step" / "gs_gups" (B x cells x steps / time) for Batch.evolve(steps,
wnum=K-1) on the B members -- what an excited step costs today.  "ratio_dup": dup over store, per repetition.  "parity": every state of
the first and the last member bit-identical to a Context's evolve(0, steps) from the same state.  "store_dispatch": the kernel line;
"store_launches": what one timed call adds.  Appended to profiles/batch_store_step_rows.jsonl unless --out names another file.

--filter K: a mode of its own -- Batch.filter_states on K stored states per member beside Batch.evolve_states on the same batch in the same
session (the arguments of --store-step).  One line per B, HIP events around the launches: --steps filter steps per repetition, in calls of an
even degree of at most 200 (no trailing copy), after --warmup steps; the interval is a0 = 0 < a = 10 < b = each member's spectral_bound()
(V >= 0: nothing grows).  "filter_us_per_step" / "filter_gups" and "store_us_per_step" / "store_gups" (B x K x cells x steps / time),
"ratio_filter": filter over store, per repetition.  "parity": before anything is timed, every state of the first and the last member after a
call of degree "parity_degree" == tests/filter_model.py's on the bits.  "solver": with --solver, one solve_filtered and one solve_block of the
loaded batch (k = K, wall clock, blocks, stencil passes per state) -- they stop on different rules and converge to different numbers.
Appended to profiles/batch_filter_rows.jsonl unless --out names another file."""
import argparse, json, os, sys, threading, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import wafer_amd


def members(n, B, ext=1, dtype="f64"):
    return [wafer_amd.Params(n, n, n, dn=0.2, dt=0.002 + 0.008 * k / max(1, B), mass=1.0, central_difference=ext, dtype=dtype) for k in range(B)]


def store(par, wnum, seed=0):
    """wnum orthonormal states on the padded grid (zero frame)"""
    e = par.ext
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((par.nx * par.ny * par.nz, wnum)))
    out = []
    for i in range(wnum):
        s = np.zeros(par.padded_shape)
        s[e:-e, e:-e, e:-e] = q[:, i].reshape(par.work_shape)
        out.append(s)
    return out


def row(n, B, steps, warmup, only_batch=False, wnum=0, variant=-1, ext=1, dtype="f64", gs_variant=-1):
    pars = members(n, B, ext, dtype)
    cells = n ** 3
    out = {"shape": [n, n, n], "B": B, "steps": steps, "warmup": warmup, "stencil": ("ThreePoint", "FivePoint", "SevenPoint")[ext - 1], "dtype": dtype,
           "potential": "Harmonic"}
    if wnum:
        out["wnum"] = wnum
        stores = [store(pars[0], wnum, seed=k) for k in range(min(B, 4))]   # (four stores shared out over the members)
    with wafer_amd.Batch(pars) as b:
        for k in range(B):
            b.set_potential(k, "Harmonic")
            b.set_initial_condition(k, "Gaussian")
            for i in range(wnum):
                b.load_state(k, i, stores[k % len(stores)][i])
        b.set_step_variant(variant)
        out["variant"], out["steps_per_launch"], out["dispatch"] = variant, b.steps_per_launch(), b.dispatch()
        b.set_gs_variant(gs_variant)
        out["gs_variant"], out["gs_dispatch"] = gs_variant, b.gs_dispatch(wnum)
        b.evolve(warmup, wnum=wnum)
        b.last_evolve_ms()   # (waits for the warm-up)
        p0, g0 = b.passes(), b.gs_steps()
        t0 = time.perf_counter()
        b.evolve(steps, wnum=wnum)
        ms, st = b.last_evolve_ms()   # blocks until the last step has finished
        t = time.perf_counter() - t0
        out["batch_host_us_per_step"] = 1e6 * t / steps
        out["batch_host_gups"] = B * cells * steps / t / 1e9
        out["kernel"] = b.kernel_name()
        out["fused_passes"], out["single_steps"] = [x - y for x, y in zip(b.passes(), p0)]
        out["gs_onepass_steps"], out["gs_sequential_steps"] = [x - y for x, y in zip(b.gs_steps(), g0)]
        out["batch_us_per_step"] = 1e3 * ms / st
        out["batch_gups"] = B * cells * st / (ms * 1e-3) / 1e9
        if only_batch:
            return out
        with wafer_amd.Context(pars[0]) as ctx:   # parity of member 0 in the same run
            ctx.set_potential("Harmonic")
            ctx.set_initial_condition("Gaussian")
            for i in range(wnum):
                ctx.load_state(i, stores[0][i])
            ctx.evolve(wnum, warmup)
            ctx.evolve(wnum, steps)
            if wnum:   # the project's excited-state bar, 1e-13 per cell (the two partition their sums differently: not bit for bit)
                want = ctx.download_phi()
                err = float(np.max(np.abs(want - b.download_phi(0))))
                bar = 1e-13 if dtype == "f64" else 4.0 * float(np.spacing(np.float32(np.max(np.abs(want)))))
                out["parity"], out["parity_max_abs"] = bool(err <= bar), "%.2e" % err
            else:
                out["parity"] = bool(np.array_equal(ctx.download_phi().view(np.int64), b.download_phi(0).view(np.int64)))
    ctxs = [wafer_amd.Context(p) for p in pars]
    try:
        for k, c in enumerate(ctxs):
            c.set_potential("Harmonic")
            c.set_initial_condition("Gaussian")
            for i in range(wnum):
                c.load_state(i, stores[k % len(stores)][i])
            c.evolve(wnum, warmup)
            c.synchronize()
        out["single_kernel"] = ctxs[0].stencil_kernel_name()
        t0 = time.perf_counter()
        for c in ctxs:
            c.evolve(wnum, steps)
            c.synchronize()
        t = time.perf_counter() - t0
        out["seq_us_per_step"] = 1e6 * t / steps
        out["seq_gups"] = B * cells * steps / t / 1e9

        def work(c):
            c.evolve(wnum, steps)
            c.synchronize()
        ths = [threading.Thread(target=work, args=(c,)) for c in ctxs]
        t0 = time.perf_counter()
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        t = time.perf_counter() - t0
        out["thr_us_per_step"] = 1e6 * t / steps
        out["thr_gups"] = B * cells * steps / t / 1e9
    finally:
        for c in ctxs:
            c.close()
    out["speedup_vs_seq"] = out["batch_host_gups"] / out["seq_gups"]
    out["speedup_vs_thr"] = out["batch_host_gups"] / out["thr_gups"]
    return out


def parse_shapes(text):
    out = []
    for tok in text.split(","):
        d = [int(x) for x in tok.strip().lower().split("x")]
        if len(d) not in (1, 3) or min(d) < 1:
            raise SystemExit("--mixed: a shape is N or NXxNYxNZ, got %r" % tok)
        out.append(tuple(d * 3 if len(d) == 1 else d))
    return out


def timed_batch(pars, steps, warmup, variant, mixed, wnum=0, gs_variant=-1, stores=None):
    """-> (timings, [phi of every member]) of one batch of these members after warmup + steps steps (wnum > 0: excited-state steps
    against stores[k], member k's orthonormal states; a mixed batch is then made with state stores)"""
    cells = sum(p.nx * p.ny * p.nz for p in pars)
    kind = dict(mixed_shapes=True, state_stores=True) if mixed and wnum else dict(mixed_shapes=mixed)
    with wafer_amd.Batch(pars, **kind) as b:
        for k in range(len(pars)):
            b.set_potential(k, "Harmonic")
            b.set_initial_condition(k, "Gaussian")
            for i in range(wnum):
                b.load_state(k, i, stores[k][i])
        b.set_step_variant(variant)
        out = {"B": len(pars), "dispatch": b.dispatch(), "shapes": b.num_shapes()}
        if wnum:
            b.set_gs_variant(gs_variant)
            out["gs_dispatch"] = b.gs_dispatch(wnum)
        b.evolve(warmup, wnum=wnum)
        b.last_evolve_ms()
        p0, g0 = b.passes(), b.gs_steps()
        t0 = time.perf_counter()
        b.evolve(steps, wnum=wnum)
        ms, st = b.last_evolve_ms()
        t = time.perf_counter() - t0
        out["host_us_per_step"] = 1e6 * t / steps
        out["host_gups"] = cells * steps / t / 1e9
        out["us_per_step"] = 1e3 * ms / st
        out["gups"] = cells * st / (ms * 1e-3) / 1e9
        out["fused_passes"], out["single_steps"] = [x - y for x, y in zip(b.passes(), p0)]
        if wnum:
            out["gs_onepass_steps"], out["gs_sequential_steps"] = [x - y for x, y in zip(b.gs_steps(), g0)]
        return out, [b.download_phi(k) for k in range(len(pars))]


def mixed_row(shapes, B, steps, warmup, variant=-1, ext=1, dtype="f64", wnum=0, gs_variant=-1):
    pars = [wafer_amd.Params(*shapes[k % len(shapes)], dn=0.2, dt=0.002 + 0.008 * k / max(1, B), mass=1.0, central_difference=ext, dtype=dtype)
            for k in range(B)]
    out = {"mixed": [list(s) for s in shapes], "B": B, "steps": steps, "warmup": warmup, "stencil": ("ThreePoint", "FivePoint", "SevenPoint")[ext - 1],
           "dtype": dtype, "potential": "Harmonic", "variant": variant}
    stores = None
    if wnum:
        out["wnum"], out["gs_variant"] = wnum, gs_variant
        per_shape = {s: [store(pars[shapes.index(s)], wnum, seed=j) for j in range(2)] for s in dict.fromkeys(shapes)}   # (two stores per shape, shared out)
        stores = [per_shape[shapes[k % len(shapes)]][(k // len(shapes)) % 2] for k in range(B)]
    m, phis = timed_batch(pars, steps, warmup, variant, True, wnum, gs_variant, stores)
    out.update({"mixed_" + k: v for k, v in m.items() if k != "B"})
    out["uniform"], parity = [], True
    for s in dict.fromkeys(shapes):   # one uniform batch per distinct shape, one after another
        idx = [k for k in range(B) if shapes[k % len(shapes)] == s]
        if not idx:
            continue
        u, uphis = timed_batch([pars[k] for k in idx], steps, warmup, variant, False, wnum, gs_variant, stores and [stores[k] for k in idx])
        u.pop("gs_dispatch", None)
        u["shape"] = list(s)
        u["dispatch"] = u["dispatch"]["kernel"]
        out["uniform"].append(u)
        parity = parity and all(np.array_equal(phis[k].view(np.int64), uphis[j].view(np.int64)) for j, k in enumerate(idx))
    for key in ("host_us_per_step", "us_per_step"):
        out["uniform_sum_" + key] = sum(u[key] for u in out["uniform"])
    out["ratio_host"] = out["uniform_sum_host_us_per_step"] / out["mixed_host_us_per_step"]
    out["ratio_events"] = out["uniform_sum_us_per_step"] / out["mixed_us_per_step"]
    out["parity"] = bool(parity)
    return out


def resample_row(shapes, B, sx, reps, ext=1, dtype="f64", contexts_only=False):
    pars = [wafer_amd.Params(*shapes[k % len(shapes)], dn=0.2, dt=0.002 + 0.008 * k / max(1, B), mass=1.0, central_difference=ext, dtype=dtype)
            for k in range(B)]
    src = np.random.default_rng(sx).standard_normal((sx, sx, sx))
    out = {"mode": "resample", "target": "potential", "source": [sx, sx, sx], "shapes": [list(s) for s in shapes], "B": B, "reps": reps,
           "stencil": ("ThreePoint", "FivePoint", "SevenPoint")[ext - 1], "dtype": dtype, "basis": "padded"}
    ctxs = [wafer_amd.Context(p) for p in pars]
    try:
        for c in ctxs:   # warm-up
            c.set_potential_resampled(src)
        out["ctx_host_ms"] = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for c in ctxs:
                c.set_potential_resampled(src)   # (returns when the device has finished: it reads V's range back)
            out["ctx_host_ms"].append(1e3 * (time.perf_counter() - t0))
        if contexts_only:
            return out
        with wafer_amd.Batch(pars, mixed_shapes=len(set(shapes)) > 1) as b:
            b.resample_potential(src)   # warm-up: the scratch is made here
            out["batch_host_ms"], out["batch_events_ms"] = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                b.resample_potential(src)
                out["batch_host_ms"].append(1e3 * (time.perf_counter() - t0))
                out["batch_events_ms"].append(b.last_resample_ms())
            b.resample_phi(src)
            parity = True
            for k in sorted({0, B - 1}):
                ctxs[k].upload_phi_resampled(src)
                parity = parity and bool(np.array_equal(ctxs[k].download_phi().view(np.int64), b.download_phi(k).view(np.int64)))
            out["parity"] = parity
            out["shapes_in_batch"] = b.num_shapes()
        out["ratio_host"] = [c / h for c, h in zip(out["ctx_host_ms"], out["batch_host_ms"])]
    finally:
        for c in ctxs:
            c.close()
    return out


SETUP_POTENTIALS = ["Harmonic", "Coulomb", "SimpleCornell", "Cube"]
SETUP_STARTS = ["Boolean", "Gaussian", "Constant", "Coulomb"]


def setup_row(shapes, B, reps, ext=1, dtype="f64"):
    pars = [wafer_amd.Params(*shapes[k % len(shapes)], dn=0.2, dt=0.002 + 0.008 * k / max(1, B), mass=1.0, central_difference=ext, dtype=dtype)
            for k in range(B)]
    pots = [SETUP_POTENTIALS[k % 4] for k in range(B)]
    starts = [SETUP_STARTS[k % 4] for k in range(B)]
    seeds = [100 + k for k in range(B)]
    out = {"mode": "setup", "shapes": [list(s) for s in shapes], "B": B, "reps": reps, "stencil": ("ThreePoint", "FivePoint", "SevenPoint")[ext - 1],
           "dtype": dtype, "potentials": SETUP_POTENTIALS, "starts": SETUP_STARTS}
    keys = ("batched_ms", "batched_starts_ms", "batched_potentials_ms", "per_member_ms", "per_member_starts_ms", "per_member_potentials_ms")
    for k in keys:
        out[k] = []

    def batched(b):
        t0 = time.perf_counter()
        b.set_initial_conditions(starts, seeds=seeds)
        t1 = time.perf_counter()
        b.set_potentials(pots)   # (its read-back waits for the stream: the starts have been written too)
        t2 = time.perf_counter()
        return 1e3 * (t2 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1)

    def per_member(b):
        t0 = time.perf_counter()
        for k in range(B):
            b.set_initial_condition(k, starts[k], seed=seeds[k])
        t1 = time.perf_counter()
        for k in range(B):
            b.set_potential(k, pots[k])   # (each reads V's range back: the last one waits for everything)
        t2 = time.perf_counter()
        return 1e3 * (t2 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1)

    def bits(b):
        return [x.view(np.int64) for k in sorted({0, B - 1}) for x in (b.download_array(k, "v"), b.download_phi(k))]

    with wafer_amd.Batch(pars, mixed_shapes=len(set(shapes)) > 1) as b:
        batched(b)       # warm-up of each
        per_member(b)
        for _ in range(reps):   # (nothing but the timed calls in here: a download allocates and frees its staging buffer)
            for key, val in zip(keys[:3], batched(b)):
                out[key].append(val)
            for key, val in zip(keys[3:], per_member(b)):
                out[key].append(val)
        c0 = b.setup_counts()
        batched(b)
        out["setup_counts"] = [x - y for x, y in zip(b.setup_counts(), c0)]
        got = bits(b)
        per_member(b)
        out["parity"] = all(np.array_equal(x, y) for x, y in zip(got, bits(b)))
        out["shapes_in_batch"] = b.num_shapes()
    out["ratio"] = [p / q for p, q in zip(out["per_member_ms"], out["batched_ms"])]
    return out


def ritz_row(shapes, B, K, reps, ext=1, dtype="f64"):
    pars = [wafer_amd.Params(*shapes[k % len(shapes)], dn=0.2, dt=0.002 + 0.008 * k / max(1, B), mass=1.0, central_difference=ext, dtype=dtype,
                             max_states=K) for k in range(B)]
    out = {"mode": "ritz", "k": K, "shapes": [list(s) for s in shapes], "B": B, "reps": reps, "stencil": ("ThreePoint", "FivePoint", "SevenPoint")[ext - 1],
           "dtype": dtype, "potential": "Harmonic"}
    per_shape = {s: [store(pars[shapes.index(s)], K, seed=j) for j in range(2)] for s in dict.fromkeys(shapes)}   # (two stores per shape, shared out)
    stores = [per_shape[shapes[k % len(shapes)]][(k // len(shapes)) % 2] for k in range(B)]
    keys = ("batch_matrices_ms", "ctx_matrices_ms", "batch_ritz_ms", "ctx_ritz_ms")
    for key in keys:
        out[key] = []
    mixed = len(set(shapes)) > 1
    ctxs = [wafer_amd.Context(p) for p in pars]
    try:
        with wafer_amd.Batch(pars, mixed_shapes=mixed, state_stores=mixed) as b:
            b.set_potentials(["Harmonic"] * B)
            for k, c in enumerate(ctxs):
                c.set_potential("Harmonic")
                for i in range(K):
                    c.load_state(i, stores[k][i])
                    b.load_state(k, i, stores[k][i])

            def batch_matrices():
                t0 = time.perf_counter()
                res = b.ritz_matrices(K)
                return 1e3 * (time.perf_counter() - t0), res

            def ctx_matrices():
                t0 = time.perf_counter()
                res = [c.ritz_matrices(K) for c in ctxs]
                return 1e3 * (time.perf_counter() - t0), res

            def batch_ritz():
                t0 = time.perf_counter()
                b.ritz(K)
                b.download_state(B - 1, 0)   # (waits for the rotation)
                return 1e3 * (time.perf_counter() - t0)

            def ctx_ritz():
                t0 = time.perf_counter()
                for c in ctxs:
                    c.ritz(K)
                ctxs[-1].download_state(0)
                return 1e3 * (time.perf_counter() - t0)

            batch_matrices(), ctx_matrices(), batch_ritz(), ctx_ritz()   # warm-up of each: the buffers are made here
            for _ in range(reps):
                out["batch_matrices_ms"].append(batch_matrices()[0])
                out["ctx_matrices_ms"].append(ctx_matrices()[0])
                out["batch_ritz_ms"].append(batch_ritz())
                out["ctx_ritz_ms"].append(ctx_ritz())
            c0 = b.ritz_counts()
            batch_ritz()
            ctx_ritz()
            out["ritz_counts"] = [x - y for x, y in zip(b.ritz_counts(), c0)]
            same = lambda x, y: bool(np.array_equal(np.ascontiguousarray(x).view(np.int64), np.ascontiguousarray(y).view(np.int64)))
            parity = True
            for (bh, bs), (ch, cs) in zip(batch_matrices()[1], ctx_matrices()[1]):
                parity = parity and same(bh, ch) and same(bs, cs)
            for k, c in enumerate(ctxs):
                parity = parity and all(same(b.download_state(k, i), c.download_state(i)) for i in range(K))
            out["parity"] = parity
            out["shapes_in_batch"] = b.num_shapes()
    finally:
        for c in ctxs:
            c.close()
    for key in keys:
        out[key.replace("_ms", "_spread")] = (max(out[key]) - min(out[key])) / float(np.median(out[key]))
    out["ratio_matrices"] = [c / h for c, h in zip(out["ctx_matrices_ms"], out["batch_matrices_ms"])]
    out["ratio_ritz"] = [c / h for c, h in zip(out["ctx_ritz_ms"], out["batch_ritz_ms"])]
    return out


def residual_row(shapes, B, K, reps, ext=1, dtype="f64"):
    """Batch.residuals on K stored states per member against B contexts calling residuals one after another, theta given and in
    Rayleigh mode; every member's theta, r2 and norm2 compared == on both sides"""
    pars = [wafer_amd.Params(*shapes[k % len(shapes)], dn=0.2, dt=0.002 + 0.008 * k / max(1, B), mass=1.0, central_difference=ext, dtype=dtype,
                             max_states=K) for k in range(B)]
    out = {"mode": "residuals", "k": K, "shapes": [list(s) for s in shapes], "B": B, "reps": reps,
           "stencil": ("ThreePoint", "FivePoint", "SevenPoint")[ext - 1], "dtype": dtype, "potential": "Harmonic"}
    per_shape = {s: [store(pars[shapes.index(s)], K, seed=j) for j in range(2)] for s in dict.fromkeys(shapes)}   # (two stores per shape, shared out)
    stores = [per_shape[shapes[k % len(shapes)]][(k // len(shapes)) % 2] for k in range(B)]
    keys = ("batch_given_ms", "ctx_given_ms", "batch_rayleigh_ms", "ctx_rayleigh_ms")
    for key in keys:
        out[key] = []
    theta = [[1.0 + 0.5 * j for j in range(K)]] * B
    mixed = len(set(shapes)) > 1
    ctxs = [wafer_amd.Context(p) for p in pars]
    try:
        with wafer_amd.Batch(pars, mixed_shapes=mixed, state_stores=mixed) as b:
            b.set_potentials(["Harmonic"] * B)
            for k, c in enumerate(ctxs):
                c.set_potential("Harmonic")
                for i in range(K):
                    c.load_state(i, stores[k][i])
                    b.load_state(k, i, stores[k][i])

            def batch(th):
                t0 = time.perf_counter()
                res = b.residuals(K, theta=th)
                return 1e3 * (time.perf_counter() - t0), res

            def contexts(th):
                t0 = time.perf_counter()
                res = [c.residuals(K, theta=None if th is None else th[k]) for k, c in enumerate(ctxs)]
                return 1e3 * (time.perf_counter() - t0), res

            batch(theta), contexts(theta), batch(None), contexts(None)   # warm-up of each: the buffers are made here
            for _ in range(reps):
                out["batch_given_ms"].append(batch(theta)[0])
                out["ctx_given_ms"].append(contexts(theta)[0])
                out["batch_rayleigh_ms"].append(batch(None)[0])
                out["ctx_rayleigh_ms"].append(contexts(None)[0])
            c0 = b.residual_counts()
            batch(theta)
            c1 = b.residual_counts()
            batch(None)
            out["residual_counts_given"] = [x - y for x, y in zip(c1, c0)]
            out["residual_counts_rayleigh"] = [x - y for x, y in zip(b.residual_counts(), c1)]
            same = lambda x, y: bool(np.array_equal(np.ascontiguousarray(x).view(np.int64), np.ascontiguousarray(y).view(np.int64)))
            parity = True
            for th in (theta, None):
                for br, cr in zip(batch(th)[1], contexts(th)[1]):
                    parity = parity and all(same(br[name], cr[name]) for name in ("theta", "r2", "norm2"))
            out["parity"] = parity
            out["shapes_in_batch"] = b.num_shapes()
    finally:
        for c in ctxs:
            c.close()
    for key in keys:
        out[key.replace("_ms", "_spread")] = (max(out[key]) - min(out[key])) / float(np.median(out[key]))
    out["ratio_given"] = [c / h for c, h in zip(out["ctx_given_ms"], out["batch_given_ms"])]
    out["ratio_rayleigh"] = [c / h for c, h in zip(out["ctx_rayleigh_ms"], out["batch_rayleigh_ms"])]
    return out


def moment_row(shapes, B, K, reps, ext=1, dtype="f64"):
    """Batch.moments on K stored states per member beside Batch.ritz_matrices on the same stores and against B contexts calling
    moments one after another; every member's five matrices compared == on both sides"""
    pars = [wafer_amd.Params(*shapes[k % len(shapes)], dn=0.2, dt=0.002 + 0.008 * k / max(1, B), mass=1.0, central_difference=ext, dtype=dtype,
                             max_states=K) for k in range(B)]
    out = {"mode": "moments", "k": K, "shapes": [list(s) for s in shapes], "B": B, "reps": reps,
           "stencil": ("ThreePoint", "FivePoint", "SevenPoint")[ext - 1], "dtype": dtype}
    per_shape = {s: [store(pars[shapes.index(s)], K, seed=j) for j in range(2)] for s in dict.fromkeys(shapes)}   # (two stores per shape, shared out)
    stores = [per_shape[shapes[k % len(shapes)]][(k // len(shapes)) % 2] for k in range(B)]
    keys = ("batch_moments_ms", "batch_ritz_matrices_ms", "ctx_moments_ms")
    for key in keys:
        out[key] = []
    mixed = len(set(shapes)) > 1
    ctxs = [wafer_amd.Context(p) for p in pars]
    try:
        with wafer_amd.Batch(pars, mixed_shapes=mixed, state_stores=mixed) as b:
            b.set_potentials(["Harmonic"] * B)
            for k, c in enumerate(ctxs):
                for i in range(K):
                    c.load_state(i, stores[k][i])
                    b.load_state(k, i, stores[k][i])

            def timed_call(fn):
                t0 = time.perf_counter()
                res = fn()
                return 1e3 * (time.perf_counter() - t0), res

            calls = (lambda: b.moments(K), lambda: b.ritz_matrices(K), lambda: [c.moments(K) for c in ctxs])
            for fn in calls:                                 # warm-up of each: the buffers are made here
                fn()
            for _ in range(reps):
                for key, fn in zip(keys, calls):
                    out[key].append(timed_call(fn)[0])
            c0 = b.moment_counts()
            got = b.moments(K)
            out["moment_counts"] = [x - y for x, y in zip(b.moment_counts(), c0)]
            same = lambda x, y: bool(np.array_equal(np.ascontiguousarray(x).view(np.int64), np.ascontiguousarray(y).view(np.int64)))
            out["parity"] = all(same(br[name], cr[name]) for br, cr in zip(got, calls[2]()) for name in ("s", "x", "y", "z", "r2"))
            out["shapes_in_batch"] = b.num_shapes()
    finally:
        for c in ctxs:
            c.close()
    for key in keys:
        out[key.replace("_ms", "_spread")] = (max(out[key]) - min(out[key])) / float(np.median(out[key]))
    out["ratio_contexts_over_batch"] = [c / h for c, h in zip(out["ctx_moments_ms"], out["batch_moments_ms"])]
    out["ratio_ritz_matrices_over_moments"] = [r / h for r, h in zip(out["batch_ritz_matrices_ms"], out["batch_moments_ms"])]
    return out


def store_step_row(n, B, K, steps, warmup, reps, ext=1, dtype="f64"):
    """Batch.evolve_states(steps, K) on B members against Batch.evolve on B x K members and against excited steps with wnum = K - 1"""
    steps += steps % 2   # (an even number of steps: no trailing copy in the timed calls)
    pars = [wafer_amd.Params(n, n, n, dn=0.2, dt=0.002 + 0.008 * k / max(1, B), mass=1.0, central_difference=ext, dtype=dtype, max_states=K)
            for k in range(B)]
    cells = n ** 3
    out = {"mode": "store_step", "k": K, "shape": [n, n, n], "B": B, "steps": steps, "warmup": warmup, "reps": reps,
           "stencil": ("ThreePoint", "FivePoint", "SevenPoint")[ext - 1], "dtype": dtype, "potential": "Harmonic"}
    stores = [store(pars[0], K, seed=j) for j in range(2)]   # (two stores, shared out)
    for key in ("store_us_per_step", "dup_us_per_step", "gs_us_per_step"):
        out[key] = []
    same = lambda x, y: bool(np.array_equal(np.ascontiguousarray(x).view(np.int64), np.ascontiguousarray(y).view(np.int64)))
    with wafer_amd.Batch(pars) as b:
        b.set_potentials(["Harmonic"] * B)
        b.set_initial_conditions(["Gaussian"] * B)
        for k in range(B):
            for i in range(K):
                b.load_state(k, i, stores[k % 2][i])
        out["store_dispatch"] = b.store_dispatch()
        parity = True
        for k in sorted({0, B - 1}):   # before anything is timed: `steps` steps of every state against a context
            with wafer_amd.Context(pars[k]) as ctx:
                ctx.set_potential("Harmonic")
                want = []
                for i in range(K):
                    ctx.upload_phi(stores[k % 2][i])
                    ctx.evolve(0, steps)
                    want.append(ctx.download_phi())
            b.evolve_states(steps, K, active=[int(m == k) for m in range(B)])
            parity = parity and all(same(b.download_state(k, i), want[i]) for i in range(K))
        out["parity"] = parity
        b.evolve_states(warmup + warmup % 2, K)
        b.last_evolve_ms()
        c0 = b.store_counts()
        for _ in range(reps):
            b.evolve_states(steps, K)
            ms, st = b.last_evolve_ms()
            out["store_us_per_step"].append(1e3 * ms / st)
        out["store_launches"] = (b.store_counts() - c0) // reps
        if K > 1:   # excited steps against K - 1 of the (no longer orthonormal, but that costs the same) states
            b.evolve(warmup, wnum=K - 1)
            b.last_evolve_ms()
            for _ in range(reps):
                b.evolve(steps, wnum=K - 1)
                ms, st = b.last_evolve_ms()
                out["gs_us_per_step"].append(1e3 * ms / st)
            out["gs_dispatch"] = b.gs_dispatch(K - 1)
    dup = [pars[k // K] for k in range(B * K)]
    with wafer_amd.Batch(dup) as d:
        d.set_potentials(["Harmonic"] * (B * K))
        d.set_initial_conditions(["Gaussian"] * (B * K))
        out["dup_dispatch"] = d.dispatch()["kernel"]
        d.evolve(warmup)
        d.last_evolve_ms()
        for _ in range(reps):
            d.evolve(steps)
            ms, st = d.last_evolve_ms()
            out["dup_us_per_step"].append(1e3 * ms / st)
    out["store_gups"] = [B * K * cells / (us * 1e-6) / 1e9 for us in out["store_us_per_step"]]
    out["dup_gups"] = [B * K * cells / (us * 1e-6) / 1e9 for us in out["dup_us_per_step"]]
    out["gs_gups"] = [B * cells / (us * 1e-6) / 1e9 for us in out["gs_us_per_step"]]
    out["ratio_dup"] = [x / y for x, y in zip(out["dup_us_per_step"], out["store_us_per_step"])]
    return out


def filter_row(n, B, K, steps, warmup, reps, ext=1, dtype="f64", solver=False):
    """Batch.filter_states beside Batch.evolve_states on the same B members and K states.  The timed calls put the anchor a0 at
    Harmonic's lowest level (about 1.5), so that a call of degree 200 leaves the lowest component of a state about as large as it
    was: the timed data neither collapse nor grow ("end_max_abs": the largest magnitude in member 0's first state after the last
    timed call, with the plain steps of evolve_states in between)."""
    from tests import filter_model as fm
    steps += steps % 2
    pars = [wafer_amd.Params(n, n, n, dn=0.2, dt=0.002 + 0.008 * k / max(1, B), mass=1.0, central_difference=ext, dtype=dtype, max_states=K)
            for k in range(B)]
    cells = n ** 3
    out = {"mode": "filter", "k": K, "shape": [n, n, n], "B": B, "steps": steps, "warmup": warmup, "reps": reps,
           "stencil": ("ThreePoint", "FivePoint", "SevenPoint")[ext - 1], "dtype": dtype, "potential": "Harmonic", "parity_degree": 4}
    stores = [store(pars[0], K, seed=j) for j in range(2)]   # (two stores, shared out)
    storage = np.float64 if dtype == "f64" else np.float32
    same = lambda x, y: bool(np.array_equal(np.ascontiguousarray(x).view(np.int64), np.ascontiguousarray(y).view(np.int64)))

    def calls(total):
        """even degrees of at most 200 that add up to `total` (even)"""
        d = []
        while total > 0:
            d.append(min(200, total))
            total -= d[-1]
        return d

    with wafer_amd.Batch(pars) as b:
        b.set_potentials(["Harmonic"] * B)
        b.set_initial_conditions(["Gaussian"] * B)

        def load():
            for k in range(B):
                for i in range(K):
                    b.load_state(k, i, stores[k % 2][i])

        load()
        ub = b.spectral_bound()
        a0, a = 1.5, 10.0
        out["interval"] = {"a0": a0, "a": a}
        parity = True
        for k in sorted({0, B - 1}):   # before anything is timed
            starts = [b.download_state(k, i) for i in range(K)]   # (as stored: rounded to the storage type)
            b.filter_states(4, a, ub, a0, K, active=[int(m == k) for m in range(B)])
            v = b.download_array(k, "v")
            cfg = fm.Cfg(ext, pars[k].dn, pars[k].mass)
            parity = parity and ub[k] == fm.bound(cfg, v)
            parity = parity and all(same(b.download_state(k, i), fm.filter(cfg, v, starts[i], 4, a, ub[k], a0, storage)) for i in range(K))
        out["parity"] = bool(parity)
        runs = (("filter_us_per_step", lambda d: b.filter_states(d, a, ub, a0, K)), ("store_us_per_step", lambda d: b.evolve_states(d, K)))
        load()
        for key, run in runs:
            out[key] = []
            for d in calls(warmup + warmup % 2):
                run(d)
        b.last_evolve_ms()
        for _ in range(reps):   # the two alternate: what else the machine does meets both alike
            for key, run in runs:
                ms_all = 0.0
                for d in calls(steps):
                    run(d)
                    ms_all += b.last_evolve_ms()[0]
                out[key].append(1e3 * ms_all / steps)
        end = b.download_state(0, 0)
        out["end_max_abs"] = float(np.max(np.abs(end))) if np.all(np.isfinite(end)) else float("nan")
        if solver:
            out["solver"] = {}
            for name, run, per_block in (("solve_filtered", lambda: b.solve_filtered(K, 1e-10, 30, 60), 30), ("solve_block", lambda: b.solve_block(K, 1e-10, 50, 400), 50)):
                load()
                t0 = time.perf_counter()
                rs = run()
                wall = time.perf_counter() - t0
                out["solver"][name] = {"wall_s": wall, "blocks": [r["blocks"] for r in rs], "status": [r["status"] for r in rs],
                                       "passes_per_state": max(r["blocks"] for r in rs) * per_block,
                                       "e0_member0": float(rs[0]["evals"][0]), "max_rho_member0": float(np.max(rs[0]["rho"][:K - 1]))}
    out["filter_gups"] = [B * K * cells / (us * 1e-6) / 1e9 for us in out["filter_us_per_step"]]
    out["store_gups"] = [B * K * cells / (us * 1e-6) / 1e9 for us in out["store_us_per_step"]]
    out["ratio_filter"] = [x / y for x, y in zip(out["filter_us_per_step"], out["store_us_per_step"])]
    return out


def rounded(d):
    if isinstance(d, dict):
        return {k: rounded(v) for k, v in d.items()}
    if isinstance(d, list):
        return [rounded(v) for v in d]
    return round(d, 4) if isinstance(d, float) else d


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[50, 64])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", help="also append the lines to this file")
    ap.add_argument("--only-batch", action="store_true", help="the batch alone, no contexts (counter runs)")
    ap.add_argument("--wnum", type=int, default=0, help="excited-state steps against K stored states per member (default 0: ground state)")
    ap.add_argument("--ext", type=int, choices=[1, 2, 3], default=1, help="central difference: 1 ThreePoint (default), 2 FivePoint, 3 SevenPoint")
    ap.add_argument("--dtype", choices=["f64", "f32", "f32fast"], default="f64", help="storage / arithmetic of the batch and the contexts")
    ap.add_argument("--variant", type=int, choices=[-1, 0, 1], default=-1, help="Batch.set_step_variant: -1 default dispatch, 0 one step per launch, 1 fused passes")
    ap.add_argument("--gs-variant", type=int, choices=[-1, 0, 1], default=-1,
                    help="Batch.set_gs_variant: -1 default dispatch, 0 the sequential chain, 1 the one-pass form (wnum <= 4)")
    ap.add_argument("--mixed", metavar="SHAPES", help='e.g. "64,50,37x50x23": the members cycle through these shapes in one mixed-shape batch, compared '
                    "with one uniform batch per shape run one after another (--wnum, --gs-variant: excited-state steps, the mixed batch with state stores; "
                    "--sizes and --only-batch do not apply)")
    ap.add_argument("--resample", type=int, metavar="SX", help="time Batch.resample_potential of one SX^3 source onto every member against B contexts "
                    "calling set_potential_resampled (a mode of its own: --steps, --warmup, --wnum and the variants do not apply)")
    ap.add_argument("--reps", type=int, default=3, help="--resample: timed repetitions after one warm-up (default 3)")
    ap.add_argument("--resample-contexts-only", action="store_true", help="--resample: the contexts alone")
    ap.add_argument("--setup", type=int, metavar="B", help="time Batch.set_initial_conditions + set_potentials on B members against the loops of "
                    "per-member calls on the same batch (a mode of its own; --reps, --sizes or --mixed, --ext, --dtype apply)")
    ap.add_argument("--ritz", type=int, metavar="K", help="time Batch.ritz_matrices and Batch.ritz on K stored states per member against B contexts "
                    "calling ritz_matrices / ritz one after another (a mode of its own; --batch, --reps, --sizes or --mixed, --ext, --dtype apply)")
    ap.add_argument("--residuals", type=int, metavar="K", help="time Batch.residuals on K stored states per member, theta given and in Rayleigh "
                    "mode, against B contexts calling residuals one after another (a mode of its own; --batch, --reps, --sizes or --mixed, --ext, "
                    "--dtype apply)")
    ap.add_argument("--moments", type=int, metavar="K", help="time Batch.moments on K stored states per member beside Batch.ritz_matrices and against "
                    "B contexts calling moments one after another (a mode of its own; --batch, --reps, --sizes or --mixed, --ext, --dtype apply)")
    ap.add_argument("--store-step", type=int, metavar="K", help="time Batch.evolve_states on K stored states per member against Batch.evolve on "
                    "B x K members and against excited steps with wnum = K - 1 (a mode of its own; --batch, --steps, --warmup, --reps, --sizes, --ext, "
                    "--dtype apply)")
    ap.add_argument("--filter", type=int, metavar="K", help="time Batch.filter_states on K stored states per member beside Batch.evolve_states on the "
                    "same batch (a mode of its own; --batch, --steps, --warmup, --reps, --sizes, --ext, --dtype apply)")
    ap.add_argument("--solver", action="store_true", help="--filter: also one solve_filtered and one solve_block of the batch (k = K)")
    a = ap.parse_args()
    if a.filter:
        if not a.out:
            a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "batch_filter_rows.jsonl")
        for n in a.sizes:
            for B in a.batch:
                row = filter_row(n, B, a.filter, a.steps, a.warmup, a.reps, a.ext, a.dtype, a.solver)
                exact = {key: row.pop(key) for key in ("solver", "end_max_abs") if key in row}   # (energies, rho and magnitudes keep every digit)
                line = json.dumps({**rounded(row), **exact})
                print(line, flush=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        return
    if a.store_step:
        if not a.out:
            a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "batch_store_step_rows.jsonl")
        for n in a.sizes:
            for B in a.batch:
                line = json.dumps(rounded(store_step_row(n, B, a.store_step, a.steps, a.warmup, a.reps, a.ext, a.dtype)))
                print(line, flush=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        return
    if a.moments:
        if not a.out:
            a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "batch_moments_rows.jsonl")
        shapes = parse_shapes(a.mixed) if a.mixed else [(a.sizes[0],) * 3]
        for B in a.batch:
            line = json.dumps(rounded(moment_row(shapes, B, a.moments, a.reps, a.ext, a.dtype)))
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
        return
    if a.residuals:
        if not a.out:
            a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "batch_residual_rows.jsonl")
        shapes = parse_shapes(a.mixed) if a.mixed else [(a.sizes[0],) * 3]
        for B in a.batch:
            line = json.dumps(rounded(residual_row(shapes, B, a.residuals, a.reps, a.ext, a.dtype)))
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
        return
    if a.ritz:
        if not a.out:
            a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "batch_ritz_rows.jsonl")
        shapes = parse_shapes(a.mixed) if a.mixed else [(a.sizes[0],) * 3]
        for B in a.batch:
            line = json.dumps(rounded(ritz_row(shapes, B, a.ritz, a.reps, a.ext, a.dtype)))
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
        return
    if a.setup:
        if not a.out:
            a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "batch_setup_rows.jsonl")
        shapes = parse_shapes(a.mixed) if a.mixed else [(a.sizes[0],) * 3]
        line = json.dumps(rounded(setup_row(shapes, a.setup, a.reps, a.ext, a.dtype)))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        return
    if a.resample:
        if not a.out:   # this mode's rows have a place of their own
            a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "batch_resample_rows.jsonl")
        shapes = parse_shapes(a.mixed) if a.mixed else [(a.sizes[0],) * 3]
        for B in a.batch:
            line = json.dumps(rounded(resample_row(shapes, B, a.resample, a.reps, a.ext, a.dtype, a.resample_contexts_only)))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        return
    if a.mixed:
        for B in a.batch:
            line = json.dumps(rounded(mixed_row(parse_shapes(a.mixed), B, a.steps, a.warmup, a.variant, a.ext, a.dtype, a.wnum, a.gs_variant)))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        return
    for n in a.sizes:
        for B in a.batch:
            line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row(n, B, a.steps, a.warmup, a.only_batch, a.wnum, a.variant, a.ext, a.dtype, a.gs_variant).items()})
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
