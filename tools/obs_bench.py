#!/usr/bin/env python3
"""HIP-event style timing of compute_observables / norm2 at 512^3 (host sync included, median of 20).

    obs_bench.py [n]                          the two rows above
    obs_bench.py [n] --ritz K [--dtype D]     Rayleigh-Ritz on K stored states: ritz_matrices and rotate_states (host sync included,
                                              median of 10), observables and wafer_diag_copy_bw from the same run

    obs_bench.py [n] --residuals K [--dtype D] [--out F]
                                              residuals(K, theta) on K stored states against K calls of observables on the same
                                              states (each on phi after an untimed clone): one warm-up, then three repetitions, all
                                              listed; both read one state and V once per state, 2 K array passes of distinct reads

    obs_bench.py [n] --moments K [--dtype D] [--out F]
                                              moments(K) on K stored states beside ritz_matrices(K) and K calls of observables on the
                                              same states (each on phi after an untimed clone): one warm-up, then three repetitions,
                                              all listed; moments reads K (K + 3) / 2 arrays (per column j the states 0 .. j and l_j)

The --ritz rows count bytes as array passes of n^3 elements: k (k + 2) reads for ritz_matrices (per column the state's own
stencil, V and the k states), 2 k passes for rotate_states (k read, k written) -- whose time includes the k (k - 1) / 2 overlap
passes of the Gram matrix the engine recomputes after every change of the store (at most 6: the matrix covers four states)."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import wafer_amd

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=512)
ap.add_argument("--ritz", type=int, default=0, metavar="K")
ap.add_argument("--residuals", type=int, default=0, metavar="K")
ap.add_argument("--moments", type=int, default=0, metavar="K")
ap.add_argument("--out", help="--residuals, --moments: also append the line to this file")
ap.add_argument("--dtype", default="f64", choices=["f64", "f32", "f32fast"])
args = ap.parse_args()
n, k = args.n, args.ritz or args.residuals or args.moments
env = {a: b for a, b in os.environ.items() if a.startswith("WAFER_")}


def timed(fn, reps):
    fn(); ts = []
    for _ in range(reps):
        ctx.synchronize(); t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return ts


with wafer_amd.Context(wafer_amd.Params(n, n, n, dn=0.05, dt=5e-4, max_states=max(1, k), dtype=args.dtype)) as ctx:
    ctx.set_potential("Coulomb")
    ctx.set_initial_condition("Boolean")
    if not k:
        for name, fn in (("observables", ctx.observables), ("norm2", ctx.norm2)):
            ts = timed(fn, 20)
            print(json.dumps({"op": name, "ms_median_incl_host_sync": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "env": env}))
        sys.exit(0)
    for j in range(k):                       # k independent states: Gaussian noise, a few steps each
        ctx.set_initial_condition("Gaussian", seed=11 + j)
        ctx.evolve(0, 3)
        ctx.normalise(ctx.norm2())
        ctx.push_state()
    if args.moments:
        esz = 8 if args.dtype == "f64" else 4
        passes = k * (k + 3) // 2                          # column j loads l_j and the states 0 .. j

        def call_ms(fn):
            ctx.synchronize(); t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3

        def observables_ms():
            total = 0.0
            for j in range(k):
                ctx.clone_state_to_phi(j); ctx.synchronize(); t0 = time.perf_counter(); ctx.observables(); total += (time.perf_counter() - t0) * 1e3
            return total

        call_ms(lambda: ctx.moments(k)), call_ms(lambda: ctx.ritz_matrices(k)), observables_ms()   # one warm-up of each
        mom, ritz, obs = [], [], []
        for _ in range(3):
            mom.append(call_ms(lambda: ctx.moments(k))); ritz.append(call_ms(lambda: ctx.ritz_matrices(k))); obs.append(observables_ms())
        line = json.dumps({"op": "moments", "n": n, "dtype": args.dtype, "k": k, "moments_ms": [round(t, 4) for t in mom],
                           "ritz_matrices_ms": [round(t, 4) for t in ritz], "observables_x_k_ms": [round(t, 4) for t in obs],
                           "array_passes": passes, "moments_tbps_loads": [round(passes * float(n) ** 3 * esz / (t * 1e-3) / 1e12, 3) for t in mom],
                           "env": env})
        print(line)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        sys.exit(0)
    if args.residuals:
        esz = 8 if args.dtype == "f64" else 4
        distinct = 2.0 * k * float(n) ** 3 * esz          # per state: the state and V, once each
        theta = np.linspace(1.0, 2.0, k)

        def residuals_ms():
            ctx.synchronize(); t0 = time.perf_counter(); ctx.residuals(k, theta=theta); return (time.perf_counter() - t0) * 1e3

        def observables_ms():
            total = 0.0
            for j in range(k):
                ctx.clone_state_to_phi(j); ctx.synchronize(); t0 = time.perf_counter(); ctx.observables(); total += (time.perf_counter() - t0) * 1e3
            return total

        residuals_ms(), observables_ms()                   # one warm-up of each
        res, obs = [], []
        for _ in range(3):
            res.append(residuals_ms()); obs.append(observables_ms())
        tbps = lambda ms: round(distinct / (ms * 1e-3) / 1e12, 3)
        line = json.dumps({"op": "residuals", "n": n, "dtype": args.dtype, "k": k, "residuals_ms": [round(t, 4) for t in res],
                           "observables_x_k_ms": [round(t, 4) for t in obs], "ratio_observables_over_residuals": [round(o / r, 3) for o, r in zip(obs, res)],
                           "residuals_tbps_distinct_reads": [tbps(t) for t in res], "observables_tbps_distinct_reads": [tbps(t) for t in obs],
                           "rayleigh_ms": [round(t, 4) for t in timed(lambda: ctx.residuals(k), 3)], "env": env})
        print(line)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        sys.exit(0)
    # a rotation close to the identity, so that repeating it keeps the states O(1)
    coef = np.eye(k) + 0.01 * np.random.default_rng(0).standard_normal((k, k))
    esz = 8 if args.dtype == "f64" else 4
    array_bytes = float(n) ** 3 * esz
    obs = timed(ctx.observables, 10)
    copy_gbps = ctx.copy_bandwidth()
    for name, fn, passes in (("ritz_matrices", lambda: ctx.ritz_matrices(k), k * (k + 2)), ("rotate_states", lambda: ctx.rotate_states(coef), 2 * k)):
        ts = timed(fn, 10)
        med = statistics.median(ts)
        gbps = passes * array_bytes / (med * 1e-3) / 1e9
        print(json.dumps({"op": name, "n": n, "dtype": args.dtype, "k": k, "ms_median_incl_host_sync": round(med, 4), "ms_min": round(min(ts), 4),
                          "array_passes": passes, "gbps": round(gbps, 1), "copy_gbps": round(copy_gbps, 1),
                          "fraction_of_copy": round(gbps / copy_gbps, 4), "observables_ms_median": round(statistics.median(obs), 4), "env": env}))
