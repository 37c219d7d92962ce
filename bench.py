#!/usr/bin/env python3
"""Benchmark of the grid::evolve hot path (BASELINE.json metric: grid-point
updates/sec on 512^3 fp64, achieved HBM GB/s vs peak).

    python bench.py --gpus N --steps K --warmup W

A "step" is ONE imaginary-time step (grid.rs:562-686, wnum = 0) of the whole
grid; potential and phi are generated in HBM (no host traffic in the timed
region).

N = 1: the 512^3 fp64 ThreePoint Coulomb grid of BASELINE configs[2], ground-state
evolve.  After the timed region the SAME kernel instance is held against the CPU
oracle bit for bit ("parity" in the result line; a mismatch is exit code 3), and
the state the timed steps produced is reproduced by the independent single-step
kernel (checksum of every cell's bits).

N > 1: BASELINE configs[3], the 1024^3 SimpleCornell grid, STRONG scaling -- z-slabs
of 1024/N planes per GPU, RCCL halo exchange behind the interior update.  Rank 0
then runs the same 1024^3 grid undecomposed on its own GPU for the same steps:
`single_gpu_ref` carries T1 (so T1 / (N * TN) needs no second run) and every slab's
checksum must equal the undecomposed run's over the same planes.
`--scaling weak` keeps 2^27 points per GPU instead: (1024, 1024, 128 N).

Launching: `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`
(one rank per GPU; RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment),
or bare `python bench.py --gpus N`: the parent then starts the N ranks itself as
child processes BEFORE anything touches a GPU, forwards rank 0's line and exits
non-zero if fewer than N devices or ranks materialise.

Prints ONE JSON line on rank 0 (contract in the task statement) with the extra
objects "roofline", "cpu_baseline" (N = 1), "parity", "comm" and "single_gpu_ref"
(N > 1).
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

# multi-process GPU work on this pool needs dmabuf IPC (RCCL's peer mappings fail with
# "hipIpcGetMemHandle: invalid argument" otherwise); must be in the environment before the HSA runtime loads
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
# the CPU baseline leg (N = 1): its OpenMP threads stay where they first touched their pages.  Read by the OpenMP runtime when
# it loads -- which may be torch's import, long before the oracle's -- so it is set here; WAFER_BENCH_OMP_BIND=0 leaves it alone.
if os.environ.get("WAFER_BENCH_OMP_BIND", "1") != "0":
    os.environ.setdefault("OMP_PROC_BIND", "spread")
    os.environ.setdefault("OMP_PLACES", "cores")

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0        # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling
BYTES_PER_UPDATE = {"f64": 32, "f32": 16, "f32fast": 16}  # phi, a, b in + phi' out
RC_PARITY = 3                 # exit code when the timed kernel's result differs from the oracle's


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32", "f32fast"])
    ap.add_argument("--grid", default=None, help="override: NX,NY,NZ (global work area)")
    ap.add_argument("--cd", type=int, default=1, help="central difference ext: 1/2/3")
    ap.add_argument("--potential", default=None, help="default: Coulomb at N = 1, SimpleCornell at N > 1")
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"],
                    help="N > 1: strong = 1024^3 split over the ranks (default); weak = 1024x1024x128 per rank")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=20.0, help="target CPU time of the oracle sample")
    ap.add_argument("--no-parity", action="store_true", help="skip the oracle / cross-kernel / undecomposed checks")
    ap.add_argument("--no-excited", action="store_true", help="N = 1: skip the informational excited-state step timings")
    ap.add_argument("--variant", type=int, default=-1, help="stencil kernel variant (-1 = default)")
    ap.add_argument("--preheat", type=int, default=300,
                    help="untimed set-up steps before the warm-up, to bring the clocks up from idle (the state is reset afterwards)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the state they left (phi's work cells: all of them, or a fixed seeded "
                         "sample of a larger grid) as DIR/*.npy, so that two builds can be compared output for output")
    return ap.parse_args(argv)


def physical_cores() -> int:
    """Wafer's own thread rule (main.rs:190-196): the rayon pool gets num_cpus::get_physical() -- bounded by what this
    process may really use (affinity mask, cgroup CPU quota: more threads than that only take turns).  A physical-core
    count that cannot be right (virtual machines report sockets, or 1) is ignored."""
    n = max(1, len(os.sched_getaffinity(0)))
    try:
        import psutil
        phys = psutil.cpu_count(logical=False)
        if phys and phys * 4 >= n:       # (SMT up to four ways; anything smaller is not a core count of this machine)
            n = int(min(n, phys))
    except Exception:
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = max(1, min(n, int(float(quota) / float(period))))
    except Exception:
        pass
    return n


# ---------------------------------------------------------------------------------------------
# launcher: bare `bench.py --gpus N` -> N rank processes, started before any GPU call
# ---------------------------------------------------------------------------------------------
def launch_ranks(args) -> int:
    n = args.gpus
    host_transport = os.environ.get("WAFER_BENCH_TRANSPORT", "rccl") == "host"
    import torch  # device_count() does not initialise the GPU; nothing else of torch.cuda is touched here
    ndev = torch.cuda.device_count()
    if ndev < n and not host_transport:
        print(f"bench.py: --gpus {n} but only {ndev} GPU(s) are visible; refusing to mislabel a smaller run",
              file=sys.stderr)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WAFER_BENCH_SELF_LAUNCHED="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, text=True))
    rc = 0
    pending = set(range(n))
    while pending and rc == 0:
        for r in sorted(pending):
            code = procs[r].poll()
            if code is not None:
                pending.discard(r)
                if code != 0:
                    rc = code
                    print(f"bench.py: rank {r} exited with code {code}", file=sys.stderr)
        if pending and rc == 0:
            time.sleep(0.2)
    if rc != 0:   # one rank failed: the others would wait in a collective for ever
        for r in pending:
            procs[r].terminate()
        for r in pending:
            try:
                procs[r].wait(timeout=30)
            except subprocess.TimeoutExpired:
                procs[r].kill()
    out = procs[0].stdout.read() if procs[0].stdout else ""
    lines = [ln for ln in out.splitlines() if ln.strip()]
    if rc == 0:
        try:
            res = json.loads(lines[-1])
            if res.get("n_gpus") != n or res.get("ranks") != n:
                print(f"bench.py: rank 0 reports n_gpus={res.get('n_gpus')} ranks={res.get('ranks')}, expected {n}",
                      file=sys.stderr)
                rc = 2
        except Exception as e:  # noqa: BLE001
            print(f"bench.py: no result line from rank 0 ({e!r})", file=sys.stderr)
            rc = 2
    if lines:
        print(lines[-1], flush=True)
    return rc


# ---------------------------------------------------------------------------------------------
# CPU legs (rank 0, N = 1): the oracle as the reported baseline and as the checker
# ---------------------------------------------------------------------------------------------
def cpu_baseline(shape, ext, potential, dn, dt, mass, sig, target_seconds):
    """The oracle (kind "port": a C restatement of Wafer's rayon path, same pass
    structure: stencil into work, copy back) timed on this host's cores on a
    bounded number of steps of the SAME grid.  Reported, not the target.

    As BASELINE.md section 3 specifies it: rebuilt -O3 -march=native -ffp-contract=off on this host (oracle/Makefile
    `native`; contraction off, so the bits stay the portable build's -- the caller checks them against the HIP engine),
    threads bound (OMP_PROC_BIND / OMP_PLACES, set at the top of this file), every array first touched by the static
    schedule that later streams it (the oracle's generators are the same `omp parallel for schedule(static)` loops
    over x as its evolve).  The thread count is the fastest of {2 x usable, usable, usable / 2} on one step each, `usable`
    = physical cores within the affinity mask and the cgroup CPU quota (the round-4 line ran 128 threads on a box whose
    quota was 16 CPUs: 0.64 G updates/s where 16-32 threads reach 1.6-2.0, tools/cpu_baseline_probe.py).

    Returns (record, phi after `total_steps` steps, total_steps) so that the same
    CPU work also serves as the parity reference."""
    from oracle import wafer_oracle as wo
    native = wo.use_native()
    cores = physical_cores()
    cfg = wo.Config(*shape, ext=ext, potential=potential, dn=dn, dt=dt, mass=mass, sig=sig)
    wo.set_threads(cores)
    v = wo.potential_generate(cfg)
    a, b = wo.ab(cfg, v)
    del v
    phi = wo.initial_condition(cfg, "Boolean")
    wo.evolve(cfg, 0, a, b, phi, [], 1)          # first touch of `work`, page faults, thread start-up
    done = 1
    tried = {}
    # (under a cgroup CPU quota smaller than the affinity mask, twice the quota's worth of threads can still win: they take
    #  turns, but each finds its pages where it left them)
    over = min(2 * cores, len(os.sched_getaffinity(0)))
    for t in sorted({over, cores, max(1, cores // 2)}, reverse=True):
        wo.set_threads(t)
        t0 = time.perf_counter()
        wo.evolve(cfg, 0, a, b, phi, [], 1)
        tried[t] = time.perf_counter() - t0
        done += 1
    threads = min(tried, key=tried.get)
    wo.set_threads(threads)
    t1 = tried[threads]
    steps = int(max(2, min(400, target_seconds / max(t1, 1e-6))))
    t0 = time.perf_counter()
    wo.evolve(cfg, 0, a, b, phi, [], steps)
    dt_s = time.perf_counter() - t0
    pts = shape[0] * shape[1] * shape[2]
    rate = pts * steps / dt_s
    try:
        copy_gbps = wo.host_copy_gbps(1 << 30, 3)
        placement = wo.thread_placement()
    except Exception:  # noqa: BLE001 -- informational
        copy_gbps, placement = None, None
    rec = {
        "value": rate,
        "unit": "updates/s",
        "cores": threads,
        "kind": "port",
        "sample": f"{steps} steps of the same {shape[0]}x{shape[1]}x{shape[2]} fp64 {potential} grid "
                  f"(oracle/wafer_oracle.c wo_evolve, OpenMP, {dt_s:.1f} s)",
        "build": "-O3 -march=native -ffp-contract=off (built on this host)" if native else "-O3 -march=x86-64-v2 -ffp-contract=off (portable build: the native one failed)",
        # the reference's pass structure moves 48 B per update: stencil pass phi, a, b in + work out, copy-back work in + phi out
        "effective_GBps": rate * 48 / 1e9,
        "host_copy_GBps": copy_gbps,   # an OpenMP copy between two first-touched 1 GiB buffers on the same threads (read + written)
        "usable_cores": cores,
        "seconds_per_step_by_threads": {str(k): round(v_, 4) for k, v_ in tried.items()},
        "thread_placement": placement,
    }
    return rec, phi, done + steps


def max_ulp(got, want) -> int:
    """largest distance in units in the last place between two float64 arrays (0 = the same bits,
    up to the sign of zero)"""
    import numpy as np
    worst = 0
    g, w = got.reshape(-1), want.reshape(-1)
    for i in range(0, g.size, 1 << 24):   # bounded temporaries
        a = g[i:i + (1 << 24)].view(np.int64).copy()
        b = w[i:i + (1 << 24)].view(np.int64).copy()
        a[a < 0] = np.int64(-2**63) - a[a < 0]   # sign-magnitude -> two's complement order
        b[b < 0] = np.int64(-2**63) - b[b < 0]
        d = np.abs(a - b)
        nan = np.isnan(g[i:i + (1 << 24)]) | np.isnan(w[i:i + (1 << 24)])
        if nan.any():
            return 2**62
        worst = max(worst, int(d.max(initial=0)))
    return worst


def boolean_norm2(shape, ext) -> float:
    """sum phi^2 over the work area of the Boolean initial condition (config.rs:676-683: 1 where all
    three PADDED indices are odd): the product over the axes of the number of odd indices in [ext, ext + n)"""
    out = 1.0
    for n in shape:
        out *= len([i for i in range(ext, ext + n) if i % 2 == 1])
    return out


def pmc_traffic(kernel_instance: str):
    """HBM bytes per launch from the committed rocprofv3 --pmc summary (a STATIC figure: counters cannot be read inside a
    timed run) -- only from the entry of EXACTLY this instantiation ("wafer_k_step3_fused<double, double, true, 0, true, 1>"
    against the profiler's "void wafer_k_step3_fused<...>(arguments)"): another instantiation's bytes (peer stores, marching
    down, fp32) describe another kernel.  -> (bytes or None, the matched key or None, stale: the kernel sources have changed
    since the figure was measured -- tools/pmc_summary.py stores their hash, wafer_amd/provenance.py -- or None if unknown)"""
    if "<" not in kernel_instance:
        return None, None, None
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        with open(path) as f:
            d = json.load(f)
        from wafer_amd.provenance import kernel_sources_sha16
        measured_on = d.get("kernel_sources_sha16")
        for k, v in d.get("kernels", {}).items():
            if "from" in v:   # entries tagged "from" are earlier builds / variants kept for the record
                continue
            if k.startswith("void " + kernel_instance + "(") or k == kernel_instance:
                on = v.get("kernel_sources_sha16", measured_on)
                return v.get("hbm_bytes_per_launch"), k, (None if on is None else on != kernel_sources_sha16())
    except Exception:
        pass
    return None, None, None


DUMP_MAX_CELLS = 1 << 21     # 16 MB of float64: a grid with more work cells is sampled
DUMP_SEED = 20240601


def dump_outputs(out_dir, ctx, shape, z_begin, z_count, dist, rank):
    """What the timed steps left for a caller of wafer_evolve: phi's work cells (the frame is zero by construction), as float64.
    A grid of at most DUMP_MAX_CELLS cells is written whole (phi.npy, shape NX x NY x NZ); a larger one as the cells at a fixed,
    seeded sample of global positions (phi_sample.npy, ascending C-order index), the same positions for every run of the same
    grid and for every slab decomposition of it.  Collective over the ranks; rank 0 writes."""
    import numpy as np
    owned = ctx.download_phi_owned()                 # (nx, ny, z_count): this rank's planes, or the whole grid
    zb = z_begin if z_count else 0
    total = shape[0] * shape[1] * shape[2]
    if total <= DUMP_MAX_CELLS:
        name, idx = "phi", None
    else:
        name = "phi_sample"
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(total, size=DUMP_MAX_CELLS, replace=False))
    if dist is None:
        out = owned if idx is None else owned.reshape(-1)[idx]
    else:
        if idx is None:
            idx = np.arange(total)
        i, j, k = np.unravel_index(idx, shape)
        mine = np.nonzero((k >= zb) & (k < zb + owned.shape[2]))[0]
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, (mine, owned[i[mine], j[mine], k[mine] - zb]))
        out = np.full(idx.shape, np.nan)
        for pos, vals in parts:
            out[pos] = vals
        if name == "phi":
            out = out.reshape(shape)
    del owned
    if rank != 0:
        return None
    os.makedirs(out_dir, exist_ok=True)
    out = np.ascontiguousarray(out, dtype=np.float64)
    np.save(os.path.join(out_dir, name + ".npy"), out)
    return {"dir": out_dir, "files": {name + ".npy": {"shape": list(out.shape), "dtype": "float64"}},
            "what": "phi's work cells after the timed steps" + ("" if name == "phi" else
                    f" at {DUMP_MAX_CELLS} positions drawn without replacement (numpy default_rng({DUMP_SEED})) from the "
                    "C-order flat index of the NX x NY x NZ work area, ascending")}


# ---------------------------------------------------------------------------------------------
# one rank
# ---------------------------------------------------------------------------------------------
def run_rank(args) -> int:
    # RCCL caches its parameters at first use, which is torch's own communicator: the channel limit the
    # slab transport wants (wafer_rccl_hooks.h) has to be in the environment before that
    os.environ.setdefault("NCCL_MAX_P2P_NCHANNELS", "8")
    # Every rank of this benchmark reaches every wafer_evolve behind a barrier, so a workgroup or gate kernel that waits for a
    # neighbour's planes for seconds is waiting for something that will not come: 5 s (gate kernels: 20 s) instead of the library's
    # 20 s / 80 s, which are sized for hosts that write files between calls.  A schedule whose wait gives up in the set-up trial is
    # dropped on every rank; the shorter bound keeps a fabric that cannot serve one of them from eating the run's time budget.
    os.environ.setdefault("WAFER_HV_WAIT_MS", "5000")
    # stdout carries exactly ONE line, the JSON result: native libraries that write to the C stdout
    # (RCCL prints a version banner there, flushed at exit) are sent to stderr instead
    sys.stdout.flush()
    result_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n_gpus = args.gpus
    if world > 1:
        # A rank that waits for a peer inside RCCL (communicator set-up, a send without its receive) waits for ever; the
        # engine's own waits are bounded (WAFER_ERR_COMM) but the library's are not.  The transport has never run between
        # two GPUs (tools/first_contact_8gpu.md), so a multi-rank run carries a deadline: say where it stands and leave with
        # a code of its own instead of holding the node until somebody else's timeout.
        import threading
        import faulthandler
        deadline = float(os.environ.get("WAFER_BENCH_DEADLINE_S", "900"))

        def give_up():
            print(f"bench.py: rank {rank}: no result after {deadline:.0f} s (WAFER_BENCH_DEADLINE_S); stacks follow",
                  file=sys.stderr, flush=True)
            faulthandler.dump_traceback(file=sys.stderr, all_threads=True)
            os._exit(5)
        watchdog = threading.Timer(deadline, give_up)
        watchdog.daemon = True
        watchdog.start()

    import numpy as np
    import torch
    import wafer_amd

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the engine has no CPU path")
    # WAFER_BENCH_TRANSPORT=host: halo planes staged through host memory over gloo, ranks folded
    # onto the GPUs present -- only for exercising the N > 1 leg on a one-GPU box
    # (tests/test_gpu_multiprocess.py); the default is RCCL, one GPU per rank, the hooks served by
    # RCCL's C API directly (WAFER_TRANSPORT=torch: through torch.distributed)
    host_transport = os.environ.get("WAFER_BENCH_TRANSPORT", "rccl") == "host"
    ndev = torch.cuda.device_count()
    # a launcher that narrows each rank's view to its own GPU (ROCR_/HIP_VISIBLE_DEVICES per rank) leaves
    # one visible device with index 0; the host-staged test transport folds ranks onto the GPUs present
    if host_transport or (ndev == 1 and world > 1 and os.environ.get("HIP_VISIBLE_DEVICES", os.environ.get("ROCR_VISIBLE_DEVICES"))):
        local_rank %= max(1, ndev)
    if local_rank >= ndev:
        raise SystemExit(f"rank {rank}: LOCAL_RANK {local_rank} but {ndev} GPU(s) visible: one GPU per rank is required")
    torch.cuda.set_device(local_rank)

    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if host_transport:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        if dist.get_world_size() != n_gpus:
            raise SystemExit(f"--gpus {n_gpus} but the process group has {dist.get_world_size()} ranks")
    coll_dev = "cpu" if host_transport else f"cuda:{local_rank}"

    ext = args.cd
    if args.grid:
        shape = tuple(int(s) for s in args.grid.split(","))
    elif n_gpus == 1:
        shape = (512, 512, 512)
    elif args.scaling == "strong":
        shape = (1024, 1024, 1024)
    else:
        shape = (1024, 1024, 128 * n_gpus)
    if n_gpus == 1:
        dn, dt, mass = 0.05, 5e-4, 1.0
        potential = args.potential or "Coulomb"
    else:
        dn, dt, mass = 0.02, 8e-5, 2.35           # config #4: SimpleCornell, sig 0.223
        potential = args.potential or "SimpleCornell"
    sig = 0.223

    nz = shape[2]
    z_begin, z_count = 0, 0
    if world > 1:
        from wafer_amd import slab
        z_begin, z_count = slab.partition(nz, world, rank)

    def make_params(zb, zc, halo):
        return wafer_amd.Params(shape[0], shape[1], shape[2], dn=dn, dt=dt, mass=mass, sig=sig,
                                central_difference=ext, dtype=args.dtype, max_states=1, device=local_rank,
                                z_begin=zb, z_count=zc, halo_depth=halo)

    # ghost planes: 3*ext (ThreePoint, every dtype: three fused steps per exchange; otherwise 2*ext: two); twice that where the
    # slabs are thick enough, so that the set-up trial can also time one exchange per TWO fused passes
    # (wafer_set_halo_cycle)
    per_pass = 3 * ext if ext == 1 else 2 * ext
    if world > 1 and os.environ.get("WAFER_BENCH_PEERS", "1") == "force":
        os.environ.setdefault("WAFER_PEER_SAME_DEVICE", "1")   # ranks folded onto one GPU on purpose (read by wafer_ctx_create)
    deep = world > 1 and min(slab.partition(nz, world, r)[1] for r in range(world)) >= 4 * per_pass
    ctx = wafer_amd.Context(make_params(z_begin, z_count, (2 * per_pass if deep else per_pass) if world > 1 else 0))
    if args.variant >= 0:
        ctx.set_stencil_variant(args.variant)
    comm, transport_name = None, None
    if world > 1:
        comm, transport_name = slab.make_slab_comm(ctx, rank, world, torch.device("cuda", local_rank),
                                                   "host" if host_transport else None)
        # A scaling record must never be a fallback's number by accident: the native RCCL hooks are what this benchmark
        # measures.  If they could not be installed (make_slab_comm then agrees on the torch.distributed hooks on every
        # rank), say so and stop, unless the caller asked for that transport by name.
        if not host_transport and "native" not in transport_name and os.environ.get("WAFER_TRANSPORT", "native") == "native":
            print(f"bench.py: rank {rank}: the native RCCL hooks are not in use (got '{transport_name}'); "
                  "set WAFER_TRANSPORT=torch to measure the torch.distributed hooks on purpose", file=sys.stderr)
            return 4
        comm.warm_up()   # RCCL channel set-up is not part of any step
        # the scalar all-reduce (excited-state steps, observables): ncclAllReduce or the device-side mailboxes, by measurement
        allreduce_choice = None
        if hasattr(comm, "pick_allreduce") and os.environ.get("WAFER_MAILBOX", "") == "":
            try:
                allreduce_choice = comm.pick_allreduce()
            except Exception as e:  # noqa: BLE001
                allreduce_choice = {"error": repr(e)}
        # peer stores (wafer_set_overlap mode 3) and peer copies (mode 4): every rank maps its z-neighbours' buffers through HIP IPC; all
        # ranks or none.  Mode 3 is the ThreePoint three-step pass on slabs of six planes or more; mode 4 is a transport and serves every pass.
        peers_ok = copies_ok = False
        # (Not by default with the host-staged test transport: ranks folded onto ONE GPU poll for each other's stores from
        #  workgroups that hold the CUs the other rank's kernel needs.  WAFER_BENCH_PEERS=force connects them there as well -- HIP
        #  IPC between processes on one device -- so that a one-GPU box executes every line the first real multi-GPU run will; the
        #  tests keep the grids at a tile per CU per rank or less, and a schedule whose bounded waits give up is dropped below.)
        want_peers = os.environ.get("WAFER_BENCH_PEERS", "1")
        if want_peers != "0" and (not host_transport or want_peers == "force"):
            try:
                copies_ok = slab.connect_peers(ctx, rank, world)
                peers_ok = copies_ok and ext == 1 and min(slab.partition(nz, world, r)[1] for r in range(world)) >= 6
            except Exception as e:  # noqa: BLE001
                print(f"bench.py: rank {rank}: peer connection failed: {e!r}", file=sys.stderr, flush=True)
    ctx.set_potential(potential)
    ctx.set_initial_condition("Boolean")   # deterministic, "good for benchmarks" (config.rs:168)
    ctx.synchronize()

    def barrier():
        # this rank's queued work first, then every rank's, then whatever the barrier itself queued
        ctx.synchronize()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    # the initial condition against its closed form (exact: a sum of ones)
    ic_check = None
    if not args.no_parity:
        n2 = ctx.norm2()   # all-reduced over the slabs
        ic_check = {"norm2": n2, "closed_form": boolean_norm2(shape, ext)}
        if n2 != ic_check["closed_form"]:
            print(f"bench.py: initial condition norm2 {n2} != closed form {ic_check['closed_form']}", file=sys.stderr)
            return RC_PARITY

    # the box itself next to the 8 TB/s datasheet peak: the bandwidth its own
    # properties imply and what a 16 B-per-lane device copy reaches on the same buffers.  Measured
    # during set-up, before the warm-up steps (it also brings the clocks up from idle).
    try:
        di = ctx.device_info()
        mclk_khz, width = di["memory_clock_khz"], di["memory_bus_bits"]
        device_info = {
            "name": di["name"], "arch": di["arch"], "compute_units": di["compute_units"],
            "hbm_GB": round(di["total_bytes"] / 2**30, 1),
            "memory_clock_MHz": mclk_khz / 1e3, "memory_bus_bits": width,
            # HBM3E moves 4 bits per pin per reported memory clock (2 GHz -> 8 Gb/s/pin):
            # 8192 pins x 8 Gb/s = 8.19 TB/s, the datasheet's "8 TB/s"
            "hbm_GBps_from_props": 4.0 * mclk_khz * 1e3 * width / 8 / 1e9,
            # read + written bytes of a device-to-device copy of one array (wafer_k_copy16)
            "measured_copy_GBps": round(ctx.copy_bandwidth(100, 4, 1), 1),   # the best setting of tools/copy_sweep.py (profiles/r02_copy_sweep.jsonl)
        }
    except Exception as e:  # informational
        device_info = {"error": repr(e)}
    ctx.set_initial_condition("Boolean")   # the copy used phi's second buffer as scratch

    # N > 1: how the halo exchange is scheduled (wafer_set_overlap).  Mode 4: mode 2's single launch with every exchange a device copy
    # into the neighbour's ghost planes (the copy engines between GPUs: no exchange kernel on any CU).  Mode 3: mode 2's single launch with the boundary workgroups
    # storing straight into the neighbours' ghost planes (HIP IPC / xGMI peer stores: no exchange kernels at all).  Mode 1: boundary planes and their exchange on a
    # second stream beside the interior update (three launches per pass); mode 2: ONE launch per three-step pass, the slab
    # as two halves marched outwards, each half's exchange released by its completion counter; mode 0: the exchange
    # follows the whole slab's update.  Which is fastest depends on the fabric, which this code has never seen: all are
    # timed over a few untimed set-up steps (and one exchange per TWO passes where the slabs are thick enough), and
    # every rank takes the schedule that is fastest for the slowest rank (the default, 2, unless another wins by more
    # than 2 %).
    overlap_choice = None
    DEFAULT_MODE = (2, 1)
    if dist is not None and os.environ.get("WAFER_OVERLAP", "") == "" and args.steps >= 8:
        # Peer stores have never crossed a link (tools/first_contact_8gpu.md): before the schedule is timed, let alone trusted with the
        # timed steps, it has to reproduce the bits of an exchange through the halo hook on every rank -- else it is dropped here
        # instead of surfacing as a parity failure of the whole run
        peer_check = copy_check = None
        if peers_ok:
            peers_ok = slab.overlap_modes_agree(ctx, rank, world, 3, 0, steps=15, device=coll_dev)
            peer_check = {"against": "overlap mode 0 (exchange through the halo hook), 15 steps, every rank's checksum", "identical": peers_ok}
            if not peers_ok and rank == 0:
                print("bench.py: peer stores (overlap mode 3) do not reproduce the exchange's bits on this fabric: dropped", file=sys.stderr, flush=True)
        # ... and so have the peer copies (mode 4: hipMemcpyAsync into the neighbour's ghost planes, a credit / arrival rendezvous
        # of one-wave kernels instead of send / recv): the same check, the same consequence
        copy_modes = []
        if copies_ok:
            # mode 4: under the single launch (its workgroups read the copied planes behind a flag wait, while they run); modes 5 / 6:
            # under mode 1's / mode 0's launches (every reader starts after the copy) -- each has to pass on its own
            copy_check = {"against": "overlap mode 0 (exchange through the halo hook), 15 steps, every rank's checksum"}
            for m in (4, 5, 6):
                good = slab.overlap_modes_agree(ctx, rank, world, m, 0, steps=15, device=coll_dev)
                copy_check["identical" if m == 4 else f"identical_mode_{m}"] = good
                if good:
                    copy_modes.append((m, 1))
                elif rank == 0:
                    print(f"bench.py: peer copies (overlap mode {m}) do not reproduce the exchange's bits on this fabric: dropped", file=sys.stderr, flush=True)
            copies_ok = bool(copy_modes)
        # (slab.time_overlap_schedules: the same collective calls on every rank whatever happens on it; a schedule that fails
        #  anywhere is dropped everywhere)
        trial = slab.time_overlap_schedules(
            ctx, ([(3, 1)] if peers_ok else []) + copy_modes + [(2, 1), (1, 1), (0, 1)] + ([(1, 2), (0, 2)] + [(m, 2) for m, _ in copy_modes if m in (5, 6)] if deep else []), rank, device=coll_dev,
            log=lambda msg: print("bench.py: " + msg, file=sys.stderr, flush=True), device_sync=torch.cuda.synchronize)
        if not trial:
            print(f"bench.py: rank {rank}: every halo schedule failed in the set-up trial", file=sys.stderr)
            return 4
        best = min(trial, key=lambda k: trial[k] * (1.0 if k == DEFAULT_MODE else 1.02))
        ctx.set_overlap(best[0])
        ctx.set_halo_cycle(best[1])
        names = {6: "6_no_overlap_peer_copies", 5: "5_boundary_first_peer_copies", 4: "4_single_launch_peer_copies", 3: "3_single_launch_peer_stores", 2: "2_single_launch_two_halves", 1: "1_boundary_first_three_launches", 0: "0_no_overlap"}
        overlap_choice = {"mode": best[0], "fused_passes_per_exchange": best[1],
                          "ms_per_step": {names[m] + ("" if cy == 1 else f"_exchange_every_{cy}_passes"): v for (m, cy), v in trial.items()},
                          **({"peer_store_check": peer_check} if peer_check else {}), **({"peer_copy_check": copy_check} if copy_check else {})}
        ctx.set_initial_condition("Boolean")
    elif dist is not None:
        mode = int(os.environ.get("WAFER_OVERLAP", "") or DEFAULT_MODE[0])
        ctx.set_overlap(mode)
        ctx.set_halo_cycle(1)
        overlap_choice = {"mode": mode, "fused_passes_per_exchange": 1, "ms_per_step": None}

    # Set-up, untimed: the device's clocks follow the load, and the few milliseconds of a short run (the
    # driver's --steps 20 --warmup 5) would otherwise be spent ramping them up -- the same 20 steps are 7 %
    # slower by the engine's own HIP events than inside a long run.  A few hundred steps bring them to
    # their sustained state; the wavefunction is then reset, so the W warm-up and K timed steps start from
    # the same state as without this.
    if args.preheat > 0:
        ctx.evolve(0, args.preheat)
        ctx.set_initial_condition("Boolean")
    # ---- the timed region ------------------------------------------------------------------------
    if args.warmup > 0:
        ctx.evolve(0, args.warmup)
    barrier()
    t0 = time.perf_counter()
    ctx.evolve(0, args.steps)
    barrier()
    elapsed = time.perf_counter() - t0
    kernel_ms, ksteps = ctx.last_evolve_ms()     # HIP events on the engine's own stream
    pts_rank = shape[0] * shape[1] * (z_count if z_count else shape[2])
    ranks_seen = 1
    if dist is not None:
        t = torch.tensor([elapsed, kernel_ms, float(pts_rank)], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, kernel_ms, pts_rank = float(t[0]), float(t[1]), int(t[2])   # the slowest rank, the largest slab
        one = torch.ones(1, dtype=torch.float64, device=coll_dev)
        dist.all_reduce(one, op=dist.ReduceOp.SUM)
        ranks_seen = int(one[0])
    total_steps = args.warmup + args.steps    # what phi has been through since the initial condition
    dumped = dump_outputs(args.dump_outputs, ctx, shape, z_begin, z_count, dist, rank) if args.dump_outputs else None

    pts_total = shape[0] * shape[1] * shape[2]
    value = pts_total * args.steps / elapsed
    bpu = BYTES_PER_UPDATE[args.dtype]
    spl = ctx.steps_per_launch()                  # the fused kernel advances two steps per launch
    launch_s = (kernel_ms / 1e3) / max(1, ksteps) * spl
    achieved = pts_rank * bpu * spl / launch_s / 1e9
    kname = ctx.stencil_kernel_name()
    kinst = ctx.stencil_kernel_instance()         # the instantiation the timed passes launched, as a profiler prints it
    # (the committed counter figure belongs to one kernel on one workload: the default grid and potential only)
    traffic, traffic_key, traffic_stale = pmc_traffic(kinst) if (n_gpus == 1 and not args.grid and not args.potential) else (None, None, None)

    comm_info = None
    if comm is not None:
        comm_info = {"transport": transport_name}
        if hasattr(comm, "info"):
            comm_info.update(comm.info())   # ncclCommCount etc. of the communicator the hooks use
        comm_info["process_group_ranks"] = dist.get_world_size()
        comm_info["halo_overlap_mode"] = overlap_choice["mode"] if overlap_choice else None
        comm_info["scalar_allreduce"] = allreduce_choice

    result = {
        "metric": "grid_point_updates_per_sec",
        "value": value,
        "unit": "updates/s",
        "n_gpus": n_gpus,
        "ranks": ranks_seen,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": args.scaling if n_gpus > 1 else "strong",
        "vs_baseline": None,   # the reference publishes no number for this metric
        "dtype": args.dtype,
        "data": "synthetic",
        "config": {
            "workload": f"{shape[0]}x{shape[1]}x{shape[2]} {potential} potential, "
                        f"{ {1: 'ThreePoint', 2: 'FivePoint', 3: 'SevenPoint'}[ext]} stencil, ground-state "
                        f"imaginary-time evolve (grid.rs:544-687), Boolean initial condition"
                        + ("" if n_gpus == 1 else f", z-slabs of {shape[2] // n_gpus} planes per GPU, "
                           + f"halo exchange: {transport_name}"),
            "grid": list(shape),
            "points_per_gpu": pts_rank,
            "parallelism": f"zslab{n_gpus}",
            "kernel": kname,
            "preheat_steps": args.preheat,   # untimed set-up steps before the warm-up (clock ramp), state reset after them
            **({"halo_overlap": overlap_choice} if overlap_choice else {}),
        },
        "roofline": {
            "bound": "hbm",
            "achieved": achieved,
            "peak": HBM_PEAK_GBPS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBPS,
            "traffic": traffic,
            "traffic_source": ("profiles/pmc_traffic.json (static: rocprofv3 --pmc of this kernel on this workload, "
                               "not re-measured in this run); entry: " + traffic_key) if traffic else None,
            # True: the kernel sources have changed since that figure was measured (wafer_amd/provenance.py hashes them,
            # tools/pmc_summary.py stores the hash with the figures); None: the committed file carries no hash
            "traffic_stale": traffic_stale if traffic else None,
            "kernel": kinst,
            "avg_launch_ms": launch_s * 1e3,
            "steps_per_launch": spl,
            "algorithmic_bytes_per_launch": pts_rank * bpu * spl,
            # what the kernel really moved per second (static PMC traffic / this run's launch time) ...
            "traffic_GBps": (traffic / launch_s / 1e9) if traffic else None,
            # ... as a fraction of the 8 TB/s peak: the PHYSICAL fraction.  `frac` above prices SURVEY 8(d)'s 32 B per update
            # whatever the kernel moved (temporal blocking makes it exceed 1); this one cannot
            "frac_traffic": (traffic / launch_s / 1e9 / HBM_PEAK_GBPS) if traffic else None,
            # ... and of what a plain 16 B-per-lane device copy reaches on this box in this run (device.measured_copy_GBps)
            "copy_ceiling_frac": (traffic / launch_s / 1e9 / device_info["measured_copy_GBps"])
                                 if (traffic and device_info.get("measured_copy_GBps")) else None,
        },
        "device": device_info,
    }
    if comm_info:
        result["comm"] = comm_info
    if dumped:
        result["dump_outputs"] = dumped
    rc = 0

    # ---- N > 1: the same grid undecomposed on rank 0's GPU: T1, and the slabs' bits -----------------
    if dist is not None and not args.no_parity:
        mine = ctx.checksum(z_begin, z_count)
        sums = [None] * world
        dist.all_gather_object(sums, (z_begin, z_count, mine))
        if rank == 0:
            ref = wafer_amd.Context(make_params(0, 0, 0))
            if args.variant >= 0:
                ref.set_stencil_variant(args.variant)
            ref.set_potential(potential)
            ref.set_initial_condition("Boolean")
            if args.warmup > 0:
                ref.evolve(0, args.warmup)
            ref.synchronize()
            t_ = time.perf_counter()
            ref.evolve(0, args.steps)
            ref.synchronize()
            ref_elapsed = time.perf_counter() - t_
            ref_kernel_ms, ref_ksteps = ref.last_evolve_ms()
            bad = [(zb, zc) for zb, zc, s in sums if ref.checksum(zb, zc) != s]
            ref_kname = ref.stencil_kernel_name()
            ref.close()
            result["single_gpu_ref"] = {
                "grid": list(shape), "ms_per_step": ref_elapsed / args.steps * 1e3,
                "kernel_ms_per_step": ref_kernel_ms / max(1, ref_ksteps), "value": pts_total * args.steps / ref_elapsed,
                "kernel": ref_kname, "steps": args.steps, "warmup": args.warmup,
                "note": "the same grid, potential and steps on rank 0's GPU alone, after the timed region",
            }
            result["single_gpu_ref_ms_per_step"] = ref_elapsed / args.steps * 1e3
            result["parity"] = {
                "kind": "every slab's checksum (a hash of each cell's bits and global index, summed mod 2^64) against the "
                        "undecomposed run's over the same planes",
                "steps": total_steps, "slabs": world, "identical": not bad, "differing_slabs": bad,
                "initial_condition": ic_check,
            }
            if bad:
                rc = RC_PARITY
        flag = torch.tensor([float(rc)], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        rc = int(flag[0])

    # ---- N = 1: the oracle beside it (baseline), and as the checker of the timed kernel instance --------
    if dist is None and rank == 0:
        phi_cpu, n_cpu = None, 0
        if not args.no_cpu_baseline:
            try:
                result["cpu_baseline"], phi_cpu, n_cpu = cpu_baseline(shape, ext, potential, dn, dt, mass, sig, args.cpu_seconds)
            except Exception as e:  # the baseline is reported, never required
                result["cpu_baseline"] = {"value": None, "unit": "updates/s", "cores": physical_cores(),
                                          "kind": "port", "sample": f"failed: {e!r}"}
        if not args.no_parity:
            parity = {"initial_condition": ic_check}
            timed_sum = ctx.checksum()
            if phi_cpu is None:   # no baseline leg: a short oracle run of its own
                from oracle import wafer_oracle as wo
                wo.set_threads(physical_cores())
                cfg = wo.Config(*shape, ext=ext, potential=potential, dn=dn, dt=dt, mass=mass, sig=sig)
                v = wo.potential_generate(cfg)
                a_, b_ = wo.ab(cfg, v)
                del v
                phi_cpu, n_cpu = wo.initial_condition(cfg, "Boolean"), 3
                wo.evolve(cfg, 0, a_, b_, phi_cpu, [], n_cpu)
                del a_, b_
            # (1) the timed kernel instance -- same context, same variant, same launch geometry -- against the
            #     oracle from the same start, cell by cell
            ctx.set_initial_condition("Boolean")
            ctx.evolve(0, n_cpu)
            got = ctx.download_phi()
            if args.dtype == "f64":
                parity.update({"against": "oracle/wafer_oracle.c (CPU restatement of grid.rs:544-687)",
                               "steps": n_cpu, "max_ulp": max_ulp(got, phi_cpu)})
                if parity["max_ulp"] != 0:
                    rc = RC_PARITY
            else:   # fp32 storage: not a bit-for-bit path; the largest deviation is reported
                parity.update({"against": "oracle/wafer_oracle.c (fp64)", "steps": n_cpu,
                               "max_abs_diff": float(np.max(np.abs(got - phi_cpu)))})
            del got, phi_cpu
            # (2) the state the TIMED steps left behind, reproduced by the independent single-step kernel
            #     (another code path, itself bit-exact against the oracle in tests/): same bits expected
            if kname != "wafer_k_step_lds" and args.dtype != "f32fast":
                ctx.set_stencil_variant(1)
                ctx.set_initial_condition("Boolean")
                ctx.evolve(0, total_steps)
                parity["timed_state_reproduced_by_single_step_kernel"] = {
                    "steps": total_steps, "identical": ctx.checksum() == timed_sum}
                if not parity["timed_state_reproduced_by_single_step_kernel"]["identical"]:
                    rc = RC_PARITY
            result["parity"] = parity
        # "kernel time via hipEvents; also end-to-end including the per-block observables": three blocks of
        # the solve loop's body (grid.rs:126-221: observables, normalise, then screen_update = 1000 steps), wall clock
        if not args.no_parity:
            try:
                ctx.set_stencil_variant(args.variant)
                ctx.set_initial_condition("Boolean")
                ctx.synchronize()
                t_ = time.perf_counter()
                for _ in range(3):
                    o_ = ctx.observables()
                    ctx.normalise(o_["norm2"])
                    ctx.evolve(0, 1000)
                ctx.synchronize()
                result["end_to_end"] = {"ms_per_step": (time.perf_counter() - t_) / 3000 * 1e3, "blocks": 3, "screen_update": 1000,
                                        "note": "observables + normalise + 1000 steps per block (the body of grid.rs:126-221), wall clock"}
            except Exception as e:
                result["end_to_end"] = {"error": repr(e)}
        # (after everything the contract asks for) the excited-state step -- where a real run of BASELINE config #3
        # spends nine steps in ten: normalise + project on load, step, sum phi'^2 and the k raw overlaps in ONE pass
        # (grid.rs:674-681 takes 2 + 2k) -- against k = 1..3 stored states on the same grid, priced at SURVEY.md 8(d)'s
        # 80 / 112 / 144 B per update (the maximally fused multi-pass form).  The stored states are the three lowest
        # modes of the empty box (deterministic, exactly orthonormal), and the block proves itself: the same kernels,
        # from the same start, against the oracle over two k = 3 steps, every cell ("excited_parity"; > 1e-13 is exit
        # code 3, like the ground-state check above).
        if args.dtype == "f64" and not args.no_excited:
            try:
                n0, n1, n2_ = shape
                e = ext

                def sine(n, m):
                    return np.sin(np.pi * m * np.arange(1, n + 1) / (n + 1)) * np.sqrt(2.0 / (n + 1))

                def mode(mx, my, mz):
                    out = np.zeros((n0 + 2 * e, n1 + 2 * e, n2_ + 2 * e))
                    out[e:-e, e:-e, e:-e] = sine(n0, mx)[:, None, None] * sine(n1, my)[None, :, None] * sine(n2_, mz)[None, None, :]
                    return out
                lowers = [mode(1, 1, 1), mode(2, 1, 1), mode(1, 1, 2)]
                ex = wafer_amd.Context(wafer_amd.Params(shape[0], shape[1], shape[2], dn=dn, dt=dt, mass=mass, sig=sig,
                                                        central_difference=ext, dtype=args.dtype, max_states=3, device=local_rank))
                ex.set_potential(potential)
                for i, l in enumerate(lowers):
                    ex.load_state(i, l)
                phi0 = mode(1, 2, 1) + 0.3 * lowers[0] - 0.2 * lowers[2]
                phi0[e:-e:2, e:-e:2, e:-e:2] += 1e-3     # (a rough component, as the Boolean grid is)
                rec = {}
                if not args.no_parity:
                    from oracle import wafer_oracle as wo
                    wo.set_threads(physical_cores())
                    cfg = wo.Config(*shape, ext=ext, potential=potential, dn=dn, dt=dt, mass=mass, sig=sig)
                    v_ = wo.potential_generate(cfg)
                    a_, b_ = wo.ab(cfg, v_)
                    del v_
                    ex.upload_phi(phi0)
                    ex.evolve(3, 2)
                    got = ex.download_phi()
                    want = phi0.copy()
                    wo.evolve(cfg, 3, a_, b_, want, lowers, 2)
                    del a_, b_
                    worst = float(np.max(np.abs(got - want)))
                    result["excited_parity"] = {"against": "oracle/wafer_oracle.c wo_evolve (grid.rs:544-687 with wnum = 3)", "k": 3, "steps": 2,
                                                "max_abs": worst, "tolerance": 1e-13, "norm2_gpu": ex.norm2(), "norm2_oracle": wo.norm2(cfg, want)}
                    del got, want
                    if not (worst <= 1e-13):
                        rc = RC_PARITY
                    # ... and the two-steps-per-pass kernel (wafer_stencil_x2.hip.h: the default for one and two stored states)
                    # over six k = 1 steps -- two one-step passes, then two passes of two steps -- at the same bar
                    ex.upload_phi(phi0)
                    p_before = ex.x2_passes()
                    ex.evolve(1, 6)
                    got = ex.download_phi()
                    want = phi0.copy()
                    a_, b_ = wo.ab(cfg, wo.potential_generate(cfg))
                    wo.evolve(cfg, 1, a_, b_, want, lowers[:1], 6)
                    del a_, b_
                    worst2 = float(np.max(np.abs(got - want)))
                    result["excited_parity_two_steps_per_pass"] = {"against": "oracle/wafer_oracle.c wo_evolve (grid.rs:544-687 with wnum = 1)", "k": 1,
                                                                   "steps": 6, "two_step_passes": ex.x2_passes() - p_before, "max_abs": worst2,
                                                                   "tolerance": 1e-13}
                    del got, want
                    if not (worst2 <= 1e-13):
                        rc = RC_PARITY
                ex.upload_phi(phi0)
                del phi0, lowers
                ex.evolve(3, 150)   # the device idled while the oracle ran on the host: bring the clocks back up before timing (as --preheat does for the headline)
                for k in (1, 2, 3):
                    ex.evolve(k, 10)
                    ms_k, st_k = None, None
                    for _ in range(3):   # median of three 100-step evolves (a real run calls wafer_evolve with screen_update = 1000)
                        ex.evolve(k, 100)
                        m_, s_ = ex.last_evolve_ms()
                        ms_k = sorted(([] if ms_k is None else ms_k) + [m_])
                        st_k = s_
                    ms_k = ms_k[1]
                    p0_ = ex.x2_passes()
                    ex.evolve(k, 4)
                    spp_k = 2 if ex.x2_passes() > p0_ else 1
                    bpu_k = 80 + 32 * (k - 1)   # stencil + norm 32, normalise + dot 24, (k - 1) x (axpy + dot) 32, last axpy 24
                    rec[f"k{k}"] = {"ms_per_step": ms_k / st_k, "algorithmic_bytes_per_update": bpu_k, "steps_per_pass": spp_k,
                                    "frac_of_hbm_peak": pts_total * bpu_k / (ms_k / st_k * 1e-3) / 1e9 / HBM_PEAK_GBPS}
                ex.close()
                result["excited_state_step"] = {"grid": list(shape), "potential": potential, **rec,
                                                "stored_states": "box modes (1,1,1), (2,1,1), (1,1,2)",
                                                "note": "wafer_evolve(wnum = k) on the same grid, HIP events, median of three 100-step evolves after a 150-step warm-up (steps_per_pass 2: two one-step passes, 49 two-step passes and the pass that materialises phi; a real run's calls are 1000 steps long); checked by excited_parity and excited_parity_two_steps_per_pass"}
            except Exception as e:  # reported, never silently dropped
                result["excited_state_step"] = {"error": repr(e)}

    if dist is not None:   # the process group goes first: its work objects refer to the engine's streams
        ctx.synchronize()
        if hasattr(comm, "close"):
            comm.close()       # the native hooks' communicator
        dist.barrier()
        dist.destroy_process_group()
    ctx.close()
    if rank == 0:
        result_out.write(json.dumps(result) + "\n")
        result_out.flush()
        if rc != 0:
            print("bench.py: PARITY FAILURE -- the timed kernel's result differs from the reference: "
                  + json.dumps(result.get("parity")), file=sys.stderr)
    return rc


def main() -> int:
    args = parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    world_env = os.environ.get("WORLD_SIZE")
    if world_env is None and args.gpus > 1:
        return launch_ranks(args)          # bare call: this process never touches a GPU
    if world_env is not None and int(world_env) != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world_env}: refusing to mislabel the run", file=sys.stderr)
        return 2
    return run_rank(args)


if __name__ == "__main__":
    sys.exit(main())
