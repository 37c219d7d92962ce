"""Engine-side z-slab logic on ONE GPU: several contexts, each owning a z-slab
of the same grid, run in lock-step threads; their comm hooks are satisfied by
device-to-device copies and a host-side sum instead of RCCL.  The decomposed
result must equal the single-context result (bit for bit for the ground state:
a halo exchange moves bytes, it does no arithmetic)."""
import ctypes as C
import functools
import os
import re
import signal
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Several ranks of a decomposed run live in ONE process on ONE GPU here; wafer_peer_connect refuses a neighbour that is another
# context on its own device unless told that this is on purpose (read once per context).
os.environ.setdefault("WAFER_PEER_SAME_DEVICE", "1")

def peer_store_process(fn):
    """Runs each parameter set of the decorated test in a pytest process of its own, where run_slabs runs connected
    slabs as one process per rank (run_slabs_as_processes).  In overlap mode 3 a rank's kernel polls for
    stores of its neighbour's kernel (modes 4 - 6: copies ordered by a credit rendezvous); with the ranks as contexts of ONE
    process the runtime folds their streams onto the process's few hardware queues, and where two such kernels share one the
    waiter sits in front of the kernel it waits for until its bounded wait gives up."""
    @functools.wraps(fn)
    def wrapper(*args, request, **kwargs):
        if os.environ.get("WAFER_TEST_CHILD") == "1":
            return fn(*args, **kwargs)
        env = dict(os.environ, WAFER_TEST_CHILD="1", WAFER_TEST_RANK_PROCESSES="1")
        # (a session of its own: on a time-out the child's rank processes go with it)
        p = subprocess.Popen([sys.executable, "-m", "pytest", request.node.nodeid, "-q", "-rA", "-m", "gpu", "-p", "no:cacheprovider"],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=request.config.rootpath,
                             start_new_session=True)
        try:
            out, err = p.communicate(timeout=280)
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGKILL)
            out, err = p.communicate()
            raise AssertionError(f"{request.node.name}: no verdict within 280 s\n{out[-6000:]}{err[-2000:]}")
        verdicts = dict((m.group(2), m.group(1)) for m in re.finditer(r"^(PASSED|FAILED|ERROR) \S*::(\S+)", out, re.M))
        assert verdicts.get(request.node.name) == "PASSED", f"{request.node.name}: {verdicts.get(request.node.name)}\n{out[-6000:]}{err[-2000:]}"
    # pytest must see `request` among the arguments it fills in
    import inspect
    sig = inspect.signature(fn)
    if "request" not in sig.parameters:
        wrapper.__signature__ = sig.replace(parameters=[*sig.parameters.values(), inspect.Parameter("request", inspect.Parameter.KEYWORD_ONLY)])
    return wrapper


def _loaded_hip_runtime():
    """the libamdhip64 this process already runs on (torch's bundled one when torch is present):
    a second copy would be a second, unrelated HIP runtime"""
    import wafer_amd
    wafer_amd.load_library()
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return line.split()[-1]
    return "libamdhip64.so"


class FakeFabric:
    """In-process stand-in for RCCL: rank r's hooks rendezvous on barriers."""

    def __init__(self, world):
        self.world = world
        self.hip = C.CDLL(_loaded_hip_runtime())
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.bar = threading.Barrier(world)
        self.send = [dict() for _ in range(world)]
        self.scal = [None] * world
        self.halo_calls = [0] * world
        self.reduce_calls = [0] * world
        self.peer_recs = [None] * world
        self.call = [None] * world   # what each rank's current hook call is: RCCL wants the same sequence of operations on every rank

    def connect_peers(self, ctx, rank):
        """wafer_peer_export / wafer_peer_connect between the contexts of this process (the precondition of overlap mode 3:
        boundary workgroups store into the neighbour's ghost planes themselves)"""
        self.peer_recs[rank] = ctx.peer_export()
        self.bar.wait()
        ctx.peer_connect(self.peer_recs[rank - 1] if rank > 0 else None, self.peer_recs[rank + 1] if rank < self.world - 1 else None)
        self.bar.wait()

    def hooks(self, rank):
        hip = self.hip

        def halo(slo, shi, rlo, rhi, nbytes, stream):
            assert hip.hipStreamSynchronize(stream) == 0   # my boundary planes are final
            self.send[rank] = dict(lo=slo, hi=shi)
            self.call[rank] = ("halo", nbytes)
            self.bar.wait()
            assert all(c == self.call[rank] for c in self.call), f"ranks are in different hook calls: {self.call}"
            if rlo:  # my lower ghost planes <- lower neighbour's top owned planes
                assert hip.hipMemcpy(rlo, self.send[rank - 1]["hi"], nbytes, 3) == 0
            if rhi:
                assert hip.hipMemcpy(rhi, self.send[rank + 1]["lo"], nbytes, 3) == 0
            # (None also on a side that has a neighbour: overlap mode 2 exchanges one direction at a time)
            assert (rlo is None or rank > 0) and (rhi is None or rank < self.world - 1)
            # a device-to-device hipMemcpy may return before the copy is done (no host-side
            # synchronisation for that kind), and the engine's streams are non-blocking: wait here
            assert hip.hipStreamSynchronize(None) == 0
            self.halo_calls[rank] += 1
            self.bar.wait()
            return 0

        def allreduce(ptr, count, stream):
            assert hip.hipStreamSynchronize(stream) == 0
            buf = (C.c_double * count)()
            assert hip.hipMemcpy(buf, ptr, 8 * count, 2) == 0
            self.scal[rank] = np.array(buf[:])
            self.call[rank] = ("allreduce", count)
            self.bar.wait()
            assert all(c == self.call[rank] for c in self.call), f"ranks are in different hook calls: {self.call}"
            total = np.sum(np.stack(self.scal), axis=0)   # same order on every rank
            self.bar.wait()
            out = (C.c_double * count)(*total)
            assert hip.hipMemcpy(ptr, out, 8 * count, 1) == 0
            self.reduce_calls[rank] += 1
            return 0

        return halo, allreduce


def run_slabs(wa, base, world, body, connect=None):
    """body(ctx, rank) runs in one thread per slab; returns the list of results.  connect: wafer_peer_connect between the slabs
    (None: where overlap mode 3 could apply -- ThreePoint with three ghost planes).  Under WAFER_TEST_RANK_PROCESSES=1 connected
    slabs run as processes instead (run_slabs_as_processes)."""
    from wafer_amd.slab import partition
    import dataclasses
    peers = connect or (connect is None and base.ext == 1 and base.halo_depth >= 3)
    if world >= 2 and peers and os.environ.get("WAFER_TEST_RANK_PROCESSES") == "1":
        return run_slabs_as_processes(base, world, body, connect)
    fabric = FakeFabric(world)
    results, errors = [None] * world, []

    def work(rank):
        try:
            zb, zc = partition(base.nz, world, rank)
            par = dataclasses.replace(base, z_begin=zb, z_count=zc)
            with wa.Context(par) as ctx:
                # Overlap mode 4 in THIS harness (several contexts of one process on ONE device): a one-wave kernel of rank B that
                # waits for rank A's credit keeps the device busy, and a device-wide synchronisation on A's host thread (hipFree
                # inside download_phi, hipMalloc) then waits for that kernel while A has not yet enqueued the signal it waits for.
                # Bodies call ctx.rendezvous() between their last blocking call and an evolve under mode 4.  One process per GPU
                # (every real run): a device-wide synchronisation sees one rank's work only.
                ctx.rendezvous = fabric.bar.wait
                ctx.set_comm_hooks(*fabric.hooks(rank))
                if connect or (connect is None and par.ext == 1 and par.halo_depth >= 3):
                    fabric.connect_peers(ctx, rank)
                results[rank] = body(ctx, rank)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
            fabric.bar.abort()

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    if errors:
        raise errors[0]
    return results, fabric


def run_slabs_as_processes(base, world, body, connect=None, timeout=240):
    """run_slabs with one process per slab (tests/slab_rank_worker.py): the same body, results and halo hook counts.  Kernels
    that wait for a neighbour's stores or copies must all be resident at once; contexts of ONE process share its few hardware
    queues, and two such kernels can land on one queue, the waiter in front of the kernel it waits for.  A
    process per rank has queues of its own, as every real run does.  The fabric is gloo with host staging instead of in-process
    copies (bytes move differently, the engine's arithmetic is the same)."""
    import pickle
    import socket
    import tempfile
    import types
    import cloudpickle
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as tmp:
        job = os.path.join(tmp, "job.pkl")
        with open(job, "wb") as f:
            cloudpickle.dump((base, body, connect), f)
        procs, logs = [], []
        try:
            for r in range(world):
                logs.append(open(os.path.join(tmp, f"rank{r}.log"), "w+"))
                env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                           MASTER_PORT=str(port), WAFER_PEER_SAME_DEVICE="1", PYTHONUNBUFFERED="1")
                procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "slab_rank_worker.py"), job,
                                               os.path.join(tmp, f"out{r}.pkl")], env=env, cwd=ROOT, stdout=logs[-1],
                                              stderr=subprocess.STDOUT))
            codes = []
            for p in procs:
                try:
                    codes.append(p.wait(timeout=timeout))
                except subprocess.TimeoutExpired:
                    codes.append(None)
                    break
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
                    p.wait()
            text = []
            for r, f in enumerate(logs):
                f.seek(0)
                text.append(f"--- rank {r} ---\n" + f.read()[-3000:])
                f.close()
        if codes != [0] * world:
            raise AssertionError(f"slab rank processes exited with {codes}\n" + "\n".join(text))
        outs = []
        for r in range(world):
            with open(os.path.join(tmp, f"out{r}.pkl"), "rb") as f:
                outs.append(pickle.load(f))
    return [o[0] for o in outs], types.SimpleNamespace(halo_calls=[o[1] for o in outs])


def assemble(base, world, pieces):
    from wafer_amd.slab import partition
    e = base.ext
    out = np.zeros(base.padded_shape)
    for r, p in enumerate(pieces):
        zb, zc = partition(base.nz, world, r)
        out[:, :, zb + e:zb + zc + e] = p[:, :, zb + e:zb + zc + e]
    return out


def assemble_with_ghosts(base, world, pieces):
    """like assemble, for arrays that are valid on the frame planes too (the potential)"""
    from wafer_amd.slab import partition
    e = base.ext
    out = np.zeros(base.padded_shape)
    for r, p in enumerate(pieces):
        zb, zc = partition(base.nz, world, r)
        lo = 0 if r == 0 else zb + e
        hi = base.nz + 2 * e if r == world - 1 else zb + zc + e
        out[:, :, lo:hi] = p[:, :, lo:hi]
    return out


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


@pytest.mark.parametrize("overlap", [True, False, 2])   # 2: the single-launch pass (three-step passes only: here as mode 1)
@pytest.mark.parametrize("world,shape,ext", [(2, (40, 24, 32), 1), (3, (33, 17, 31), 2), (2, (20, 20, 12), 3),
                                            (4, (130, 12, 40), 1)])
def test_ground_state_slabs_bit_exact(wa, world, shape, ext, overlap):
    base = wa.Params(*shape, dn=0.2, dt=0.004, mass=1.0, central_difference=ext)
    steps = 12
    with wa.Context(base) as ctx:
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        want = ctx.download_phi()
        want_obs = ctx.observables()

    def body(ctx, rank):
        ctx.set_overlap(overlap)
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, 5)
        ctx.evolve(0, steps - 5)
        return ctx.download_phi(), ctx.observables()

    res, fabric = run_slabs(wa, base, world, body)
    got = assemble(base, world, [r[0] for r in res])
    assert np.array_equal(got, want)
    for _, obs in res:   # every rank holds the all-reduced observables
        for k in want_obs:
            assert obs[k] == pytest.approx(want_obs[k], rel=1e-12, abs=1e-300)
    assert all(n == steps for n in fabric.halo_calls)   # one exchange per step, none extra


@pytest.mark.parametrize("overlap", [True, False, 2])
@pytest.mark.parametrize("world,shape,ext,steps", [(2, (40, 24, 32), 1, 12), (3, (33, 17, 31), 2, 7), (4, (130, 12, 40), 1, 9),
                                                  (2, (300, 70, 96), 1, 6), (2, (130, 40, 100), 2, 5)])   # thick slabs: the mixed long / short interior launch
def test_fused_kernel_on_slabs_bit_exact(wa, world, shape, ext, steps, overlap):
    """two fused steps per pass on z-slabs: 2*ext ghost planes, one exchange of
    2*ext planes per pass (plus ext planes after an odd trailing step)"""
    base = wa.Params(*shape, dn=0.2, dt=0.004, mass=1.0, central_difference=ext, halo_depth=2 * ext)
    with wa.Context(wa.Params(*shape, dn=0.2, dt=0.004, mass=1.0, central_difference=ext)) as ctx:
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 3)
        want = ctx.download_phi()

    def body(ctx, rank):
        ctx.set_stencil_variant(2)
        ctx.set_overlap(overlap)
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 3)
        return ctx.download_phi()

    res, fabric = run_slabs(wa, base, world, body)
    assert np.array_equal(assemble(base, world, res), want)


@pytest.mark.parametrize("overlap", [True, False, 2])
@pytest.mark.parametrize("cycle", [2, 3])
@pytest.mark.parametrize("world,shape,ext,steps", [(2, (40, 24, 32), 1, 12), (3, (33, 17, 37), 2, 7), (4, (130, 12, 40), 1, 9),
                                                  (2, (300, 70, 96), 1, 10), (2, (20, 20, 12), 1, 8)])
def test_deep_halo_cycles_bit_exact(wa, world, shape, ext, steps, cycle, overlap):
    """deep halos (wafer_set_halo_cycle): 2 * ext * cycle ghost planes exchanged once per `cycle` fused
    passes, the passes in between run unsplit over the owned planes plus the still-valid ghost planes.
    Same bits as one context, and fewer exchanges than one per pass."""
    base = wa.Params(*shape, dn=0.2, dt=0.004, mass=1.0, central_difference=ext, halo_depth=2 * ext * cycle)
    with wa.Context(wa.Params(*shape, dn=0.2, dt=0.004, mass=1.0, central_difference=ext)) as ctx:
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 3)
        ctx.evolve(0, 8)
        want = ctx.download_phi()

    def body(ctx, rank):
        ctx.set_stencil_variant(2)
        ctx.set_overlap(overlap)
        ctx.set_halo_cycle(cycle)
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 3)           # an odd count: a trailing single step and its ext-plane exchange in between
        ctx.evolve(0, 8)
        return ctx.download_phi()

    res, fabric = run_slabs(wa, base, world, body)
    assert np.array_equal(assemble(base, world, res), want)
    passes = steps // 2 + 1 + 4
    assert all(n <= passes // cycle + 6 for n in fabric.halo_calls), fabric.halo_calls   # fewer exchanges than passes
    with pytest.raises(wa.WaferError):
        with wa.Context(wa.Params(*shape, dn=0.2, dt=0.004, central_difference=ext, z_begin=0, z_count=shape[2] // 2,
                                  halo_depth=2 * ext)) as ctx:
            ctx.set_halo_cycle(2)      # needs 4 * ext ghost planes
    with pytest.raises(wa.WaferError):     # a ghost zone deeper than the slab: the neighbour would need planes this rank does not own
        wa.Context(wa.Params(*shape, dn=0.2, dt=0.004, central_difference=ext, z_begin=0, z_count=2 * ext, halo_depth=2 * ext + 1))


F3_SLAB_CASES = [(2, (40, 24, 32), 12), (3, (140, 17, 37), 7), (4, (130, 33, 48), 10), (2, (300, 70, 96), 11)]


# overlap 2: ONE launch per pass, two halves marched outwards, exchanges released by counters; 3: ... with peer stores instead of
# exchanges (four contexts on ONE GPU share hardware queues: that case runs in test_peer_store_four_slabs_in_a_subprocess)
@pytest.mark.parametrize("world,shape,steps,cycle,overlap",
                         [(w, sh, st, cy, ov) for (w, sh, st) in F3_SLAB_CASES for cy in (1, 2) for ov in (True, False, 2, 3) if not (ov == 3 and w > 3)])
@peer_store_process   # (mode 3 among the parameters: three slabs run as processes)
def test_three_step_kernel_on_slabs_bit_exact(wa, world, shape, steps, cycle, overlap, monkeypatch):
    """three fused ThreePoint steps per pass on z-slabs (3 ghost planes per pass and side; 6 with one exchange
    per two passes): boundary-first overlap, the mixed long / short interior launch, two-step and single-step
    remainders with their own exchange depths in between -- the same bits as one context"""
    monkeypatch.setenv("WAFER_FUSE3_MIN_NY", "1")
    base = wa.Params(*shape, dn=0.2, dt=0.004, mass=1.0, central_difference=1, halo_depth=3 * cycle)
    with wa.Context(wa.Params(*shape, dn=0.2, dt=0.004, mass=1.0, central_difference=1)) as ctx:
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 5)
        ctx.evolve(0, 9)
        want = ctx.download_phi()

    def body(ctx, rank):
        assert ctx.stencil_kernel_name() == "wafer_k_step3_fused" and ctx.steps_per_launch() == 3
        ctx.set_overlap(overlap)
        ctx.set_halo_cycle(cycle)
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 5)           # one three-step pass + one two-step pass
        ctx.evolve(0, 9)
        return ctx.download_phi()

    res, fabric = run_slabs(wa, base, world, body)
    got = assemble(base, world, res)
    if not np.array_equal(got, want):   # say where: which padded planes, against the slabs' boundaries
        from wafer_amd.slab import partition
        planes = sorted(set(np.argwhere(got != want)[:, 2].tolist()))
        raise AssertionError(f"{int(np.sum(got != want))} cells differ on padded planes {planes}; slabs (z_begin, z_count): "
                             f"{[partition(shape[2], world, r) for r in range(world)]}; halo calls {fabric.halo_calls}")
    passes = -(-steps // 3) + 2 + 3
    per_pass = 2 if (overlap == 2 and cycle == 1) else 1   # mode 2: one hook call per half of the slab
    assert all(n <= per_pass * passes // cycle + 6 for n in fabric.halo_calls), fabric.halo_calls
    if overlap == 3 and cycle == 1:   # peer stores: the hook serves the first pass of each call and the remainders only
        assert all(n <= 3 + 2 + 3 for n in fabric.halo_calls), fabric.halo_calls


@pytest.mark.parametrize("overlap", [0, 1, 2])
def test_three_step_kernel_on_slabs_without_the_division_plan_bit_exact(wa, overlap, monkeypatch):
    """the case above on its smallest shape with WAFER_FLAG_UNPLANNED_DIV on the base Params: every slab runs the VIR = false
    instantiations (overlap 2: the single-launch pass, MODE = 1) and the assembled slabs hold one context's bits"""
    monkeypatch.setenv("WAFER_FUSE3_MIN_NY", "1")
    world, shape, steps = F3_SLAB_CASES[0]
    kw = dict(dn=0.2, dt=0.004, mass=1.0, central_difference=1, unplanned_div=True)
    base = wa.Params(*shape, halo_depth=3, **kw)
    with wa.Context(wa.Params(*shape, **kw)) as ctx:
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        assert ctx.stencil_kernel_instance().startswith("wafer_k_step3_fused<double, double, false, 0,"), ctx.stencil_kernel_instance()
        ctx.evolve(0, 5)
        ctx.evolve(0, 9)
        want = ctx.download_phi()

    def body(ctx, rank):
        assert ctx.stencil_kernel_name() == "wafer_k_step3_fused" and ctx.steps_per_launch() == 3
        assert ctx.div_plan().checked == 0
        ctx.set_overlap(overlap)
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        instance = ctx.stencil_kernel_instance()      # (the launch and this call are on the slab's own thread)
        ctx.evolve(0, 5)
        ctx.evolve(0, 9)
        return ctx.download_phi(), instance

    res, fabric = run_slabs(wa, base, world, body, connect=False)
    for _, instance in res:
        print(f"overlap {overlap}: {instance}")
        assert instance.startswith("wafer_k_step3_fused<double, double, false, "), instance
    got = assemble(base, world, [phi for phi, _ in res])
    if not np.array_equal(got, want):
        from wafer_amd.slab import partition
        planes = sorted(set(np.argwhere(got != want)[:, 2].tolist()))
        raise AssertionError(f"{int(np.sum(got != want))} cells differ on padded planes {planes}; slabs (z_begin, z_count): "
                             f"{[partition(shape[2], world, r) for r in range(world)]}; halo calls {fabric.halo_calls}")


@pytest.mark.parametrize("world,shape,steps", [(2, (40, 24, 10), 12), (3, (140, 40, 13), 9), (2, (300, 70, 96), 15), (4, (130, 33, 17), 6),
                                               (2, (1100, 300, 80), 9)])   # the last: more than 64 tiles, i.e. short pieces in the schedule
def test_single_launch_pass_thin_and_uneven_slabs_bit_exact(wa, world, shape, steps, monkeypatch):
    """overlap mode 2 on slabs whose halves are thinner than the exchange depth (the side's boundary planes then reach
    into the other half: its exchange waits for both counters), on uneven partitions; several evolve calls, so that the
    alternating order of the halves carries over between calls"""
    monkeypatch.setenv("WAFER_FUSE3_MIN_NY", "1")
    base = wa.Params(*shape, dn=0.2, dt=0.004, mass=1.0, central_difference=1, halo_depth=3)
    with wa.Context(wa.Params(*shape, dn=0.2, dt=0.004, mass=1.0, central_difference=1)) as ctx:
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 3)
        ctx.evolve(0, 7)
        want = ctx.download_phi()
        want_n2 = ctx.norm2()

    def body(ctx, rank):
        ctx.set_overlap(2)
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 3)           # ONE single-launch pass: the order of the halves flips between calls
        ctx.evolve(0, 7)
        return ctx.download_phi(), ctx.norm2()

    res, fabric = run_slabs(wa, base, world, body)
    assert np.array_equal(assemble(base, world, [r[0] for r in res]), want)
    assert all(r[1] == pytest.approx(want_n2, rel=1e-12) for r in res)
    assert len(set(fabric.halo_calls)) == 1   # every rank made the same number of exchange calls


@pytest.mark.parametrize("layout", ["3", "4", "5"])   # the two halves marched outwards / whole columns, direction alternating per pass / by the
                                                        # slab's thickness: the thinner ranks of an uneven partition whole, the thicker in halves
@pytest.mark.parametrize("world,shape,steps", [(2, (40, 24, 12), 12), (3, (140, 40, 19), 9), (2, (300, 70, 96), 15), (3, (130, 33, 20), 6),
                                               (3, (260, 50, 40), 30)])
@peer_store_process
def test_peer_store_pass_uneven_slabs_bit_exact(wa, world, shape, steps, layout, monkeypatch):
    """overlap mode 3: the boundary workgroups of the single-launch pass store their planes into the neighbour's ghost planes
    and count themselves into its arrival counter (no exchange, no gate kernel, no second stream); uneven partitions, slabs
    down to the six planes the mode needs, several evolve calls (the order of the halves and the arrival counts carry over),
    an operation in between that invalidates the ghost planes; norm through the all-reduce hook"""
    monkeypatch.setenv("WAFER_FUSE3_MIN_NY", "1")
    monkeypatch.setenv("WAFER_HV_LAYOUT", layout)
    if layout == "5":   # (an even partition: every rank whole -- the uneven ones are the point)
        monkeypatch.setenv("WAFER_HV_WHOLE_MAX", str(shape[2] // world))
    base = wa.Params(*shape, dn=0.2, dt=0.004, mass=1.0, central_difference=1, halo_depth=3)
    with wa.Context(wa.Params(*shape, dn=0.2, dt=0.004, mass=1.0, central_difference=1)) as ctx:
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 3)
        ctx.normalise(0.25)        # (a power of two: the slabs' all-reduced norm would differ from one context's in its last bits)
        ctx.evolve(0, 7)
        want = ctx.download_phi()
        want_n2 = ctx.norm2()

    def body(ctx, rank):
        ctx.set_overlap(3)
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 3)           # ONE single-launch pass: the order of the halves flips between calls
        ctx.normalise(0.25)
        ctx.evolve(0, 7)
        return ctx.download_phi(), ctx.norm2()

    res, fabric = run_slabs(wa, base, world, body)
    assert np.array_equal(assemble(base, world, [r[0] for r in res]), want)
    assert all(r[1] == pytest.approx(want_n2, rel=1e-12) for r in res)
    # the halo hook ran for the first pass of each call and for the two-step / single-step remainders, never per pass
    assert all(n <= 8 for n in fabric.halo_calls), fabric.halo_calls


@pytest.mark.parametrize("sched", ["2", "1", "0"])   # the schedule under the copies: single launch on two halves / boundary planes first / exchange after the pass
@pytest.mark.parametrize("world,shape,steps", [(2, (40, 24, 12), 12), (3, (140, 40, 19), 9), (2, (300, 70, 96), 15), (3, (130, 33, 20), 6),
                                               (3, (260, 50, 40), 30), (4, (64, 20, 13), 8)])
@peer_store_process
def test_peer_copy_pass_uneven_slabs_bit_exact(wa, world, shape, steps, sched, monkeypatch):
    """overlap mode 4 (round 6): every exchange of phi's ghost planes is a device copy from this rank's boundary planes INTO the
    neighbour's ghost planes (hipMemcpyAsync through the mapping wafer_peer_connect holds: the copy engines between GPUs),
    ordered by a credit / arrival rendezvous of one-wave kernels; the halo hook is never called.  Uneven partitions, slabs down
    to three planes (as thin as an exchange is deep), several evolve calls,
    an operation in between that invalidates the ghost planes, under each of the three schedules; norm through the all-reduce hook"""
    monkeypatch.setenv("WAFER_FUSE3_MIN_NY", "1")
    monkeypatch.setenv("WAFER_COPY_SCHED", sched)
    base = wa.Params(*shape, dn=0.2, dt=0.004, mass=1.0, central_difference=1, halo_depth=3)
    with wa.Context(wa.Params(*shape, dn=0.2, dt=0.004, mass=1.0, central_difference=1)) as ctx:
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 3)
        ctx.normalise(0.25)        # (a power of two: the slabs' all-reduced norm would differ from one context's in its last bits)
        ctx.evolve(0, 7)
        want = ctx.download_phi()
        want_n2 = ctx.norm2()

    def body(ctx, rank):
        ctx.set_overlap(4)
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 3)           # ONE single-launch pass: the order of the halves flips between calls
        ctx.normalise(0.25)
        ctx.evolve(0, 7)
        return ctx.download_phi(), ctx.norm2()

    res, fabric = run_slabs(wa, base, world, body)
    assert np.array_equal(assemble(base, world, [r[0] for r in res]), want)
    assert all(r[1] == pytest.approx(want_n2, rel=1e-12) for r in res)
    assert fabric.halo_calls == [0] * world, fabric.halo_calls       # nothing went through the hook


@pytest.mark.parametrize("mode", [5, 6])
@pytest.mark.parametrize("world,shape,steps", [(3, (140, 40, 19), 9), (4, (64, 20, 13), 8), (2, (300, 70, 96), 15)])
@peer_store_process
def test_peer_copies_under_the_split_and_the_unsplit_launches(wa, world, shape, steps, mode, monkeypatch):
    """overlap modes 5 / 6: the peer copies under mode 1's (boundary planes first) / mode 0's (exchange after the pass) launches, where
    every kernel that reads ghost planes starts after the copy that filled them has completed -- the forms of mode 4 that rest on
    nothing but what a completed memcpy guarantees; WAFER_COPY_SCHED plays no part; bit for bit against one context"""
    monkeypatch.setenv("WAFER_FUSE3_MIN_NY", "1")
    monkeypatch.setenv("WAFER_COPY_SCHED", "2")     # (mode 4's knob: must not matter here)
    base = wa.Params(*shape, dn=0.2, dt=0.004, mass=1.0, central_difference=1, halo_depth=3)
    with wa.Context(wa.Params(*shape, dn=0.2, dt=0.004, mass=1.0, central_difference=1)) as ctx:
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 5)
        want = ctx.download_phi()

    def body(ctx, rank):
        ctx.set_overlap(mode)
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 5)
        return ctx.download_phi()

    res, fabric = run_slabs(wa, base, world, body)
    assert np.array_equal(assemble(base, world, res), want)
    assert fabric.halo_calls == [0] * world


@pytest.mark.parametrize("ext,dtype", [(2, "f64"), (3, "f64"), (1, "f32"), (2, "f32fast")])
@peer_store_process
def test_peer_copies_serve_every_stencil_and_storage_type(wa, ext, dtype, monkeypatch):
    """mode 4 is a transport, not a kernel: FivePoint / SevenPoint passes (two steps / one step per pass, 4 / 3 ghost planes) and
    fp32 storage exchange their planes through the same copies -- against one context, bit for bit"""
    shape, world = (140, 40, 36), 3
    kw = dict(dn=0.2, dt=0.004, mass=1.0, central_difference=ext, dtype=dtype)
    with wa.Context(wa.Params(*shape, **kw)) as ctx:
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, 11)
        want = ctx.download_phi()
    depth = {1: 3, 2: 4, 3: 3}[ext]
    base = wa.Params(*shape, halo_depth=depth, **kw)

    def connect_and_run(ctx, rank):
        ctx.set_overlap(4)
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, 11)
        return ctx.download_phi()

    res, fabric = run_slabs(wa, base, world, connect_and_run, connect=True)
    assert np.array_equal(assemble(base, world, res), want)
    assert fabric.halo_calls == [0] * world


# potential, its parameters (BASELINE config #4's for SimpleCornell: m = 2.35, sig = 0.223, dn = 0.02, dt = 0.2 dn^2), per-cell bar
_ORACLE_CASES = [("SimpleCornell", dict(dn=0.02, dt=8e-5, mass=2.35, sig=0.223), 0.0),
                 ("QuadWell", dict(dn=0.2, dt=0.004, mass=1.0, sig=1.0), 0.0),         # z-special: the short side of the well lies along z
                 ("FullCornell", dict(dn=0.1, dt=0.002, mass=2.35, sig=0.223), 1e-12)]  # z-special (the anisotropic Debye mass; device libm: not bit exact); pot_sub is an ARRAY sharded with the slabs


@pytest.mark.parametrize("mode", [2, 3, 4])
@pytest.mark.parametrize("world,shape", [(2, (136, 40, 48)), (3, (130, 33, 50)), (4, (72, 36, 61))])
@pytest.mark.parametrize("case", _ORACLE_CASES, ids=[c[0] for c in _ORACLE_CASES])
@peer_store_process
def test_decomposed_ground_state_against_the_oracle_directly(wa, oracle, case, world, shape, mode, monkeypatch):
    """Every other test of this file compares slabs with ONE CONTEXT of the same engine (itself held against the oracle
    elsewhere): a slab whose potential were generated from the wrong global z would pass there if the single context shared
    the mistake.  Here the assembled slabs are held against the ORACLE: three-step passes in overlap modes 2 (single launch,
    exchange through the halo hook), 3 (peer stores) and 4 (peer copies), 2 - 4 uneven slabs, config #4's potential and two whose formula
    singles out z; the potential arrays themselves, the ground-state evolve (bit for bit where the potential is algebraic)
    and the all-reduced observables (pot_sub: a scalar for SimpleCornell, an array sharded with the slabs for FullCornell;
    r2 from the work-area index, grid.rs:428-437)."""
    wo = oracle
    potential, kw, bar = case
    monkeypatch.setenv("WAFER_FUSE3_MIN_NY", "1")
    cfg = wo.Config(*shape, ext=1, potential=potential, **kw)
    v = wo.potential_generate(cfg)
    a, b = wo.ab(cfg, v)
    phi = wo.initial_condition(cfg, "Boolean")
    calls = (13, 5)    # 4 three-step passes + 1 step; 1 pass + a two-step pass
    for n in calls:
        wo.evolve(cfg, 0, a, b, phi, [], n)
    want_obs = wo.observables(cfg, v, phi, wo.potential_sub(cfg))
    base = wa.Params(*shape, central_difference=1, halo_depth=3, **kw)

    def body(ctx, rank):
        ctx.set_overlap(mode)
        ctx.set_potential(potential)
        ctx.set_initial_condition("Boolean")
        for n in calls:
            ctx.evolve(0, n)
        return ctx.download_phi(), ctx.observables(), ctx.download_array("v"), ctx.steps_per_launch()

    res, fabric = run_slabs(wa, base, world, body)
    assert all(r[3] == 3 for r in res)                     # the three-step kernel (and with it the single-launch passes) ran
    got_v = assemble_with_ghosts(base, world, [r[2] for r in res])
    got = assemble(base, world, [r[0] for r in res])
    if bar == 0.0:
        assert np.array_equal(got_v, v), "a slab's potential differs from the oracle's"
        assert np.array_equal(got, phi), f"decomposed evolve differs from the oracle: {int(np.sum(got != phi))} cells, max {np.max(np.abs(got - phi))}"
    else:
        assert np.allclose(got_v, v, rtol=1e-13, atol=0)
        assert np.allclose(got, phi, rtol=0, atol=bar)
    for r in res:                                           # every rank holds the all-reduced sums
        for k, w in want_obs.items():
            assert r[1][k] == pytest.approx(w, rel=1e-11 if bar else 1e-12, abs=1e-300), (k, r[1][k], w)


def test_peer_connect_refuses_another_context_on_the_same_device(wa, monkeypatch):
    """two ranks folded onto one GPU poll for each other's stores from workgroups that hold the CUs the other's kernel needs:
    wafer_peer_connect says so unless WAFER_PEER_SAME_DEVICE=1 (this file sets it, on purpose); a slab that is its own neighbour
    (the self-loop of tools/slab_overhead.py) is no other context"""
    monkeypatch.delenv("WAFER_PEER_SAME_DEVICE")
    lo = wa.Params(64, 32, 40, dn=0.2, dt=0.004, central_difference=1, z_begin=0, z_count=20, halo_depth=3)
    hi = wa.Params(64, 32, 40, dn=0.2, dt=0.004, central_difference=1, z_begin=20, z_count=20, halo_depth=3)
    with wa.Context(lo) as c0, wa.Context(hi) as c1:
        with pytest.raises(wa.WaferError, match="WAFER_PEER_SAME_DEVICE"):
            c0.peer_connect(None, c1.peer_export())
        with pytest.raises(wa.WaferError):
            c0.set_overlap(3)
    mid = wa.Params(64, 32, 60, dn=0.2, dt=0.004, central_difference=1, z_begin=20, z_count=20, halo_depth=3)
    with wa.Context(mid) as c:
        rec = c.peer_export()
        c.peer_connect(rec, rec)
        c.set_overlap(3)


def test_peer_store_four_slabs_in_a_subprocess():
    """four slabs (two middle ranks), each a process of its own (run_slabs_as_processes): a kernel polling for its neighbour's
    stores never shares a hardware queue with that neighbour's kernel"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for layout in ("3", "4"):
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "peer_store_worker.py"), "4", "130,33,48", "10,5,9", "3", layout],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, WAFER_PEER_SAME_DEVICE="1", WAFER_TEST_RANK_PROCESSES="1"), cwd=root)
        assert r.returncode == 0 and "PEER-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("seed", [41, 42])
def test_randomised_slab_sweep_against_the_oracle(seed):
    """tests/fuzz_slabs.py: random grids, stencil orders, storage types, 2 - 4 uneven slabs, every overlap mode (peer stores in both
    pass layouts), deep halos, several evolve calls, potentials incl. the z-special ones -- the assembled slabs against the ORACLE
    bit for bit (fp32 storage: against one context), all-reduced observables to 1e-11; connected slabs as processes (run_slabs_as_processes)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz_slabs.py")], capture_output=True, text=True,
                       env=dict(os.environ, N="40", SEED=str(seed), WAFER_PEER_SAME_DEVICE="1", WAFER_TEST_RANK_PROCESSES="1"), timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "bad = 0" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_peer_copy_mode_needs_a_connection(wa):
    with wa.Context(wa.Params(64, 32, 32, dn=0.2, dt=0.004, z_begin=8, z_count=12, halo_depth=3)) as ctx:
        with pytest.raises(wa.WaferError) as e:
            ctx.set_overlap(4)
        assert "wafer_peer_connect" in str(e.value)
    with wa.Context(wa.Params(64, 32, 32, dn=0.2, dt=0.004)) as ctx:   # an undecomposed grid: nothing to connect, nothing to copy
        ctx.set_overlap(4)
        ctx.set_potential("Harmonic")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, 7)


def test_peer_store_mode_needs_a_connection(wa):
    par = wa.Params(64, 32, 40, dn=0.2, dt=0.004, central_difference=1, z_begin=0, z_count=20, halo_depth=3)
    with wa.Context(par) as ctx:
        with pytest.raises(wa.WaferError):
            ctx.set_overlap(3)
        with pytest.raises(wa.WaferError):
            ctx.peer_connect(ctx.peer_export(), None)    # a record for a side without a neighbour


def test_kernel_choice_on_slabs_does_not_depend_on_the_local_thickness(wa, monkeypatch):
    """ranks exchange K * ext planes per K-step pass, so K must not depend on anything local: an uneven partition whose
    slabs straddle the cell threshold of the three-step kernel (WAFER_FUSE3_MIN_CELLS) still gives every rank K = 3"""
    from wafer_amd.slab import partition
    import dataclasses
    shape, world = (64, 32, 45), 2
    sizes = [partition(shape[2], world, r)[1] for r in range(world)]
    assert len(set(sizes)) == 2
    monkeypatch.setenv("WAFER_FUSE3_MIN_CELLS", str(shape[0] * shape[1] * max(sizes) - 1))   # between the two slabs' cell counts
    base = wa.Params(*shape, dn=0.2, dt=0.004, central_difference=1, halo_depth=3)
    ks = []
    for r in range(world):
        zb, zc = partition(shape[2], world, r)
        with wa.Context(dataclasses.replace(base, z_begin=zb, z_count=zc)) as ctx:
            ks.append(ctx.steps_per_launch())
    assert ks == [3, 3]


@pytest.mark.parametrize("overlap", [2, 1, 0])
def test_all_fp32_three_step_kernel_on_slabs_bit_exact(wa, overlap, monkeypatch):
    """f32fast with three ghost planes: the three-step kernel (256 x 16 tiles) on z-slabs, every schedule, against one context"""
    monkeypatch.setenv("WAFER_FUSE3_MIN_NY", "1")
    shape, world, steps = (264, 40, 72), 3, 11
    base = wa.Params(*shape, dn=0.2, dt=0.004, central_difference=1, dtype="f32fast", halo_depth=3)
    with wa.Context(wa.Params(*shape, dn=0.2, dt=0.004, central_difference=1, dtype="f32fast")) as ctx:
        assert ctx.stencil_kernel_name() == "wafer_k_step3_fused"
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 3)
        want = ctx.download_phi()

    def body(ctx, rank):
        ctx.set_overlap(overlap)
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 3)
        return ctx.download_phi(), None

    res, _ = run_slabs(wa, base, world, body)
    assert np.array_equal(assemble(base, world, [r[0] for r in res]), want)


@pytest.mark.parametrize("overlap", [3, 2, 1, 0])
@pytest.mark.parametrize("world,shape", [(3, (264, 40, 72)), (2, (256, 32, 41))])   # ragged tiles / whole tiles (exact store counts), uneven slabs
@peer_store_process
def test_fp32_storage_three_step_kernel_on_slabs_bit_exact(wa, world, shape, overlap, monkeypatch):
    """dtype f32 (fp32 storage, fp64 arithmetic) with three ghost planes: the three-step kernel on z-slabs, every schedule -- peer
    stores (float stores into the neighbour's ghost planes) included -- against one context"""
    monkeypatch.setenv("WAFER_FUSE3_MIN_NY", "1")
    steps = 11
    base = wa.Params(*shape, dn=0.2, dt=0.004, central_difference=1, dtype="f32", halo_depth=3)
    with wa.Context(wa.Params(*shape, dn=0.2, dt=0.004, central_difference=1, dtype="f32")) as ctx:
        assert ctx.stencil_kernel_name() == "wafer_k_step3_fused"
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 3)
        want = ctx.download_phi()

    def body(ctx, rank):
        ctx.set_overlap(overlap)
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        ctx.evolve(0, 3)
        return ctx.download_phi(), ctx.steps_per_launch()

    res, _ = run_slabs(wa, base, world, body)
    assert all(r[1] == 3 for r in res)
    assert np.array_equal(assemble(base, world, [r[0] for r in res]), want)


@pytest.mark.parametrize("dtype", ["f32", "f32fast"])
def test_fp32_storage_on_slabs_bit_exact(wa, dtype):
    """fp32 storage (and fp32 step arithmetic) on z-slabs: the same bits as one context"""
    shape, world, steps = (264, 40, 72), 3, 9
    base = wa.Params(*shape, dn=0.2, dt=0.004, central_difference=1, dtype=dtype, halo_depth=2)
    with wa.Context(wa.Params(*shape, dn=0.2, dt=0.004, central_difference=1, dtype=dtype)) as ctx:
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        want = ctx.download_phi()
        want_obs = ctx.observables()

    def body(ctx, rank):
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        return ctx.download_phi(), ctx.observables()

    res, _ = run_slabs(wa, base, world, body)
    assert np.array_equal(assemble(base, world, [r[0] for r in res]), want)
    for _, obs in res:
        for k in want_obs:
            assert obs[k] == pytest.approx(want_obs[k], rel=1e-12, abs=1e-300)


def test_excited_state_and_solve_on_slabs(wa):
    import sys
    sys.setswitchinterval(1e-4)   # three lock-step threads hand the GIL over at every hook
    shape, world = (16, 16, 18), 3
    base = wa.Params(*shape, dn=0.55, dt=0.05, mass=1.0, central_difference=1, max_states=2)

    def solve_all(ctx, rank=0):
        ctx.set_potential("Harmonic")
        ctx.set_initial_condition("Gaussian", seed=9)
        energies = []
        for wnum in range(2):
            if wnum:
                # a fresh guess per state (the reference's alternative to its clone of the
                # previous state, grid.rs:70 vs :95; the clone is annihilated by Gram-Schmidt
                # down to rounding noise -- or to exactly zero, which is a NaN hazard)
                ctx.set_initial_condition("Gaussian", seed=9 + wnum)
            recs, final, conv = ctx.solve_state(wnum, 1e-7, 100, max_steps=20000)
            assert conv, (wnum, rank, recs[-3:])
            energies.append((final["energy"], final["r"], len(recs)))
        return energies, [ctx.download_state(i) for i in range(2)]

    with wa.Context(base) as ctx:
        want_e, want_states = solve_all(ctx)
    res, _ = run_slabs(wa, base, world, solve_all)
    for energies, _ in res:
        for (e, r, n), (we, wr, wn) in zip(energies, want_e):
            assert e == pytest.approx(we, abs=5e-7) and r == pytest.approx(wr, rel=1e-5)
            assert abs(n - wn) <= 1
    assert want_e[0][0] == pytest.approx(1.5, abs=0.06) and want_e[1][0] == pytest.approx(2.5, abs=0.1)
    ground = assemble(base, world, [r[1][0] for r in res])
    assert np.allclose(ground, want_states[0], rtol=0, atol=1e-8)


@pytest.mark.parametrize("overlap", [True, False, 2])
@pytest.mark.parametrize("world,shape,ext,wnum", [(2, (40, 24, 32), 1, 1), (3, (33, 17, 30), 2, 2), (4, (130, 20, 40), 1, 3),
                                                  # uneven THIN slabs (3, 2, 2, 2 / 3, 3, 2 planes): only some ranks are thick enough to split a step
                                                  # into boundary and interior launches -- the hooks must still be called in one order on every rank
                                                  # (round 5, found by tests/fuzz_slabs.py: halo exchange and all-reduce swapped places on the thin ranks)
                                                  (4, (140, 40, 9), 1, 3), (3, (24, 40, 8), 1, 3)])
def test_excited_state_steps_on_slabs(wa, world, shape, ext, wnum, overlap):
    """excited-state evolve (renormalise + Gram-Schmidt every step) on z-slabs against one context:
    with overlap the R boundary planes of each side are stepped first and their raw halo exchange
    runs behind the interior launch; the sums then associate per launch, so cells agree to 1e-13"""
    import sys
    sys.setswitchinterval(1e-4)
    base = wa.Params(*shape, dn=0.25, dt=0.006, mass=1.0, central_difference=ext, max_states=wnum)

    def body(ctx, rank=0):
        ctx.set_overlap(overlap)
        ctx.set_potential("Harmonic")
        for j in range(wnum):      # orthonormalised random stored states, identical on every slab
            ctx.set_initial_condition("Gaussian", seed=40 + j)
            ctx.normalise(ctx.norm2())
            ctx.orthogonalise(j)
            ctx.normalise(ctx.norm2())
            ctx.push_state()
        ctx.set_initial_condition("Gaussian", seed=7)
        ctx.evolve(wnum, 5)
        ctx.evolve(wnum, 2)
        return ctx.download_phi(), ctx.norm2()

    with wa.Context(base) as ctx:
        want, want_n2 = body(ctx)
    res, fabric = run_slabs(wa, base, world, body)
    got = assemble(base, world, [r[0] for r in res])
    err = float(np.max(np.abs(got - want))) / max(1.0, float(np.max(np.abs(want))))
    assert err <= 1e-13, f"max error {err:.3e} (600 runs of this case measured <= 3.8e-16), halo calls {fabric.halo_calls}"
    for _, n2 in res:
        assert n2 == pytest.approx(want_n2, rel=1e-12)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("world,shape,wnum,depth", [(2, (40, 24, 32), 1, 2), (3, (140, 17, 30), 2, 2), (4, (130, 20, 40), 3, 3),
                                                    (2, (24, 40, 9), 1, 2)])
def test_two_excited_steps_per_pass_on_slabs(wa, world, shape, wnum, depth, dtype, monkeypatch):
    """the two-steps-per-pass excited-state kernels (wafer_stencil_x2.hip.h) on z-slabs with two (or three) ghost planes:
    the raw result's two boundary planes per side travel after every pass, the stored states and their images A l_j carry
    two current ghost planes, the 2 + 3k sums are all-reduced -- against one context, 1e-12 per cell (sums associate per
    slab); thin and uneven slabs included"""
    import sys
    sys.setswitchinterval(1e-4)
    monkeypatch.setenv("WAFER_X2_MAX_K", "3")
    base = wa.Params(*shape, dn=0.25, dt=0.006, mass=1.0, central_difference=1, max_states=wnum, halo_depth=depth, dtype=dtype)
    single = wa.Params(*shape, dn=0.25, dt=0.006, mass=1.0, central_difference=1, max_states=wnum, dtype=dtype)
    # fp32 storage (round 6: the two-step kernels on a storage tag): the slabs' sums associate differently in their last bits, the
    # transform's coefficients with them, and a cell's rounding to float can then fall the other way: one float ulp, not 1e-12
    bar = 1e-12 if dtype == "f64" else 3e-7

    def body(ctx, rank=0):
        ctx.set_potential("Coulomb")
        for j in range(wnum):      # orthonormalised random stored states, identical on every slab
            ctx.set_initial_condition("Gaussian", seed=40 + j)
            ctx.normalise(ctx.norm2())
            ctx.orthogonalise(j)
            ctx.normalise(ctx.norm2())
            ctx.push_state()
        ctx.set_initial_condition("Gaussian", seed=7)
        ctx.evolve(wnum, 8)
        ctx.evolve(wnum, 5)
        assert ctx.x2_passes() == 3 + 1
        return ctx.download_phi(), ctx.norm2()

    with wa.Context(single) as ctx:
        want, want_n2 = body(ctx)
    res, fabric = run_slabs(wa, base, world, body)
    got = assemble(base, world, [r[0] for r in res])
    err = float(np.max(np.abs(got - want))) / max(1.0, float(np.max(np.abs(want))))
    assert err <= bar, f"max error {err:.3e}, halo calls {fabric.halo_calls}"
    for _, n2 in res:
        assert n2 == pytest.approx(want_n2, rel=1e-12 if dtype == "f64" else 1e-6)


@pytest.mark.parametrize("world,shape,ext,wnum,depth,steps", [(2, (40, 24, 32), 1, 1, 2, (8, 5)), (3, (33, 17, 30), 2, 2, 2, (5, 2)), (4, (130, 20, 40), 1, 3, 3, (8, 5)),
                                                               (4, (140, 40, 9), 1, 3, 1, (5, 2))])
@peer_store_process
def test_excited_state_steps_through_peer_copies(wa, world, shape, ext, wnum, depth, steps, monkeypatch):
    """overlap mode 4 under the excited-state steps: one plane per side and step (two per two-step pass) travels as a device copy
    into the neighbour's ghost planes, the sums through the all-reduce hook; the stored states' own ghost planes (exchanged once)
    keep the halo hook -- against one context, 1e-12 per cell; one-step and two-steps-per-pass kernels, thin uneven slabs"""
    import sys
    sys.setswitchinterval(1e-4)
    monkeypatch.setenv("WAFER_X2_MAX_K", "3")
    kw = dict(dn=0.25, dt=0.006, mass=1.0, central_difference=ext, max_states=wnum)
    base = wa.Params(*shape, halo_depth=depth, **kw)

    def body(ctx, rank=0):
        ctx.set_overlap(4)
        ctx.set_potential("Coulomb")
        for j in range(wnum):      # orthonormalised random stored states, identical on every slab
            ctx.set_initial_condition("Gaussian", seed=40 + j)
            ctx.normalise(ctx.norm2())
            ctx.orthogonalise(j)
            ctx.normalise(ctx.norm2())
            ctx.push_state()
        ctx.set_initial_condition("Gaussian", seed=7)
        for n in steps:
            ctx.evolve(wnum, n)
        return ctx.download_phi(), ctx.norm2(), ctx.x2_passes()

    with wa.Context(wa.Params(*shape, **kw)) as ctx:
        want, want_n2, _ = body(ctx)
    res, fabric = run_slabs(wa, base, world, body, connect=True)
    got = assemble(base, world, [r[0] for r in res])
    err = float(np.max(np.abs(got - want))) / max(1.0, float(np.max(np.abs(want))))
    assert err <= 1e-12, f"max error {err:.3e}, halo calls {fabric.halo_calls}"
    for _, n2, _ in res:
        assert n2 == pytest.approx(want_n2, rel=1e-12)
    assert len(set(r[2] for r in res)) == 1                      # every rank took the same kernels
    # the hook served the stored states' ghost planes only (never a step): a handful of calls, the same on every rank
    assert len(set(fabric.halo_calls)) == 1 and fabric.halo_calls[0] <= 4 * wnum


def test_slab_without_hooks_fails_loudly(wa):
    par = wa.Params(16, 16, 16, dn=0.2, dt=0.004, z_begin=0, z_count=8)
    with wa.Context(par) as ctx:
        ctx.set_potential("Harmonic")
        ctx.set_initial_condition("Boolean")
        with pytest.raises(wa.WaferError):
            ctx.evolve(0, 1)


@pytest.mark.parametrize("ext,dtype", [(1, "f64"), (3, "f64"), (2, "f32")])
def test_slab_host_transfers_touch_only_the_slab(wa, ext, dtype):
    """uploads take the slab's z-range out of a GLOBAL host array (gathered through pinned chunks:
    a memory-mapped file works as the source) and wafer_download_phi_owned returns exactly the owned
    work planes, (nx, ny, z_count)"""
    shape = (21, 18, 40)
    rng = np.random.default_rng(3)
    full = np.zeros(tuple(s + 2 * ext for s in shape))
    full[ext:-ext, ext:-ext, ext:-ext] = rng.standard_normal(shape)
    if dtype == "f32":
        full = full.astype(np.float32).astype(np.float64)
    for z0, zc in ((0, 13), (13, 17), (30, 10), (0, 0)):
        par = wa.Params(*shape, dn=0.2, dt=0.004, central_difference=ext, dtype=dtype, z_begin=z0, z_count=zc,
                        halo_depth=2 * ext if zc else 0)
        with wa.Context(par) as ctx:
            ctx.upload_phi(full)
            owned = ctx.download_phi_owned()
            zc_ = zc if zc else shape[2]
            assert owned.shape == (shape[0], shape[1], zc_)
            assert np.array_equal(owned, full[ext:-ext, ext:-ext, ext + z0:ext + z0 + zc_])
            back = ctx.download_phi()      # global-shaped: the slab's planes (ghosts included) and zeros elsewhere
            g = 2 * ext if zc else 0
            lo, hi = max(0, ext + z0 - g), min(full.shape[2], ext + z0 + zc_ + g)
            assert np.array_equal(back[:, :, ext + z0:ext + z0 + zc_], full[:, :, ext + z0:ext + z0 + zc_])
            assert not back[:, :, :lo].any() and not back[:, :, hi:].any()


def test_torch_hooks_alias_engine_memory(wa):
    """wafer_amd.slab.TorchSlabComm's plumbing on one GPU: the tensors it builds from the
    hooks' raw device addresses (__cuda_array_interface__), the ExternalStream it issues
    under, and the hook signatures -- with the collective itself replaced by an in-process
    exchange (RCCL needs one GPU per rank).  3 slabs, fused two-step path, bit exact."""
    import dataclasses
    import torch
    from wafer_amd.slab import TorchSlabComm, partition

    world, shape, ext, steps = 3, (40, 24, 36), 1, 9
    base = wa.Params(*shape, dn=0.2, dt=0.004, central_difference=ext, halo_depth=2 * ext, max_states=1)
    with wa.Context(wa.Params(*shape, dn=0.2, dt=0.004, central_difference=ext)) as ctx:
        ctx.set_potential("Coulomb")
        ctx.set_initial_condition("Boolean")
        ctx.evolve(0, steps)
        want = ctx.download_phi()
        want_obs = ctx.observables()

    bar = threading.Barrier(world)
    mail = [dict() for _ in range(world)]
    scal = [None] * world

    class Loopback(TorchSlabComm):
        def exchange(self, send_lo, send_hi, recv_lo, recv_hi):
            torch.cuda.current_stream().synchronize()
            mail[self.rank] = dict(lo=send_lo, hi=send_hi)
            bar.wait()
            if recv_lo is not None:
                assert recv_lo.dtype == torch.uint8 and recv_lo.is_cuda
                recv_lo.copy_(mail[self.rank - 1]["hi"])
            if recv_hi is not None:
                recv_hi.copy_(mail[self.rank + 1]["lo"])
            torch.cuda.current_stream().synchronize()
            bar.wait()
            return []

        def allreduce(self, t):
            assert t.dtype == torch.float64 and t.is_cuda
            torch.cuda.current_stream().synchronize()
            scal[self.rank] = t.clone()
            bar.wait()
            total = torch.stack(scal).sum(dim=0)
            bar.wait()
            t.copy_(total)
            torch.cuda.current_stream().synchronize()
            return t

    results, errors = [None] * world, []

    def work(rank):
        try:
            zb, zc = partition(base.nz, world, rank)
            with wa.Context(dataclasses.replace(base, z_begin=zb, z_count=zc)) as c:
                comm = Loopback(c, rank, world, torch.device("cuda", 0))
                c.set_potential("Coulomb")
                c.set_initial_condition("Boolean")
                c.evolve(0, steps)
                results[rank] = (c.download_phi(), c.observables())
                del comm
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
            bar.abort()

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    if errors:
        raise errors[0]
    assert np.array_equal(assemble(base, world, [r[0] for r in results]), want)
    for _, obs in results:
        for k in want_obs:
            assert obs[k] == pytest.approx(want_obs[k], rel=1e-12, abs=1e-300)
