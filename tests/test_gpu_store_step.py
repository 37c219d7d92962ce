"""Stepping the state stores on the device: wafer_k_batch_store_step through Batch.evolve_states, the context's host-only
wafer_evolve_states, the refusals, and subspace iteration (solve_block) against the numpy backend of tests/store_step_model.py.

The one guarantee: after evolve_states(k, n) every one of the first k stored states holds, bit for bit (==, uint64 views), what phi
holds after evolve(0, n) had phi started as that state -- held to a Context of the member's own Params on f64, f32 and f32fast and,
on f64, to the oracle's n steps.  phi, the states from k on, V and every member not listed keep every bit.

Shapes: (12, 10, 9) odd and smaller than a tile in x; (65, 6, 5) puts a column past the 64-wide tile and gives a ragged tile row;
(5, 4, 20) is cut into several z-chunks by the workgroup table (asserted from the table itself).  The calls n = 1, 2, 5 follow one
another on the same store (1, 3 and 8 steps in all), so both the odd path (the trailing copy) and the even path run, and a later call
starts from what an earlier one left in the slots and the shadows."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import ritz_model as rm  # noqa: E402
from tests import store_step_model as ssm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wafer_amd", "csrc")
DT = 0.004
DTYPES = ["f64", "f32", "f32fast"]
SHAPES = [(12, 10, 9), (65, 6, 5), (5, 4, 20)]
POTS = ["Harmonic", "Cube", "Periodic", "NoPotential", "Harmonic"]
CALLS = [1, 2, 5]
COMBOS = [(dtype, ext) for dtype in DTYPES for ext in (1, 2, 3)]


def storage_of(dtype):
    return np.float64 if dtype == "f64" else np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


@pytest.fixture(scope="module")
def wo():
    from oracle import wafer_oracle
    wafer_oracle.build()
    return wafer_oracle


def member(wa, shape, ext, dtype, m, max_states=10):
    """member m's Params: its own dn and mass (dt <= dn^2 / 3 for every one of them)"""
    return wa.Params(*shape, dn=0.2 + 0.03 * m, dt=DT, mass=1.3 - 0.1 * m, central_difference=ext, dtype=dtype, max_states=max_states)


def arrays_for(members, dtype, ext, counts, seed):
    """per member counts[m] N(0, 1) arrays on the work cells inside a zero frame, rounded to the storage type"""
    return [rm.random_states(p.work_shape, ext, counts[m], seed + 17 * m, frame=False, storage=storage_of(dtype)) for m, p in enumerate(members)]


def make_batch(wa, members, pots, states, phis):
    mixed = len({p.work_shape for p in members}) > 1
    b = wa.Batch(members, mixed_shapes=mixed, state_stores=mixed)
    if pots is not None:
        b.set_potentials(pots)
    for m, ls in enumerate(states):
        for j, l in enumerate(ls):
            b.load_state(m, j, l)
    if phis is not None:
        for m, phi in enumerate(phis):
            b.upload_phi(m, phi)
    return b


# ---- the workgroup table, from wafer_batch_plan.h itself -------------------------------------------------------------------------------
TABLE_DRIVER = r"""
#include "wafer_batch_plan.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv)
{   // R cus esz nx,ny,nz ... -> one line "member z0 z1" per entry of the one-step table over all members
    if (argc < 5) return 2;
    const int R = atoi(argv[1]), cus = atoi(argv[2]), esz = atoi(argv[3]);
    const uint32_t n = (uint32_t)(argc - 4);
    std::vector<int> nxyz(3 * n);
    for (uint32_t m = 0; m < n; ++m)
        if (sscanf(argv[4 + m], "%d,%d,%d", &nxyz[3 * m], &nxyz[3 * m + 1], &nxyz[3 * m + 2]) != 3) return 2;
    const WaferBatchLayout L = wafer_batch_layout(nxyz.data(), n, R, R, (size_t)esz);
    if (L.overflow) return 4;
    for (const WaferBatchBlock &b : wafer_batch_step_table(L.geoms.data(), L.shape_of.data(), nullptr, n, cus, 64, 4))
        printf("%d %d %d\n", b.member, b.z0, b.z1);
    return 0;
}
"""


@pytest.fixture(scope="module")
def zchunks(wa, tmp_path_factory):
    """(shapes, ext, dtype) -> per member the set of (z0, z1) of its table entries on this device"""
    d = tmp_path_factory.mktemp("store_step_table")
    src, exe = d / "table.cpp", d / "table"
    src.write_text(TABLE_DRIVER)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    with wa.Context(wa.Params(8, 8, 8, dn=0.2, dt=DT)) as ctx:
        cus = ctx.device_info()["compute_units"]

    def call(shapes, ext, dtype):
        out = subprocess.run([str(exe), str(ext), str(cus), "8" if dtype == "f64" else "4", *["%d,%d,%d" % s for s in shapes]],
                             capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr[-2000:]
        chunks = {}
        for line in out.stdout.splitlines():
            m, z0, z1 = [int(x) for x in line.split()]
            chunks.setdefault(m, set()).add((z0, z1))
        return chunks
    return call


# ---- 1. batch bits ---------------------------------------------------------------------------------------------------------------------
def context_steps(wa, p, pot, states, calls):
    """per state the padded arrays after each of the cumulative calls, from a Context of the member's Params: upload as phi, evolve(0, n)"""
    out = []
    with wa.Context(p) as ctx:
        ctx.set_potential(pot)
        for l in states:
            ctx.upload_phi(l)
            per_call = []
            for n in calls:
                ctx.evolve(0, n)
                per_call.append(ctx.download_phi())
            out.append(per_call)
    return out


def check_batch(wa, wo, zchunks, shapes, nst, ks, active, dtype, ext, seed):
    B = len(shapes)
    members = [member(wa, shape, ext, dtype, m) for m, shape in enumerate(shapes)]
    pots = [POTS[m % len(POTS)] for m in range(B)]
    arrays = arrays_for(members, dtype, ext, [n + 1 for n in nst], seed)
    states, phis = [a[:-1] for a in arrays], [a[-1] for a in arrays]
    listed = [m for m in range(B) if active is None or active[m]]
    refs = {m: context_steps(wa, members[m], pots[m], states[m][:ks[m]], CALLS) for m in listed}
    with make_batch(wa, members, pots, states, phis) as b:
        d = b.store_dispatch()
        assert d["kernel"].startswith("wafer_k_batch_store_step<%d," % ext) and d["states_per_workgroup"] == 4
        assert d["shapes"] == len(set(shapes))
        assert ("WaferBatchGeomTable" in d["kernel"]) == (len(set(shapes)) > 1)
        vs = [b.download_array(m, "v") for m in range(B)]
        if dtype == "f64":   # the oracle's n steps, from the device's own V
            cfgs = [wo.Config(*p.work_shape, ext=ext, potential="NoPotential", dn=p.dn, dt=p.dt, mass=p.mass) for p in members]
            abs_ = [wo.ab(cfgs[m], vs[m]) for m in range(B)]
            oracle_states = {m: [l.copy() for l in states[m][:ks[m]]] for m in listed}
        launches = 0
        assert b.store_counts() == 0
        for c, n in enumerate(CALLS):
            b.evolve_states(n, ks, active=active)
            launches += n + (n % 2)
            assert b.store_counts() == launches, (n, b.store_counts(), launches)   # n launches, or n + 1: whatever B, k and the shapes
            assert b.last_evolve_ms()[1] == n
            for m in range(B):
                k = ks[m] if m in listed else 0
                for j in range(nst[m]):
                    got = b.download_state(m, j)
                    if j >= k:
                        assert same(got, states[m][j]), ("untouched", m, j, n)
                        continue
                    assert same(got, refs[m][j][c]), ("context", shapes[m], dtype, ext, m, j, n)
                    if dtype == "f64":
                        wo.evolve(cfgs[m], 0, abs_[m][0], abs_[m][1], oracle_states[m][j], [], n)
                        assert same(got, oracle_states[m][j]), ("oracle", shapes[m], ext, m, j, n)
                assert same(b.download_phi(m), phis[m]), ("phi", m, n)
                assert same(b.download_array(m, "v"), vs[m]), ("V", m, n)
        # a listed member with k = 0 and an empty list cost nothing
        b.evolve_states(3, [0] * B)
        b.evolve_states(3, ks, active=[0] * B)
        assert b.store_counts() == launches
    return members


@pytest.mark.parametrize("dtype,ext", COMBOS)
def test_batch_bits_one_shape(wa, wo, zchunks, dtype, ext):
    for s, shape in enumerate(SHAPES):
        check_batch(wa, wo, zchunks, [shape] * 3, [2, 3, 8], [1, 3, 8], None, dtype, ext, seed=100 * s + ext)
    chunks = zchunks([SHAPES[2]] * 3, ext, dtype)
    assert all(len(chunks[m]) > 1 for m in range(3)), chunks   # nz = 20: several z-chunks per tile


@pytest.mark.parametrize("dtype,ext", COMBOS)
def test_batch_bits_mixed_shapes(wa, wo, zchunks, dtype, ext):
    """the three shapes in one batch with state stores, a fourth member with 4 stored states and k = 2, a fifth not listed"""
    shapes = SHAPES + [SHAPES[0], SHAPES[1]]
    check_batch(wa, wo, zchunks, shapes, [2, 3, 8, 4, 2], [1, 3, 8, 2, 2], [1, 1, 1, 1, 0], dtype, ext, seed=700 + ext)
    chunks = zchunks(shapes, ext, dtype)
    assert len(chunks[2]) > 1, chunks


# ---- 2. the excited-state steps see the stepped store -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_excited_steps_after_evolve_states_equal_a_fresh_batch(wa, dtype, variant):
    ext, shape = 1, (12, 10, 9)
    members = [member(wa, shape, ext, dtype, m) for m in range(3)]
    pots = POTS[:3]
    arrays = arrays_for(members, dtype, ext, [4, 4, 4], 31)
    states, phis = [a[:3] for a in arrays], [a[3] for a in arrays]
    with make_batch(wa, members, pots, states, phis) as b:
        b.set_gs_variant(variant)
        b.evolve(2, wnum=2)                       # the one-pass form has formed its Gram matrices from the old store
        b.evolve_states(3, [2, 3, 1])
        stepped = [[b.download_state(m, j) for j in range(3)] for m in range(3)]
        phi_now = [b.download_phi(m) for m in range(3)]
        assert not same(stepped[0][0], states[0][0]) and same(stepped[2][1], states[2][1])
        b.evolve(4, wnum=2)
        got = [b.download_phi(m) for m in range(3)]
        assert b.gs_steps() == ((6, 0) if variant == 1 else (0, 6))   # (the form asked for ran, before and after)
    with make_batch(wa, members, pots, stepped, phi_now) as f:
        f.set_gs_variant(variant)
        f.evolve(4, wnum=2)
        for m in range(3):
            assert same(got[m], f.download_phi(m)), (dtype, variant, m)


# ---- 3. contexts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(12, 10, 9), (130, 9, 7)])
@pytest.mark.parametrize("dtype,ext", COMBOS)
def test_context_evolve_states(wa, dtype, ext, shape):
    p = wa.Params(*shape, dn=0.2, dt=DT, mass=1.1, central_difference=ext, dtype=dtype, max_states=8)
    arrays = rm.random_states(shape, ext, 4, 900 + ext + sum(shape), frame=False, storage=storage_of(dtype))
    states, phi = arrays[:3], arrays[3]
    k = 2
    with wa.Context(p) as ctx:
        ctx.set_potential("Harmonic")
        for n in (1, 3, 7):   # ThreePoint: three-step passes plus both remainders
            for j, l in enumerate(states):
                ctx.load_state(j, l)
            want = []
            for j in range(k):
                ctx.clone_state_to_phi(j)
                ctx.evolve(0, n)
                want.append(ctx.download_phi())
            if n == 7:
                ctx.upload_phi(phi)
                ctx.evolve(1, 8)   # (the two-step excited pass, where it applies, has built its images of the old states)
            ctx.upload_phi(phi)
            ctx.evolve_states(k, n)
            assert ctx.last_evolve_ms()[1] == n
            for j in range(k):
                assert same(ctx.download_state(j), want[j]), (dtype, ext, shape, n, j)
            assert same(ctx.download_state(2), states[2]), n
            assert same(ctx.download_phi(), phi), ("phi / cur", n)   # (a flipped cur would show the other buffer)
        ctx.evolve(1, 8)
        got = ctx.download_phi()
        final = [ctx.download_state(j) for j in range(3)]
    with wa.Context(p) as fresh:
        fresh.set_potential("Harmonic")
        for j, l in enumerate(final):
            fresh.load_state(j, l)
        fresh.upload_phi(phi)
        fresh.evolve(1, 8)
        assert same(got, fresh.download_phi()), (dtype, ext, shape)


def test_context_evolve_states_needs_no_phi(wa):
    shape, ext = (12, 10, 9), 1
    p = wa.Params(*shape, dn=0.2, dt=DT, central_difference=ext, max_states=4)
    states = rm.random_states(shape, ext, 2, 5, frame=False)
    with wa.Context(p) as ref:
        ref.set_potential("Harmonic")
        ref.upload_phi(states[1])
        ref.evolve(0, 4)
        want = ref.download_phi()
    with wa.Context(p) as ctx:
        ctx.set_potential("Harmonic")
        for j, l in enumerate(states):
            ctx.load_state(j, l)
        ctx.evolve_states(2, 4)
        assert same(ctx.download_state(1), want)
        with pytest.raises(wa.WaferError):   # phi is still not set
            ctx.evolve(0, 1)


# ---- 4. refusals change nothing ------------------------------------------------------------------------------------------------------------
def test_batch_refusals_change_nothing(wa):
    from wafer_amd.engine import WAFER_ERR_INVALID, WAFER_ERR_STATE
    dtype, ext, B = "f64", 1, 3
    members = [member(wa, shape, ext, dtype, m) for m, shape in enumerate(SHAPES)]
    arrays = arrays_for(members, dtype, ext, [4, 4, 4], 55)
    states, phis = [a[:3] for a in arrays], [a[3] for a in arrays]

    def unchanged(b, vs):
        for m in range(B):
            assert same(b.download_phi(m), phis[m]), m
            for j in range(3):
                assert same(b.download_state(m, j), states[m][j]), (m, j)
            if vs[m] is not None:
                assert same(b.download_array(m, "v"), vs[m]), m
        assert b.store_counts() == 0

    def refused(b, ks, code, word, active=None):
        with pytest.raises(wa.WaferError, match=word) as e:
            b.evolve_states(2, ks, active=active)
        assert e.value.code == code, (ks, e.value)

    with make_batch(wa, members, None, states, phis) as b:
        b.set_potential(0, "Harmonic")
        b.set_potential(2, "Cube")
        vs = [b.download_array(0, "v"), None, b.download_array(2, "v")]
        refused(b, [2, 2, 2], WAFER_ERR_STATE, "member 1: potential")       # member 1 has no potential
        unchanged(b, vs)
        b.evolve_states(2, [2, 0, 2])                                       # ... which k = 0 does not need
        b.evolve_states(2, [2, 2, 2], active=[1, 0, 1])
        assert b.store_counts() == 4
    with make_batch(wa, members, POTS[:3], states, phis) as b:
        vs = [b.download_array(m, "v") for m in range(B)]
        refused(b, [2, 2, 9], WAFER_ERR_INVALID, "member 2")                # above WAFER_RITZ_MAX
        unchanged(b, vs)
        refused(b, [4, 2, 2], WAFER_ERR_STATE, "member 0")                  # above the member's stored states
        unchanged(b, vs)
        refused(b, [2, 2, 4], WAFER_ERR_STATE, "member 2")                  # the checks run for every member before any launch
        unchanged(b, vs)
    with wa.Batch(members, mixed_shapes=True) as b:                          # several shapes, no state stores
        b.set_potentials(POTS[:3])
        for m in range(B):
            b.upload_phi(m, phis[m])
        with pytest.raises(wa.WaferError, match="mixed-shape") as e:
            b.evolve_states(2, [1, 1, 1])
        assert e.value.code == WAFER_ERR_INVALID and "wafer_batch_evolve_states" in str(e.value)
        for m in range(B):
            assert same(b.download_phi(m), phis[m])


def test_context_refusals_change_nothing(wa):
    from wafer_amd.engine import WAFER_ERR_INVALID, WAFER_ERR_STATE
    shape, ext = (12, 10, 9), 1
    arrays = rm.random_states(shape, ext, 4, 77, frame=False)
    states, phi = arrays[:3], arrays[3]

    def refused(ctx, k, code):
        with pytest.raises(wa.WaferError) as e:
            ctx.evolve_states(k, 2)
        assert e.value.code == code, (k, e.value)
        for j in range(3):
            assert same(ctx.download_state(j), states[j]), (k, j)
        assert same(ctx.download_phi(), phi), k

    def loaded(ctx):
        for j, l in enumerate(states):
            ctx.load_state(j, l)
        ctx.upload_phi(phi)

    p = wa.Params(*shape, dn=0.2, dt=DT, central_difference=ext, max_states=10)
    with wa.Context(p) as ctx:
        loaded(ctx)
        refused(ctx, 2, WAFER_ERR_STATE)       # no potential
        ctx.set_potential("Harmonic")
        v = ctx.download_array("v")
        refused(ctx, 0, WAFER_ERR_INVALID)
        refused(ctx, 9, WAFER_ERR_INVALID)     # above WAFER_RITZ_MAX
        refused(ctx, 4, WAFER_ERR_STATE)       # above the stored states
        assert same(ctx.download_array("v"), v)
    slab = wa.Params(*shape, dn=0.2, dt=DT, central_difference=ext, max_states=10, z_begin=0, z_count=shape[2])
    with wa.Context(slab) as ctx:
        ctx.set_potential("Harmonic")
        loaded(ctx)
        with pytest.raises(wa.WaferError, match="z-slab"):
            ctx.evolve_states(2, 2)
        refused(ctx, 2, WAFER_ERR_INVALID)


# ---- 5. solve_block on the device ------------------------------------------------------------------------------------------------------------
DNS = [0.1, 0.11, 0.12]


def model_results(wo, kind, dns):
    """the numpy backend's loop on the members of the device run: the same potential and the same starting states"""
    members = []
    for dn in dns:
        v = np.zeros(tuple(n + 2 for n in ssm.SHAPE)) if kind == "free" else ssm.harmonic_v(ssm.SHAPE, 1, dn)
        members.append(ssm.Member(wo, ssm.SHAPE, dn, v, ssm.start_states()))
    return ssm.solve_block(members)


def check_against_model(r, model, kind, dn):
    from wafer_amd.engine import BLOCK_CONVERGED
    print(kind, dn, r["status"], r["blocks"], r["evals"], model["blocks"], model["evals"], r["rho"])
    assert r["status"] == model["status"] == BLOCK_CONVERGED
    assert abs(r["blocks"] - model["blocks"]) <= 1
    assert np.all(np.abs(r["evals"] - model["evals"]) <= 1e-9 * np.abs(model["evals"])), (r["evals"], model["evals"])
    if kind == "free":
        exact = ssm.box_levels(dn)
        assert np.all(np.abs(r["evals"] - exact) <= 1e-9 * exact), (r["evals"], exact)
        assert np.all(r["rho"] <= 1e-4)
    else:
        assert np.all(r["rho"] > 0.1)   # the floor of O(dt V): why rho is reported and never decides


def device_v(kind, dn):
    return np.zeros(tuple(n + 2 for n in ssm.SHAPE)) if kind == "free" else ssm.harmonic_v(ssm.SHAPE, 1, dn)


@pytest.mark.parametrize("kind", ["free", "harmonic"])
def test_context_solve_block(wa, wo, kind):
    dn = DNS[0]
    model = model_results(wo, kind, [dn])[0]
    p = wa.Params(*ssm.SHAPE, dn=dn, dt=ssm.dt_of(dn), central_difference=1, max_states=8)
    with wa.Context(p) as ctx:
        ctx.set_potential_host(device_v(kind, dn))
        for j, l in enumerate(ssm.start_states()):
            ctx.load_state(j, l)
        r = ctx.solve_block(ssm.K, ssm.TOLERANCE, ssm.STEPS_PER_BLOCK, ssm.MAX_BLOCKS)
    check_against_model(r, model, kind, dn)
    assert len(r["rows"]) == r["blocks"] and r["steps"] == r["blocks"] * ssm.STEPS_PER_BLOCK


@pytest.mark.parametrize("kind", ["free", "harmonic"])
def test_batch_solve_block(wa, wo, kind):
    models = model_results(wo, kind, DNS)
    members = [wa.Params(*ssm.SHAPE, dn=dn, dt=ssm.dt_of(dn), central_difference=1, max_states=8) for dn in DNS]
    with wa.Batch(members) as b:
        for m, dn in enumerate(DNS):
            b.set_potential_host(m, device_v(kind, dn))
            for j, l in enumerate(ssm.start_states()):
                b.load_state(m, j, l)
        before = b.store_counts()
        rs = b.solve_block(ssm.K, ssm.TOLERANCE, ssm.STEPS_PER_BLOCK, ssm.MAX_BLOCKS)
        # one launch per step for the members still going, whatever their number: an even block is exactly its steps
        assert b.store_counts() - before == ssm.STEPS_PER_BLOCK * max(r["blocks"] for r in rs)
    for m, dn in enumerate(DNS):
        check_against_model(rs[m], models[m], kind, dn)


def test_seed_states_fill_the_store_and_overwrite_phi(wa):
    p = wa.Params(9, 9, 9, dn=0.1, dt=ssm.dt_of(0.1), central_difference=1, max_states=8)
    with wa.Context(p) as ctx, wa.Batch([p, p]) as b:
        ctx.set_potential("NoPotential")
        ctx.seed_states(3, 11)
        b.set_potentials(["NoPotential"] * 2)
        b.seed_states(3, 11, active=[0, 1])
        assert ctx.num_states() == 3 and b.num_states() == [0, 3]
        for j in range(3):
            assert same(ctx.download_state(j), b.download_state(1, j))
        assert not same(ctx.download_state(0), ctx.download_state(1))
        assert same(ctx.download_phi(), ctx.download_state(2))   # phi holds the last of them
