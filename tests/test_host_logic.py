"""Host-side launch logic that needs no GPU: compiled with g++ from the headers the engine uses."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wafer_amd", "csrc")

HARNESS = r"""
#include "wafer_tuning.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv)
{
    // per_layer nplanes slots fill  ->  zchunk
    for (int i = 1; i + 3 < argc; i += 4)
        printf("%d\n", wafer_pick_zchunk(atoll(argv[i]), atoi(argv[i + 1]), atoll(argv[i + 2]), atoi(argv[i + 3])));
    return 0;
}
"""


@pytest.fixture(scope="module")
def pick(tmp_path_factory):
    d = tmp_path_factory.mktemp("host")
    src, exe = d / "pick.cpp", d / "pick"
    src.write_text(HARNESS)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

    def call(*cases):
        args = [str(x) for c in cases for x in c]
        out = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr[-2000:]
        return [int(x) for x in out.stdout.split()]
    return call


def makespan(per_layer, nplanes, slots, fill, zc):
    nch = -(-nplanes // zc)
    rounds = -(-per_layer * nch // slots)
    return rounds * (zc + fill)


def test_zchunk_choices_of_the_known_grids(pick):
    """what the three-step kernel (fill 6, 256 CUs) chooses: unchanged where rounds 1-2 measured it, the fix at 384^3"""
    got = pick((128, 512, 256, 6), (32, 256, 256, 6), (72, 384, 256, 6), (512, 128, 256, 6), (512, 1024, 256, 6))
    assert got == [256, 32, 55, 128, 1024]


@pytest.mark.parametrize("slots,fill", [(256, 6), (512, 3), (256, 5), (304, 6)])
def test_zchunk_minimises_the_makespan(pick, slots, fill):
    """exhaustively against a Python statement of the same cost, on awkward tile counts and plane counts"""
    cases = [(pl, n, slots, fill) for pl in (1, 3, 7, 32, 60, 72, 100, 128, 200, 512, 2048) for n in (1, 2, 5, 31, 64, 100, 128, 384, 1000)]
    got = pick(*cases)
    for (pl, n, s, f), zc in zip(cases, got):
        assert 1 <= zc <= n
        best = min(makespan(pl, n, s, f, -(-n // nch)) for nch in range(1, min(n, 64) + 1))
        assert makespan(pl, n, s, f, zc) == best, (pl, n, zc)


def test_zchunk_degenerate_arguments(pick):
    zc = pick((0, 10, 256, 6), (5, 1, 256, 6), (5, 10, 0, 6))
    assert all(1 <= z <= n for z, n in zip(zc, (10, 1, 10)))


# ---- workgroup schedules of the three-step kernel (wafer_stencil_fused3.hip.h, host code) ---------------------------------
SCHED = r"""
#include "wafer_stencil_fused3.hip.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv)
{
    std::vector<WaferF3Block> t;
    const int kind = atoi(argv[1]), ntx = atoi(argv[2]), nty = atoi(argv[3]), lo = atoi(argv[4]), hi = atoi(argv[5]);
    if (kind == 0) wafer_f3_schedule_plain(t, ntx, nty, lo, hi, atoi(argv[6]), atoi(argv[7]) != 0);
    else if (kind == 1) wafer_f3_schedule_mixed(t, ntx, nty, lo, hi, atoi(argv[6]));
    else {
        const bool nw[2] = {atoi(argv[8]) != 0, atoi(argv[9]) != 0};
        wafer_f3_schedule_halves(t, ntx, nty, lo, hi, atoi(argv[6]), atoi(argv[7]), nw, atoi(argv[10]), atoi(argv[11]), atoi(argv[12]), true, 0,
                                 atoi(argv[13]));
    }
    for (const auto &b : t) printf("%d %d %d %d %d %d %d %d\n", b.tile, b.zs, b.ze, b.down, b.wait_late, b.wait_it, b.bump, b.wt);
    return 0;
}
"""


@pytest.fixture(scope="module")
def sched(tmp_path_factory):
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("sched")
    src, exe = d / "sched.hip", d / "sched"
    src.write_text(SCHED)
    r = subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def call(*args):
        out = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr[-2000:]
        keys = ("tile", "zs", "ze", "down", "wait_late", "wait_it", "bump", "wt")
        return [dict(zip(keys, (int(x) for x in line.split()))) for line in out.stdout.splitlines()]
    return call


def covered_once(blocks, ntiles, lo, hi):
    for t in range(ntiles):
        planes = sorted(p for b in blocks if b["tile"] == t for p in range(b["zs"], b["ze"]))
        assert planes == list(range(lo, hi)), f"tile {t}: planes {planes[:5]}.. of [{lo}, {hi})"


@pytest.mark.parametrize("ntx,nty,lo,hi,zc,swz", [(4, 32, 0, 512, 256, 1), (3, 24, 3, 387, 55, 1), (1, 1, 0, 7, 3, 0), (2, 5, 3, 20, 100, 1),
                                                  (8, 64, 3, 131, 128, 1)])
def test_plain_schedule_covers_every_plane_of_every_tile_once(sched, ntx, nty, lo, hi, zc, swz):
    b = sched(0, ntx, nty, lo, hi, zc, swz)
    covered_once(b, ntx * nty, lo, hi)
    assert all(x["down"] == 0 and x["bump"] == -1 and x["wait_late"] == -1 for x in b)
    if swz:   # XCD-contiguous: the tiles dispatch slots b, b+8, b+16, ... (one XCD) work on are consecutive
        ids = [x["tile"] + (x["zs"] - lo) // zc * ntx * nty for x in b]
        assert sorted(ids) == list(range(len(b)))
        per_xcd = ids[0::8]
        assert per_xcd == list(range(per_xcd[0], per_xcd[0] + len(per_xcd)))


def test_mixed_schedule_long_columns_then_short_pieces(sched):
    b = sched(1, 8, 64, 6, 125, 4)
    covered_once(b, 512, 6, 125)
    n_long = sum(1 for x in b if (x["zs"], x["ze"]) == (6, 125))
    assert n_long == 512 - 32 and all((x["zs"], x["ze"]) == (6, 125) for x in b[:n_long])


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("need", [(1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize("ntx,nty,lo,nzl,nshort,nsub,layout", [(8, 64, 3, 128, 32, 4, 0), (8, 64, 3, 128, 32, 4, 1), (8, 64, 3, 128, 32, 4, 2),
                                                              (2, 3, 3, 16, 1, 2, 0), (1, 2, 3, 7, 0, 4, 0), (3, 5, 3, 37, 2, 3, 1),
                                                              (2, 2, 3, 5, 1, 2, 0)])
def test_halves_schedule_invariants(sched, ntx, nty, lo, nzl, nshort, nsub, layout, first, need):
    """what the engine's single-launch pass relies on (wafer_engine.hip launch_halves_pass): both halves cover their planes
    once; half A marches down to the lower boundary, half B up to the upper one; exactly one piece per tile and half stores
    the boundary, counts itself done and -- where that side has a neighbour -- waits for the ghost flag at the iteration
    whose prefetch first touches a ghost plane; the half named `first` is dispatched first"""
    hi, mid, depth, ntiles = lo + nzl, lo + nzl // 2, 3, ntx * nty
    b = sched(2, ntx, nty, lo, hi, mid, first, need[0], need[1], nshort, nsub, depth, layout)
    covered_once(b, ntiles, lo, hi)
    thin = mid - lo < depth or hi - mid < depth
    for x in b:
        half = 0 if x["down"] else 1
        assert (lo <= x["zs"] < x["ze"] <= mid) if half == 0 else (mid <= x["zs"] < x["ze"] <= hi)
        at_boundary = x["zs"] == lo if half == 0 else x["ze"] == hi
        assert (x["bump"] == half) == at_boundary and (x["bump"] in (-1, half))
        if at_boundary:
            n = x["ze"] - x["zs"]
            assert x["wt"] == (n if (thin or depth > n) else depth)
            if need[half]:
                assert x["wait_late"] == half
                # marching z1 = ze + 1 - it (down) / zs - 2 + it (up), the prefetch reads plane z -+ 2: first ghost plane at
                assert x["wait_it"] == (x["ze"] - lo if half == 0 else hi - x["zs"])
                assert 0 <= x["wait_it"] < (x["ze"] - x["zs"]) + 4
            else:
                assert x["wait_late"] == -1
        else:
            assert x["wait_late"] == -1 and x["wt"] == 0
    for half in (0, 1):
        assert sum(1 for x in b if x["bump"] == half) == ntiles
    halves_in_order = [0 if x["down"] else 1 for x in b]
    assert halves_in_order[0] == first and halves_in_order == sorted(halves_in_order, reverse=bool(first))


def test_committed_counter_figures_name_the_kernel_sources_they_were_measured_on():
    """profiles/pmc_traffic.json carries the hash of the kernel sources it was measured on (tools/pmc_summary.py,
    wafer_amd/provenance.py); bench.py's roofline.traffic is labelled stale when the kernels have changed since"""
    import importlib.util
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from wafer_amd import provenance
    doc = json.load(open(os.path.join(root, "profiles", "pmc_traffic.json")))
    assert len(doc["kernel_sources_sha16"]) == 16
    files = [os.path.basename(f) for f in provenance.kernel_sources()]
    assert "wafer_stencil_fused3.hip.h" in files and "wafer_tu_fused3.hip" in files and "wafer_engine.hip" not in files
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    traffic, key, stale = bench.pmc_traffic("wafer_k_step3_fused<double, double, true, 0, true, 1>")
    assert traffic > 3e9 and key.startswith("void wafer_k_step3_fused<double, double, true, 0, true, 1>(")
    assert stale == (doc["kernel_sources_sha16"] != provenance.kernel_sources_sha16())
    assert bench.pmc_traffic("wafer_k_step3_fused") == (None, None, None)          # a family name matches nothing


# ---- which pass of wafer_evolve comes next (wafer_passes.h) -----------------------------------------------------------------
PASSES = r"""
#include "wafer_passes.h"
#include <cstdio>
#include <cstdlib>
// plays whole calls: asks the planner until the steps are done, feeding every pass's "valid after" back in.  One line per call:
//   wnum steps R G cycle sched decomposed kernels x2 one_pass fused start | kind:steps:need:rendezvous:extend:exchange:valid_after:first:last ... ("D": a drain)
// argv: 0 (ground state) or 1 (excited states).  kernels: 0 neither fused kernel applies, 1 the two-step one, 2 both.
static bool possible(const WaferPassFacts &f)
{
    // what fuse2_applies / fuse3_applies / x2_applies never report: a slab with fewer ghost planes than a pass consumes, the three-step
    // kernel without the two-step one or off ThreePoint, two steps per pass without the one-pass kernel it starts from
    if (f.fuse3 && (f.R != 1 || !f.fuse2)) return false;
    if (f.decomposed && ((f.fuse2 && f.G < 2 * f.R) || (f.fuse3 && f.G < 3 * f.R))) return false;
    if (f.x2 && (f.R != 1 || f.wnum > 3 || !f.one_pass || !f.excited_fused || (f.decomposed && f.G < 2))) return false;
    return true;
}
static int play(const WaferPassFacts &f, int kernels, uint64_t steps_asked, int start)
{
    const uint64_t steps = steps_asked == 0 ? 1 : steps_asked;
    printf("%u %llu %d %d %d %d %d %d %d %d %d %d |", f.wnum, (unsigned long long)steps_asked, f.R, f.G, f.halo_cycle, f.sched, (int)f.decomposed, kernels,
           (int)f.x2, (int)f.one_pass, (int)f.excited_fused, start);
    int valid = start, depth = 0;
    bool in_flight = false;
    for (uint64_t s = 0; s < steps;) {
        WaferPass p = wafer_next_pass(f, s, steps, valid, in_flight);
        if (p.drain_first) {
            if (!in_flight) return 1;   // a drain with nothing in flight
            printf(" D");
            valid = depth;
            in_flight = false;
            continue;
        }
        printf(" %d:%llu:%d:%d:%d:%d:%d:%d:%d", p.kind, (unsigned long long)p.steps, p.need, (int)p.rendezvous, p.extend, p.exchange, p.valid_after,
               (int)p.first, (int)p.last);
        if (p.steps == 0) return 2;
        in_flight = p.kind == WAFER_PASS_HALVES || p.kind == WAFER_PASS_PEER;
        if (in_flight) depth = p.exchange;
        valid = p.valid_after;
        s += p.steps;
    }
    if (in_flight) printf(" D");
    printf("\n");
    return 0;
}
int main(int argc, char **argv)
{
    const bool excited = argc > 1 && atoi(argv[1]) != 0;
    const uint64_t counts[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 20, 21, 100, 101, 1000};
    for (uint64_t steps : counts)
        for (int R = 1; R <= 3; ++R)
            for (int G = R; G <= 9 * R; ++G)
                for (int sched = 0; sched <= 3; ++sched)
                    for (int dec = 0; dec <= 1; ++dec) {
                        WaferPassFacts f;
                        f.R = R; f.G = G; f.sched = sched; f.decomposed = dec != 0;
                        if (!excited) {
                            for (int cycle = 1; cycle <= 3; ++cycle)
                                for (int kernels = 0; kernels <= 2; ++kernels)
                                    for (int start : {0, G}) {
                                        f.halo_cycle = cycle; f.fuse2 = kernels >= 1; f.fuse3 = kernels == 2;
                                        if (!possible(f) || (start && !dec)) continue;
                                        if (int rc = play(f, kernels, steps, start)) return rc;
                                    }
                            continue;
                        }
                        if (G != R && G != 2 * R && G != 9 * R) continue;   // (the excited-state passes look at G only through `possible`)
                        for (uint32_t wnum = 1; wnum <= 5; ++wnum)
                            for (int bits = 0; bits < 8; ++bits) {
                                f.wnum = wnum; f.x2 = bits & 1; f.one_pass = bits & 2; f.excited_fused = bits & 4;
                                f.fuse2 = f.fuse3 = R == 1 && (!dec || G >= 3);   // the ground-state kernels apply or not: nothing an excited-state call may look at
                                if (!possible(f)) continue;
                                if (int rc = play(f, f.fuse3 ? 2 : 0, steps, 0)) return rc;
                            }
                    }
    return 0;
}
"""
HALVES, PEER, FUSED, STEP, EXCITED, EXCITED_ROWS, X2_TAIL = range(7)


@pytest.fixture(scope="module")
def played(tmp_path_factory):
    d = tmp_path_factory.mktemp("passes")
    src, exe = d / "passes.cpp", d / "passes"
    src.write_text(PASSES)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    keys = ("wnum", "steps", "R", "G", "cycle", "sched", "decomposed", "kernels", "x2", "one_pass", "fused", "start")
    pkeys = ("kind", "steps", "need", "rendezvous", "extend", "exchange", "valid_after", "first", "last")

    def calls(excited):
        out = subprocess.run([str(exe), str(int(excited))], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
        for line in out.stdout.splitlines():
            head, _, tail = line.partition("|")
            facts = dict(zip(keys, (int(x) for x in head.split())))
            yield facts, ["D" if t == "D" else dict(zip(pkeys, (int(x) for x in t.split(":")))) for t in tail.split()]
    return {0: list(calls(False)), 1: list(calls(True))}


def test_planner_passes_of_whole_calls(played):
    """wafer_passes.h against statements read off wafer_evolve: the steps add up, every pass of a slab finds the ghost planes it
    consumes, three steps per pass while three remain, deep halos exchange once per cycle, a single-launch sequence is drained
    before anything else, two excited-state steps per pass only behind their head"""
    ncalls = 0
    for f, seq in played[0] + played[1]:
        ncalls += 1
        R, G, dec, steps = f["R"], f["G"], f["decomposed"], max(1, f["steps"])
        passes = [p for p in seq if p != "D"]
        # 1. the steps add up (grid.rs:682-685: a call of 0 steps advances one) and no pass advances none
        assert all(p["steps"] > 0 for p in passes) and sum(p["steps"] for p in passes) == steps, (f, seq)
        assert passes[0]["first"] and passes[-1]["last"] and not any(p["first"] for p in passes[1:]) and not any(p["last"] for p in passes[:-1])
        # 2. enough ghost planes before every pass of a slab, never more than the slab has
        valid, depth, in_flight, prev = f["start"], 0, False, None
        for p in seq:
            if p == "D":
                # 5. a drain is reported only with a sequence in flight, and leaves the sequence's exchange depth
                assert in_flight, (f, seq)
                valid, in_flight, prev = depth, False, p
                continue
            single = p["kind"] in (HALVES, PEER)
            per_pass = 2 if p["kind"] == X2_TAIL else p["steps"]
            if dec:
                assert max(valid, p["need"]) >= per_pass * R + p["extend"], (f, p, valid)
                assert p["valid_after"] <= G and p["exchange"] <= G and p["need"] <= G, (f, p)
            else:
                assert p["exchange"] == 0 and p["extend"] == 0 and not single, (f, p)
            # 5. single-launch kinds: schedules 2 / 3 of a slab, three steps, one exchange per pass; never left without a drain
            if single:
                assert dec and f["sched"] == (3 if p["kind"] == PEER else 2) and p["steps"] == 3 and p["exchange"] == 3 * R == p["need"], (f, p)
                assert p["rendezvous"] == (p["kind"] == PEER and not in_flight), (f, seq)   # the first peer pass of a sequence: always an exchange
                depth = p["exchange"]
            else:
                assert not in_flight and not p["rendezvous"], (f, seq)
            in_flight, valid, prev = single, p["valid_after"], p
        assert not in_flight, (f, seq)   # ... and before ev_stop
        if f["wnum"] == 0:
            # 3. three steps per pass exactly while the three-step kernel applies and three remain, then two, then one
            left = steps
            for p in passes:
                want = 3 if (f["kernels"] == 2 and left >= 3) else 2 if (f["kernels"] >= 1 and left >= 2) else 1
                assert p["steps"] == want and (p["kind"] in (HALVES, PEER, FUSED) if want > 1 else p["kind"] == STEP), (f, p, left)
                left -= want
            # 4. deep halos: one exchange per min(cycle, G / (K R)) passes, and exactly the passes without one compute beyond the slab
            if dec:
                for p in passes:
                    if p["kind"] == FUSED:
                        assert (p["exchange"] == 0) == (p["extend"] > 0), (f, p)
                    else:
                        assert p["extend"] == 0 and p["exchange"] > 0, (f, p)
            K = passes[0]["steps"]
            if dec and f["sched"] in (0, 1) and K > 1 and G >= 2 * K * R and f["start"] == 0:
                every = min(f["cycle"], G // (K * R))
                stretch = [p for p in passes if p["steps"] == K]   # (the first stretch of the call: K never grows again)
                for i, p in enumerate(stretch, 1):
                    assert (p["exchange"] > 0) == (i % every == 0), (f, i, every, seq)
                    if p["exchange"]:
                        assert p["exchange"] == every * K * R, (f, p)
        else:
            # 6. two steps per pass: a head of 2 + (steps & 1) single steps, then ONE pass with the (even) rest; never below four steps
            tails = [i for i, p in enumerate(passes) if p["kind"] == X2_TAIL]
            if f["x2"] and steps >= 4:
                head = 2 + (steps & 1)
                assert tails == [head] and len(passes) == head + 1, (f, seq)
                assert all(p["steps"] == 1 for p in passes[:head]) and passes[head]["steps"] == steps - head and passes[head]["steps"] % 2 == 0
                assert passes[head]["valid_after"] == 0
            else:
                assert not tails and len(passes) == steps, (f, seq)
            for p in passes:
                if p["kind"] != X2_TAIL:
                    assert p["kind"] == (EXCITED if f["fused"] else EXCITED_ROWS) and p["need"] == R, (f, p)
                    # the last step of the one-pass scheme materialises phi and exchanges nothing
                    quiet = p["kind"] == EXCITED and f["one_pass"] and p["last"]
                    assert p["valid_after"] == (0 if quiet else R) and p["exchange"] == (0 if quiet or not dec else R), (f, p)
    assert ncalls > 50000


def test_planner_known_calls(played):
    """the remainder bench.py's driver form leaves (20 = 6 x 3 + 2) and the calls tools/path_bench.py times"""
    def ground(steps, kernels, **kw):
        want = dict(wnum=0, steps=steps, R=1, G=3, cycle=1, sched=0, decomposed=0, kernels=kernels, start=0)
        want.update(kw)
        hits = [seq for f, seq in played[0] if all(f[k] == v for k, v in want.items())]
        assert len(hits) == 1
        return [(p["kind"], p["steps"]) for p in hits[0] if p != "D"]
    assert ground(20, 2) == [(FUSED, 3)] * 6 + [(FUSED, 2)]
    assert ground(4, 2) == [(FUSED, 3), (STEP, 1)]
    assert ground(5, 1) == [(FUSED, 2)] * 2 + [(STEP, 1)]
    assert ground(3, 0) == [(STEP, 1)] * 3
    # a slab under the single launch: three-step passes in one sequence, drained before the two-step remainder
    hits = [seq for f, seq in played[0] if f == dict(wnum=0, steps=8, R=1, G=3, cycle=1, sched=2, decomposed=1, kernels=2, x2=0, one_pass=1, fused=0, start=0)]
    assert len(hits) == 1 and [p if p == "D" else (p["kind"], p["steps"]) for p in hits[0]] == [(HALVES, 3), (HALVES, 3), "D", (FUSED, 2)]
