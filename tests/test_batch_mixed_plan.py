"""The workgroup tables and the layout of a batch of several shapes (wafer_batch_step_table, wafer_batch_fused_table,
wafer_batch_layout, wafer_amd/csrc/wafer_batch_plan.h), compiled with g++ and the sanitizers as tests/test_batch_plan.py does.  No GPU."""
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wafer_amd", "csrc")

# table kind R K cus mask nx,ny,nz ... -> "G gz TX TY", one "nx ny nz shape" line per member, "--", then one line per entry
# kind: step (the one-step kernel's 64 x 4 tiles; K ignored), fused (64 x 12);
# layout (K, cus ignored, mask for the member count): after "--" one "off total" line per member, then "cells"
DRIVER = r"""
#include "wafer_batch_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
int main(int argc, char **argv)
{
    if (argc < 7) return 2;
    const char *kind = argv[1];
    const int R = atoi(argv[2]), K = atoi(argv[3]), cus = atoi(argv[4]);
    const char *mask = argv[5];
    const uint32_t n = (uint32_t)strlen(mask);
    if ((uint32_t)(argc - 6) != n) return 2;
    std::vector<uint8_t> active(n);
    for (uint32_t m = 0; m < n; ++m) active[m] = mask[m] == '1';
    std::vector<int> nxyz(3 * n);
    for (uint32_t m = 0; m < n; ++m)
        if (sscanf(argv[6 + m], "%d,%d,%d", &nxyz[3 * m], &nxyz[3 * m + 1], &nxyz[3 * m + 2]) != 3) return 2;
    const WaferBatchLayout L = wafer_batch_layout(nxyz.data(), n, R, R, 8);   // the engine's
    if (L.overflow) return 4;
    const std::vector<WaferGeom> &geoms = L.geoms;
    const std::vector<int> &shape_of = L.shape_of;
    const bool step = !strcmp(kind, "step");
    const int TX = step ? 64 : WAFER_BATCHK_TX, TY = step ? 4 : WAFER_BATCHK_TY;
    printf("%d %d %d %d\n", geoms[0].G, geoms[0].gz, TX, TY);
    for (uint32_t m = 0; m < n; ++m) printf("%d %d %d %d\n", geoms[shape_of[m]].nx, geoms[shape_of[m]].ny, geoms[shape_of[m]].nz, shape_of[m]);
    printf("--\n");
    if (!strcmp(kind, "layout")) {
        for (uint32_t m = 0; m < n; ++m) printf("%zu %lld\n", L.off[m], geoms[shape_of[m]].total);
        printf("%zu\n", L.cells);
        return 0;
    }
    std::vector<WaferBatchBlock> t;
    if (step) t = wafer_batch_step_table(geoms.data(), shape_of.data(), active.data(), n, cus, TX, TY);
    else if (!strcmp(kind, "fused")) t = wafer_batch_fused_table(geoms.data(), shape_of.data(), active.data(), n, cus, K, TX, TY);
    else return 2;
    for (const WaferBatchBlock &b : t) printf("%d %d %d %d %d %d\n", b.member, b.x0, b.y0, b.z0, b.z1, b.shape);
    // a null active set is every member
    std::vector<uint8_t> ones(n, 1);
    if (step && wafer_batch_step_table(geoms.data(), shape_of.data(), nullptr, n, cus, TX, TY).size() !=
                    wafer_batch_step_table(geoms.data(), shape_of.data(), ones.data(), n, cus, TX, TY).size()) return 3;
    if (!strcmp(kind, "fused") && wafer_batch_fused_table(geoms.data(), shape_of.data(), nullptr, n, cus, K, TX, TY).size() !=
                                      wafer_batch_fused_table(geoms.data(), shape_of.data(), ones.data(), n, cus, K, TX, TY).size()) return 3;
    return 0;
}
"""

MIXED = [(50, 50, 50), (64, 64, 64), (37, 50, 23), (130, 6, 5), (8, 8, 8), (65, 13, 3)]
UNIFORM = [(37, 50, 23)] * 6
MASKS = {"all": "111111", "one": "000100", "none": "000000", "alternating": "101010"}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_mixed_plan")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(DRIVER)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I", CSRC,
                        str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

    def call(kind, R, K, cus, mask, shapes):
        out = subprocess.run([str(exe), kind, str(R), str(K), str(cus), mask, *["%d,%d,%d" % s for s in shapes]],
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (kind, R, K, cus, mask, out.stderr[-2000:])
        lines = out.stdout.splitlines()
        G, gz, TX, TY = [int(x) for x in lines[0].split()]
        sep = lines.index("--")
        members = [tuple(int(x) for x in l.split()) for l in lines[1:sep]]
        entries = [tuple(int(x) for x in l.split()) for l in lines[sep + 1:]]
        return (G, gz, TX, TY), members, entries
    return call


def check_cover(head, members, entries, mask, R, K, fused):
    """the properties every table must have, whatever the shapes"""
    G, gz, TX, TY = head
    active = [m for m, c in enumerate(mask) if c == "1"]
    if not active:
        assert entries == []   # a frozen member costs nothing
        return
    count = {m: np.zeros(members[m][2::-1], dtype=np.int32) for m in active}   # [nz][ny][nx]
    for member, x0, y0, z0, z1, shape in entries:
        assert member in count, member                          # no entry names an inactive member
        nx, ny, nz, sh = members[member]
        assert shape == sh, (member, shape, sh)                 # the entry's shape index is its member's
        assert z1 > z0, "an empty chunk"
        assert x0 % TX == 0 and y0 % TY == 0 and 0 <= x0 < nx and 0 <= y0 < ny   # inside the member's OWN nx, ny
        assert G <= z0 and z1 <= G + nz                         # output planes are the member's work planes
        if fused:
            lz = nz + 2 * G
            # every plane the entry loads, [z0 - K R, z1 + K R), lies in that member's [-gz, lz + gz)
            assert z0 - K * R >= -gz and z1 + K * R <= lz + gz, (member, z0, z1)
            assert z1 - z0 >= min(nz, 4 * R * (K - 1)), (member, z0, z1)
        count[member][z0 - G:z1 - G, y0:y0 + TY, x0:x0 + TX] += 1
    for m in active:   # every work cell of every active member is the output of exactly one entry
        assert np.all(count[m] == 1), m
    # members in order, a member's entries together
    order = [e[0] for e in entries]
    assert order == sorted(order)


def todays_build_blocks(shape, R, mask, cus):
    """wafer_engine_batch.hip's build_blocks as it stood for one shape (G = R, nzl = nz), restated"""
    nx, ny, nz = shape
    G = R
    ntx, nty = (nx + 63) // 64, (ny + 3) // 4
    nact = mask.count("1")
    layer = nact * ntx * nty
    target = 8 * cus
    nch = (target + layer - 1) // layer if layer > 0 else 1
    nch = max(1, min(nch, (nz + 7) // 8))
    zchunk = (nz + nch - 1) // nch
    out = []
    for m, c in enumerate(mask):
        if c != "1":
            continue
        for z0 in range(G, G + nz, zchunk):
            for ty in range(nty):
                for tx in range(ntx):
                    out.append((m, tx * 64, ty * 4, z0, min(z0 + zchunk, G + nz), 0))
    return out


def one_shape_fused_table(shape, R, K, mask, cus):
    """the fused pass's table as it stood for one shape (G = R, nzl = nz), restated: the layer is nact ntx nty, the chunk count
    wafer_batch_fused_nchunks's rule, chunk i is [G + i nz / n, G + (i + 1) nz / n)"""
    nx, ny, nz = shape
    G = R
    ntx, nty = (nx + 63) // 64, (ny + 11) // 12
    layer = mask.count("1") * ntx * nty
    if layer == 0 or nz < 1:
        return []
    min_chunk = max(4 * R * (K - 1), 1)
    nch = max(1, min((2 * max(cus, 1) + layer - 1) // layer, max(nz // min_chunk, 1)))
    out = []
    for m, c in enumerate(mask):
        if c != "1":
            continue
        for i in range(nch):
            for ty in range(nty):
                for tx in range(ntx):
                    out.append((m, tx * 64, ty * 12, G + i * nz // nch, G + (i + 1) * nz // nch, 0))
    return out


@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("shapes", [MIXED, UNIFORM], ids=["mixed", "uniform"])
def test_step_table(plan, shapes, R):
    for (name, mask), cus in itertools.product(MASKS.items(), (1, 256)):
        head, members, entries = plan("step", R, 1, cus, mask, shapes)
        assert [m[:3] for m in members] == list(shapes)
        assert [m[3] for m in members] == ([0] * 6 if shapes is UNIFORM else list(range(6)))
        check_cover(head, members, entries, mask, R, 1, fused=False)
        if shapes is UNIFORM:
            assert entries == todays_build_blocks(shapes[0], R, mask, cus), (name, cus)
        else:
            # the rule: one layer summed over the active members' own tiles; per member its own chunk count
            layer = sum(((s[0] + 63) // 64) * ((s[1] + 3) // 4) for s, c in zip(shapes, mask) if c == "1")
            for m, (s, c) in enumerate(zip(shapes, mask)):
                if c != "1":
                    continue
                nch = max(1, min((8 * cus + layer - 1) // layer, (s[2] + 7) // 8))
                zchunk = (s[2] + nch - 1) // nch
                z = sorted({(e[3], e[4]) for e in entries if e[0] == m})
                assert z == [(R + z0, min(R + z0 + zchunk, R + s[2])) for z0 in range(0, s[2], zchunk)], (name, cus, m)


@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("shapes", [MIXED, UNIFORM], ids=["mixed", "uniform"])
def test_fused_table(plan, shapes, R):
    for (name, mask), cus, K in itertools.product(MASKS.items(), (1, 256), (2, 3)):
        head, members, entries = plan("fused", R, K, cus, mask, shapes)
        check_cover(head, members, entries, mask, R, K, fused=True)
        if shapes is UNIFORM:
            one = one_shape_fused_table(shapes[0], R, K, mask, cus)
            assert entries == one, (name, cus, K)   # the one-shape rule, entry for entry
        else:
            # chunk i of a member is [i nz / n, (i + 1) nz / n) for its own n
            for m, (s, c) in enumerate(zip(shapes, mask)):
                z = sorted({(e[3], e[4]) for e in entries if e[0] == m})
                if c != "1":
                    assert z == []
                    continue
                n = len(z)
                assert z == [(R + i * s[2] // n, R + (i + 1) * s[2] // n) for i in range(n)], (name, cus, K, m)


REPEATS = [MIXED[0], MIXED[2], MIXED[0], MIXED[3], MIXED[2]]   # shapes A, B, A, C, B


@pytest.mark.parametrize("R", [1, 2, 3])
def test_layout(plan, R):
    """wafer_batch_layout: shapes numbered in order of first appearance, members at the prefix sums of their padded totals"""
    for shapes in (MIXED, REPEATS, UNIFORM):
        _, members, lines = plan("layout", R, 1, 1, "1" * len(shapes), shapes)
        assert [m[:3] for m in members] == list(shapes)
        first = list(dict.fromkeys(shapes))   # the distinct shapes in order of first appearance
        numbers = [m[3] for m in members]
        assert numbers == [first.index(s) for s in shapes]
        if shapes is REPEATS:
            assert numbers == [0, 1, 0, 2, 1]
        off, totals = [l[0] for l in lines[:-1]], [l[1] for l in lines[:-1]]
        assert len(off) == len(shapes) and all(t > 0 for t in totals)
        assert len(set(zip(numbers, totals))) == len(first)   # one geometry, so one padded total, per distinct shape
        assert off == [sum(totals[:m]) for m in range(len(shapes))]
        assert lines[-1] == (sum(totals),)
        if shapes is UNIFORM:
            assert off == [m * totals[0] for m in range(len(shapes))]   # m * geoms[0].total


# ---- members that share shapes: the list the GPU tests of tests/test_gpu_batch_mixed_shared.py run ----------------------------------
from tests.test_gpu_batch_mixed_shared import SHAPE_LIST as SHARED, first_appearance, masks as shared_masks  # noqa: E402


def step_chunks(s, layer, R, cus):
    """wafer_batch_step_table's z-chunks of a member of shape s when the launch's layer is `layer`"""
    nch = max(1, min((8 * cus + layer - 1) // layer, (s[2] + 7) // 8))
    zchunk = (s[2] + nch - 1) // nch
    return [(R + z0, min(R + z0 + zchunk, R + s[2])) for z0 in range(0, s[2], zchunk)]


def fused_chunks(s, layer, R, K, cus):
    """wafer_batch_fused_table's"""
    nch = max(1, min((2 * max(cus, 1) + layer - 1) // layer, max(s[2] // max(4 * R * (K - 1), 1), 1)))
    return [(R + i * s[2] // nch, R + (i + 1) * s[2] // nch) for i in range(nch)]


@pytest.mark.parametrize("R", [1, 2, 3])
def test_shared_shapes_keep_member_and_shape_indexing_apart(plan, R):
    """The inputs of the GPU tests discriminate: with them the shape index is not the member index, a member's offset is not its
    shape's, every table entry carries shape_of[its member], and under the masks that empty a shape the tables hold the active
    members only, cut by the layer of the active members only."""
    for shapes in (SHARED, SHARED[::-1]):
        n = len(shapes)
        table, shape_of = first_appearance(shapes)
        assert 1 < len(table) < n and sum(1 for m in range(n) if shape_of[m] != m) > n // 2
        _, members, lines = plan("layout", R, 1, 1, "1" * n, shapes)
        assert [m[:3] for m in members] == list(shapes)
        assert [m[3] for m in members] == shape_of                       # first-appearance order
        off, totals = [l[0] for l in lines[:-1]], [l[1] for l in lines[:-1]]
        assert off == [sum(totals[:m]) for m in range(n)]               # the prefix sum over MEMBERS
        assert lines[-1] == (sum(totals),)
        total_of_shape = {shape_of[m]: totals[m] for m in range(n)}
        by_shape = [sum(total_of_shape[k] for k in range(shape_of[m])) for m in range(n)]   # ... which the one over the table is not
        assert sum(1 for m in range(n) if off[m] != by_shape[m]) > n // 2, (off, by_shape)
        assert len(set(off)) == n                                        # members of one shape lie apart
    shapes, n = SHARED, len(SHARED)
    _, shape_of = first_appearance(shapes)
    every = {"all": [1] * n}
    every.update(shared_masks(shapes))
    seen_by_layer = set()   # the masks whose tables differ from the ones the layer of ALL members would give
    for kind, K, tx, ty in (("step", 1, 64, 4), ("fused", 2, 64, 12), ("fused", 3, 64, 12)):
        if kind == "fused" and K * R > 6:
            continue
        for (name, mask), cus in itertools.product(every.items(), (1, 4, 20, 32, 256)):
            bits = "".join(str(a) for a in mask)
            head, members, entries = plan(kind, R, K, cus, bits, shapes)
            check_cover(head, members, entries, bits, R, K, fused=(kind == "fused"))
            assert all(e[5] == shape_of[e[0]] for e in entries), (kind, name)            # shape == shape_of[entry.member]
            assert any(e[5] != e[0] for e in entries), (kind, name)                        # ... and that is not the member
            assert {e[0] for e in entries} == {m for m in range(n) if mask[m]}, (kind, name)   # no frozen member, every active one
            tiles = lambda s: ((s[0] + tx - 1) // tx) * ((s[1] + ty - 1) // ty)   # noqa: E731
            layer = sum(tiles(s) for s, a in zip(shapes, mask) if a)
            layer_all = sum(tiles(s) for s in shapes)
            for m in range(n):
                if not mask[m]:
                    continue
                chunks = (lambda l: step_chunks(shapes[m], l, R, cus)) if kind == "step" else (lambda l: fused_chunks(shapes[m], l, R, K, cus))
                z = sorted({(e[3], e[4]) for e in entries if e[0] == m})
                assert z == chunks(layer), (kind, K, name, cus, m)       # the summed layer is the active members'
                assert len([e for e in entries if e[0] == m]) == len(z) * tiles(shapes[m])
                if chunks(layer) != chunks(layer_all):
                    seen_by_layer.add(name)
    # where an active member is thick enough to be cut at all, the active set's layer shows in its chunks: (130, 6, 5) alone -- mask
    # (c) -- is one chunk under every layer, and so are mask (d)'s (260, 5, 4) and (8, 8, 8) except in the ThreePoint two-step pass
    want = {k for k in every if k[:2] in (("a_", "b_", "d_") if R == 1 else ("a_", "b_"))}
    assert want <= seen_by_layer, seen_by_layer
