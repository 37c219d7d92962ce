"""The Gram-Schmidt partition of a batch (wafer_batch_gs_partition, wafer_amd/csrc/wafer_batch_plan.h): every member's workgroup
count under the excited-state kernels and the places of its rows of partials, one shape or several -- compiled with g++ and the
sanitizers as tests/test_batch_mixed_plan.py does.  No GPU."""
import subprocess

import pytest

from tests.test_batch_mixed_plan import CSRC, MIXED, UNIFORM

TX, TY, ZC = 64, 4, 4              # WAFER_BATCH_TX, WAFER_BATCH_TY, WAFER_GS_ZC
ROWS = {"chain": 1, "sums": 5, "gram": 6}   # 1, WAFER_GS_ONE_ROWS = 1 + WAFER_MAX_LOW, WAFER_GRAM_PAIRS = WAFER_MAX_LOW (WAFER_MAX_LOW - 1) / 2

# R rows nx,ny,nz ... -> one "nb first row_off" line per member, then "blocks max_nb doubles"
DRIVER = r"""
#include "wafer_batch_plan.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const int R = atoi(argv[1]), rows = atoi(argv[2]);
    const uint32_t n = (uint32_t)(argc - 3);
    std::vector<int> nxyz(3 * n);
    for (uint32_t m = 0; m < n; ++m)
        if (sscanf(argv[3 + m], "%d,%d,%d", &nxyz[3 * m], &nxyz[3 * m + 1], &nxyz[3 * m + 2]) != 3) return 2;
    const WaferBatchLayout L = wafer_batch_layout(nxyz.data(), n, R, R, 8);   // the engine's
    if (L.overflow) return 4;
    const WaferBatchGsPartition P = wafer_batch_gs_partition(L.geoms.data(), L.shape_of.data(), n, 64, 4, 4);
    if (P.nb.size() != n || P.first.size() != n) return 3;
    for (uint32_t m = 0; m < n; ++m) {
        if (P.nb[m] != wafer_gs_blocks_of(L.geoms[L.shape_of[m]], 64, 4, 4)) return 3;
        printf("%d %lld %lld\n", P.nb[m], P.first[m], P.row_off(m, rows));
    }
    printf("%lld %d %lld\n", P.blocks, P.max_nb, P.doubles(rows));
    return 0;
}
"""


@pytest.fixture(scope="module")
def partition(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_mixed_states_plan")
    src, exe = d / "gsplan.cpp", d / "gsplan"
    src.write_text(DRIVER)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I", CSRC,
                        str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

    def call(R, rows, shapes):
        out = subprocess.run([str(exe), str(R), str(rows), *["%d,%d,%d" % s for s in shapes]], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (R, rows, shapes, out.stderr[-2000:])
        lines = [tuple(int(x) for x in l.split()) for l in out.stdout.splitlines()]
        return lines[:-1], lines[-1]
    return call


def gs_blocks(shape):
    """wafer_gs_blocks of the shape: tiles of 64 x 4 work cells, chunks of 4 planes -- fixed by the shape alone"""
    nx, ny, nz = shape
    return ((nx + TX - 1) // TX) * ((ny + TY - 1) // TY) * ((nz + ZC - 1) // ZC)


def test_the_six_shapes_have_the_partitions_the_gpu_tests_rely_on():
    nb = [gs_blocks(s) for s in MIXED]
    assert nb == [169, 256, 78, 12, 4, 8]   # (so a member of 4 workgroups lies beside one of 256: the early-leaving workgroups run)
    assert len(set(nb)) == len(nb)


@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("kind", sorted(ROWS))
@pytest.mark.parametrize("shapes", [MIXED, MIXED[::-1], UNIFORM, [MIXED[0], MIXED[5], MIXED[4], MIXED[0], MIXED[5]]],
                         ids=["mixed", "reversed", "uniform", "shared"])
def test_partition(partition, shapes, kind, R):
    rows = ROWS[kind]
    members, (blocks, max_nb, doubles) = partition(R, rows, shapes)
    n = len(shapes)
    nb = [m[0] for m in members]
    assert nb == [gs_blocks(s) for s in shapes]                              # every member's gs_nb is wafer_gs_blocks of ITS shape
    assert [m[1] for m in members] == [sum(nb[:m]) for m in range(n)]        # first: the prefix sums over MEMBERS
    assert [m[2] for m in members] == [rows * sum(nb[:m]) for m in range(n)]  # offsets: the prefix sums times the row count
    assert blocks == sum(nb) and max_nb == max(nb) and doubles == rows * sum(nb)   # totals
    # no two members' rows overlap, none passes the end: member m owns [row_off, row_off + rows * nb), row q at row_off + q * nb
    spans = sorted((m[2], m[2] + rows * m[0]) for m in members)
    assert spans[0][0] == 0 and spans[-1][1] == doubles
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))               # end to end: no gap either
    owner = {}
    for m, (b, _, off) in enumerate(members):
        for q in range(rows):
            for w in (0, b - 1):
                assert owner.setdefault(off + q * b + w, (m, q, w)) == (m, q, w)
    if len(set(shapes)) == 1:   # one shape: the records hold the closed forms a one-shape batch used to index by, member * rows * nb
        assert [m[1] for m in members] == [m * nb[0] for m in range(n)] and doubles == rows * n * nb[0]
        assert [m[2] for m in members] == [m * rows * nb[0] for m in range(n)]
        assert all(off + q * nb[0] == (m * rows + q) * nb[0] for m, (_, _, off) in enumerate(members) for q in range(rows))


def test_the_partition_does_not_depend_on_the_stencil_or_the_neighbours(partition):
    for R in (1, 2, 3):
        alone = [partition(R, 1, [s])[0][0][0] for s in MIXED]
        together = [m[0] for m in partition(R, 1, MIXED)[0]]
        assert alone == together == [gs_blocks(s) for s in MIXED]
