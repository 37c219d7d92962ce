"""The host-side plan of a batched ground-state evolve (wafer_amd/csrc/wafer_batch_plan.h), compiled with g++ and the
sanitizers: the pass sequence of a call and the workgroup table of the fused K-step pass.  No GPU."""
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wafer_amd", "csrc")

DRIVER = r"""
#include "wafer_batch_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
int main(int argc, char **argv)
{
    if (argc >= 5 && !strcmp(argv[1], "seq")) {   // seq steps K have2 -> "launches fused : k k k ..."
        const uint64_t steps = strtoull(argv[2], nullptr, 10);
        const int K = atoi(argv[3]);
        const bool have2 = atoi(argv[4]) != 0;
        uint64_t fused = 0;
        const uint64_t n = wafer_batch_launch_count(steps, K, have2, &fused);
        printf("%llu %llu :", (unsigned long long)n, (unsigned long long)fused);
        for (int k : wafer_batch_pass_sequence(steps, K, have2)) printf(" %d", k);
        printf("\n");
        return 0;
    }
    if (argc >= 10 && !strcmp(argv[1], "table")) {   // table nx ny nz R G K cus mask -> geometry line, then one line per entry
        const int nx = atoi(argv[2]), ny = atoi(argv[3]), nz = atoi(argv[4]), R = atoi(argv[5]), G = atoi(argv[6]), K = atoi(argv[7]);
        const int cus = atoi(argv[8]);
        const char *mask = argv[9];
        const uint32_t n = (uint32_t)strlen(mask);
        std::vector<uint8_t> active(n);
        for (uint32_t m = 0; m < n; ++m) active[m] = mask[m] == '1';
        std::vector<int> nxyz;
        for (uint32_t m = 0; m < n; ++m) nxyz.insert(nxyz.end(), {nx, ny, nz});
        const WaferBatchLayout L = wafer_batch_layout(nxyz.data(), n, R, G, 8);   // one geometry, shape_of all zero
        if (L.overflow || L.geoms.size() != 1) return 4;
        const WaferGeom &g = L.geoms[0];
        printf("%d %d %d %d %d %d\n", g.G, g.nzl, g.lz, g.gz, WAFER_BATCHK_TX, WAFER_BATCHK_TY);
        for (const WaferBatchBlock &b : wafer_batch_fused_table(&g, L.shape_of.data(), active.data(), n, cus, K, WAFER_BATCHK_TX, WAFER_BATCHK_TY))
            printf("%d %d %d %d %d\n", b.member, b.x0, b.y0, b.z0, b.z1);
        // a null active set is every member
        const size_t all = wafer_batch_fused_table(&g, L.shape_of.data(), nullptr, n, cus, K, WAFER_BATCHK_TX, WAFER_BATCHK_TY).size();
        std::vector<uint8_t> ones(n, 1);
        if (all != wafer_batch_fused_table(&g, L.shape_of.data(), ones.data(), n, cus, K, WAFER_BATCHK_TX, WAFER_BATCHK_TY).size()) return 3;
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "cells")) {   // cells R K -> "lx ly" of every cell of the level-0 region, in order
        const int R = atoi(argv[2]), K = atoi(argv[3]);
        const int n = (WAFER_BATCHK_TX + 2 * K * R) * (WAFER_BATCHK_TY + 2 * K * R);
        printf("%d %d\n", WAFER_BATCHK_TX, WAFER_BATCHK_TY);
        for (int c = 0; c < n; ++c) {
            int lx = -1, ly = -1;
            wafer_batchk_cell(R, K, c, lx, ly);
            printf("%d %d\n", lx, ly);
        }
        return 0;
    }
    return 2;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_plan")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(DRIVER)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I", CSRC,
                        str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

    def call(*args):
        out = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (args, out.stderr[-2000:])
        return out.stdout
    return call


def expected_sequence(steps, K, have2):
    """the issue's statement of it: passes of K while at least K remain, then a two-step pass if there is one, then single steps"""
    left, seq = max(steps, 1), []
    while K > 1 and left >= K:
        seq.append(K)
        left -= K
    while have2 and left >= 2:
        seq.append(2)
        left -= 2
    seq += [1] * left
    return seq


@pytest.mark.parametrize("K,have2", [(3, True), (3, False), (2, False), (2, True), (1, False), (1, True)])
def test_pass_sequence(plan, K, have2):
    for steps in list(range(0, 21)) + [1000]:
        head, _, tail = plan("seq", steps, K, int(have2)).partition(":")
        launches, fused = [int(x) for x in head.split()]
        seq = [int(x) for x in tail.split()]
        assert seq == expected_sequence(steps, K, have2), (steps, K, have2, seq)
        assert sum(seq) == max(steps, 1)
        assert all(k >= 1 for k in seq)
        left = max(steps, 1)
        for k in seq:   # no fused pass is started with fewer steps left than it takes
            assert k <= left and k in (1, 2, K)
            left -= k
        # the engine flips `cur` by the parity of this count: it is the number of launches of the sequence
        assert launches == len(seq) and launches % 2 == len(seq) % 2
        assert fused == sum(1 for k in seq if k > 1)


SHAPES = [(50, 50, 50), (64, 64, 64), (37, 50, 23), (130, 70, 40), (5, 4, 3), (1, 1, 1), (64, 64, 2)]
MASKS = {"all": "111111", "one": "000100", "none": "000000", "alternating": "101010"}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("R", [1, 2, 3])
def test_fused_table(plan, shape, R):
    nx, ny, nz = shape
    for (name, mask), cus, K, G in itertools.product(MASKS.items(), (1, 256), (2, 3), (R, R + 2)):
        lines = plan("table", nx, ny, nz, R, G, K, cus, mask).splitlines()
        g_G, nzl, lz, gz, TX, TY = [int(x) for x in lines[0].split()]
        assert (g_G, nzl, lz, gz) == (G, nz, nz + 2 * G, 3 * R)
        entries = [tuple(int(x) for x in l.split()) for l in lines[1:]]
        active = [m for m, c in enumerate(mask) if c == "1"]
        if not active:
            assert entries == [], name   # a frozen member costs nothing
            continue
        count = {m: np.zeros((nz, ny, nx), dtype=np.int32) for m in active}
        for member, x0, y0, z0, z1 in entries:
            assert member in count, (name, member)            # no entry names an inactive member
            assert z1 > z0, "an empty chunk"
            assert x0 % TX == 0 and y0 % TY == 0 and 0 <= x0 < nx and 0 <= y0 < ny
            assert G <= z0 and z1 <= G + nzl                   # output planes are work planes
            # every plane the entry loads, [z0 - K R, z1 + K R), lies inside the allocation [-gz, lz + gz)
            assert z0 - K * R >= -gz and z1 + K * R <= lz + gz, (shape, R, K, G, z0, z1)
            count[member][z0 - G:z1 - G, y0:y0 + TY, x0:x0 + TX] += 1
        for m in active:   # every work cell is the output of exactly one entry
            assert np.all(count[m] == 1), (shape, R, K, name, cus, m)
        # chunks of at least 4 R (K-1) planes -- the recomputed share R (K-1) / (L + R (K-1)) is at most 1/5 -- unless the grid
        # itself is thinner than that
        for member, x0, y0, z0, z1 in entries:
            assert z1 - z0 >= min(nz, 4 * R * (K - 1)), (shape, R, K, cus, z0, z1)


@pytest.mark.parametrize("R,K", [(1, 3), (1, 2), (2, 2), (3, 2), (2, 3)])
def test_fused_cell_order(plan, R, K):
    """every level's region is a prefix of the cell order, and the order is a bijection onto the level-0 region"""
    lines = plan("cells", R, K).splitlines()
    TX, TY = [int(x) for x in lines[0].split()]
    cells = [tuple(int(x) for x in l.split()) for l in lines[1:]]
    H = K * R
    W0, H0 = TX + 2 * H, TY + 2 * H
    assert len(cells) == W0 * H0 and len(set(cells)) == len(cells)
    assert all(0 <= lx < W0 and 0 <= ly < H0 for lx, ly in cells)
    for k in range(K + 1):   # level k: the tile grown by (K - k) R
        m = (K - k) * R
        n = (TX + 2 * m) * (TY + 2 * m)
        region = {(lx, ly) for lx in range(H - m, H + TX + m) for ly in range(H - m, H + TY + m)}
        assert set(cells[:n]) == region, (R, K, k)
    # the tile itself row by row: one wave across a 64-cell row
    assert cells[:TX * TY] == [(H + c % TX, H + c // TX) for c in range(TX * TY)]
