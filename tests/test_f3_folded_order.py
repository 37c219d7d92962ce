"""The folded tile order of the paired three-step pass (wafer_f3_schedule_plain with fold, wafer_stencil_fused3.hip.h), host code
compiled here and run without a device.

The paired pass gains only because the two tiles (tx, ty) and (tx, nty-1-ty) of a z-chunk run on the SAME XCD at the same time
and share V's lines in its L2.  The GPU tests compare bits, which any permutation of the tiles would also produce; this file
holds the order itself: every (tile, chunk) once, and partners at dispatch slots with equal b % 8 (workgroup b runs on XCD
b % 8), in the same launch where the table goes out as one launch per round of 256 CUs.

A pair is split only where an XCD's contiguous range of the sequence ends inside it: at most ntx pairs per range end, 7 * ntx
per table.  No pair is split at 512^3, 768^3, 1024^3, 1024 x 1024 x 128 and on the GPU tests' grids 128^3 and 128 x 144 x 120
(range ends fall between pairs of rows, or between chunks).  384^3 (72 tiles per layer, 7 chunks, ranges of 63) splits 12 of its
252 pairs; tables with fewer workgroups than two rows per XCD split most or all of theirs (SHAPES, last column)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wafer_amd", "csrc")

HARNESS = r"""
#include "wafer_stencil_fused3.hip.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv)
{
    std::vector<WaferF3Block> t;
    // ntx nty lo hi zchunk swz fold
    wafer_f3_schedule_plain(t, atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]) != 0, false, atoi(argv[7]) != 0);
    for (const auto &b : t) printf("%d %d %d %d %d %d\n", b.tile, b.zs, b.ze, b.down, b.wait_late, b.bump);
    return 0;
}
"""


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("fold")
    src, exe = d / "fold.hip", d / "fold"
    src.write_text(HARNESS)
    r = subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def call(ntx, nty, lo, hi, zc, swz, fold):
        out = subprocess.run([str(exe), *[str(a) for a in (ntx, nty, lo, hi, zc, swz, fold)]], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr[-2000:]
        keys = ("tile", "zs", "ze", "down", "wait_late", "bump")
        return [dict(zip(keys, (int(x) for x in line.split()))) for line in out.stdout.splitlines()]
    return call


def folded_position(ty, nty):
    """where tile row ty stands in the order 0, nty-1, 1, nty-2, ... (stated from the row, the code states it from the position)"""
    return 2 * ty if ty < (nty + 1) // 2 else 2 * (nty - 1 - ty) + 1


# (ntx, nty, lo, hi, planes per workgroup, launch size or 0, pairs an XCD range end splits)
SHAPES = [
    (4, 32, 3, 515, 256, 0, 0),       # 512^3: 256 workgroups, ranges of 32 = 4 pairs of rows
    (8, 64, 3, 1027, 342, 256, 0),    # 1024^3: 3 chunks, 1536 workgroups in six launches of 256; ranges of 192 = 12 pairs of rows
    (6, 48, 3, 771, 256, 0, 0),       # 768^3: 864 workgroups, ranges of 108 = 9 pairs of rows
    (8, 64, 3, 131, 128, 0, 0),       # 1024 x 1024 x 128: 512 workgroups, ranges of 64
    (1, 8, 3, 131, 4, 0, 0),          # 128^3: 32 chunks of 8 tiles
    (1, 9, 3, 123, 5, 0, 0),          # 128 x 144 x 120: nty odd, the middle row alone; 24 chunks of 9: ranges of 27 end between chunks
    (3, 24, 3, 387, 55, 0, 12),       # 384^3: 7 chunks of 72, ranges of 63, not a multiple of 6: 12 of 252 pairs split
    (4, 9, 0, 40, 7, 0, 12),          # nty odd, ntx 4, 6 chunks: 12 of 96
    (4, 2, 0, 10, 10, 0, 4),          # one pair of rows, 8 workgroups: every XCD one tile -- all 4 pairs split, nothing can be shared
    (8, 3, 0, 30, 10, 0, 21),         # 72 workgroups, ranges of 9 against pairs of 16: 21 of 24
]


@pytest.mark.parametrize("ntx,nty,lo,hi,zc,launch,cuts", SHAPES)
def test_folded_order_keeps_partners_on_one_xcd(plain, ntx, nty, lo, hi, zc, launch, cuts):
    b = plain(ntx, nty, lo, hi, zc, 1, 1)
    ntiles, nch = ntx * nty, -(-(hi - lo) // zc)
    n = ntiles * nch
    assert len(b) == n and all(x["down"] == 0 and x["bump"] == -1 and x["wait_late"] == -1 for x in b)
    # every (tile, chunk) once, every plane of every tile once
    assert len({(x["tile"], x["zs"], x["ze"]) for x in b}) == n
    for t in range(ntiles):
        planes = sorted(p for x in b if x["tile"] == t for p in range(x["zs"], x["ze"]))
        assert planes == list(range(lo, hi)), t
    # position of each workgroup in the folded sequence: x fastest, folded rows, then chunks
    seq = [(x["zs"] - lo) // zc * ntiles + folded_position(x["tile"] // ntx, nty) * ntx + x["tile"] % ntx for x in b]
    assert sorted(seq) == list(range(n))
    # XCD k (slots k, k + 8, ...) works through one contiguous range of that sequence, in order
    ends = []
    for k in range(8):
        mine = seq[k::8]
        if mine:
            assert mine == list(range(mine[0], mine[0] + len(mine))), k
            ends.append(mine[-1])
    slot = {(x["tile"], x["zs"]): i for i, x in enumerate(b)}
    split = together = 0
    for c in range(nch):
        zs = lo + c * zc
        for ty in range(nty // 2):
            for tx in range(ntx):
                s0, s1 = slot[(ty * ntx + tx, zs)], slot[((nty - 1 - ty) * ntx + tx, zs)]
                p0 = c * ntiles + 2 * ty * ntx + tx               # the partner stands ntx further on
                assert seq[s0] == p0 and seq[s1] == p0 + ntx
                cut = any(p0 <= e < p0 + ntx for e in ends[:-1])  # an XCD's range ends between the two
                assert (s0 % 8 == s1 % 8) == (not cut), (c, tx, ty, s0, s1)
                if cut:
                    split += 1
                    continue
                together += 1
                assert s1 - s0 == 8 * ntx                         # ntx entries apart in that XCD's queue
                if launch:
                    assert s0 // launch == s1 // launch, (c, tx, ty, s0, s1)
    assert split <= 7 * ntx and split + together == nch * (nty // 2) * ntx
    assert split == cuts


@pytest.mark.parametrize("ntx,nty,lo,hi,zc", [(4, 32, 3, 515, 256), (1, 9, 3, 123, 5), (3, 24, 3, 387, 55)])
def test_fold_off_is_the_order_it_was(plain, ntx, nty, lo, hi, zc):
    """without fold: x fastest, then y, then chunk, cut into XCD ranges -- the default argument changes nothing"""
    b = plain(ntx, nty, lo, hi, zc, 1, 0)
    ids = [x["tile"] + (x["zs"] - lo) // zc * ntx * nty for x in b]
    for k in range(8):
        mine = ids[k::8]
        assert mine == list(range(mine[0], mine[0] + len(mine)))
    unswizzled = plain(ntx, nty, lo, hi, zc, 0, 1)
    assert [x["tile"] for x in unswizzled[:2 * ntx]] == list(range(ntx)) + [(nty - 1) * ntx + t for t in range(ntx)]
