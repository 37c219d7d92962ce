"""The eight-wave tile roles of the fused stencil kernels (wafer_tile_roles.hip.h), expanded in a host function and run without a
device: who owns which row and which halo-column cell of a tile, where the requests go in global memory and in LDS, and the
XCD-aware order of the tiles.

The GPU tests compare bits end to end; a cell with two owners, or a redirected request that lands in another tile's lines, would
pass them (the same values, more traffic), and one that lands outside the allocation may pass them too.  This file holds the
assignment itself, for the three kernels' configurations, over every tile of whole, ragged and tiny grids.

The harness expands the SAME macros as the kernels, with each kernel's own parameters (the column a row offset is formed at, the
outer-row table, the levels a halo-column cell exists at): wafer_k_step3_fused, wafer_k_step2_wide, wafer_k_xstep2."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wafer_amd", "csrc")

HARNESS = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
using std::min;
#include "wafer_stencil_fused3.hip.h"
#include "wafer_stencil_fused2w.hip.h"
#include "wafer_stencil_x2.hip.h"

// one line per (wave, lane):
//   wave lane xl x_row inner | y wk off (RY times; off: of the lane's first cell) | xy xwk xy_out xoff | has_o oy oy_out ooff olds |
//   c_ok crow ckk clc cxw cy c_wk c_xout c_off c_lds0 c_l1 c_lds1 c_l2 c_lds2
#define EMIT_HEAD printf("%d %d %d %d %d", wave, lane, xl, (int)x_row, (int)(WAFER_TILE_INNER_ROW_WAVE))
#define EMIT_ROWS(LANE_)                                                                                           \
    for (int r = 0; r < RY; ++r) printf(" %d %d %lld", yrow[r], (int)rowwk[r], rowoff[r] + (LANE_));              \
    printf(" %d %d %d %lld", xy, (int)xwk, (int)xy_out, xoff_row + (LANE_))
#define EMIT_CELL printf(" %d %d %d %d %d %d %d %d %lld %d", (int)c_ok, crow, ckk, clc, cxw, cy, (int)c_wk, (int)c_xout, c_off, c_lds0)

template <typename T>
static void probe_f3(const WaferGeom &g, int x0, int y0, int wave, int lane)
{
    using Cfg = WaferF3Cfg<T>;
    constexpr int R = 1, VEC = Cfg::VEC, RY = Cfg::RY, TX = Cfg::TX, TY = Cfg::TY;
    constexpr int HX0 = Cfg::HX0, HX1 = Cfg::HX1, HX2 = Cfg::HX2, LP0 = Cfg::LP0, LP1 = Cfg::LP1, LP2 = Cfg::LP2;
    const bool x_row = WAFER_TILE_ROW_WAVE, has_orow = WAFER_TILE_OUTER_ROW_WAVE;
    const int xl = lane * VEC;
    WAFER_TILE_MAIN_ROWS(x0, )
    WAFER_TILE_HALO_ROW(x0);
    const int oy = WAFER_F3_OUTER_ROW_Y;
    const bool oy_out = WAFER_TILE_ROW_OUTSIDE(oy);
    const long long orow_off = WAFER_TILE_ROW_REQUEST(oy, oy_out, x0);
    const int orow_lds = WAFER_TILE_LDS0_ROW(oy);
    WAFER_TILE_CELL_HEAD;
    const bool c_l1 = WAFER_TILE_CELL_AT(1, 1), c_l2 = WAFER_TILE_CELL_AT(2, 2);
    WAFER_TILE_CELL_TAIL;
    const int c_lds0 = WAFER_TILE_CELL_LDS0, c_lds1 = WAFER_TILE_CELL_LDS(1), c_lds2 = WAFER_TILE_CELL_LDS(2);
    EMIT_HEAD;
    EMIT_ROWS(xl);   // (the lane's columns are added at the request)
    printf(" %d %d %d %lld %d", (int)has_orow, oy, (int)oy_out, orow_off + xl, orow_lds);
    EMIT_CELL;
    printf(" %d %d %d %d\n", (int)c_l1, c_lds1, (int)c_l2, c_lds2);
}

template <typename T>
static void probe_w2(const WaferGeom &g, int x0, int y0, int wave, int lane)
{
    using Cfg = WaferW2Cfg<T>;
    constexpr int R = 2, VEC = Cfg::VEC, RY = Cfg::RY, TX = Cfg::TX, TY = Cfg::TY;
    constexpr int HX0 = Cfg::HX0, HX1 = Cfg::HX1, LP0 = Cfg::LP0, LP1 = Cfg::LP1;
    const bool x_row = WAFER_TILE_ROW_WAVE;
    const int xl = lane * VEC, xi = x0 + xl;
    WAFER_TILE_MAIN_ROWS(xi, )
    WAFER_TILE_HALO_ROW(xi);
    const int oy = WAFER_W2_OUTER_ROW_Y;
    const bool oy_out = WAFER_TILE_ROW_OUTSIDE(oy);
    const long long orow_off = WAFER_TILE_ROW_REQUEST(oy, oy_out, xi);
    const int orow_lds = WAFER_TILE_LDS0_ROW(oy);
    WAFER_TILE_CELL_HEAD;
    const bool c_l1 = WAFER_TILE_CELL_AT(1, R);
    WAFER_TILE_CELL_TAIL;
    const int c_lds0 = WAFER_TILE_CELL_LDS0, c_lds1 = WAFER_TILE_CELL_LDS(1);
    EMIT_HEAD;
    EMIT_ROWS(0);   // (the lane's columns are folded into the offsets)
    printf(" %d %d %d %lld %d", (int)x_row, oy, (int)oy_out, orow_off, orow_lds);
    EMIT_CELL;
    printf(" %d %d 0 0\n", (int)c_l1, c_lds1);
}

template <int RY>
static void probe_x2(const WaferGeom &g, int x0, int y0, int wave, int lane)
{
    using Cfg = WaferX2Cfg<RY>;
    constexpr int R = 1, VEC = Cfg::VEC, TX = Cfg::TX, TY = Cfg::TY;
    constexpr int HX0 = Cfg::HX0, HX1 = Cfg::HX1, LP0 = Cfg::LP0, LP1 = Cfg::LP1;
    const bool x_row = WAFER_TILE_ROW_WAVE;
    const int xl = lane * VEC;
    int qoff[RY];
    WAFER_TILE_MAIN_ROWS(x0, qoff[r] = (wave * RY + r) * TX + xl)
    (void)qoff;
    WAFER_TILE_HALO_ROW(x0);
    WAFER_TILE_CELL_HEAD;
    const bool c_l1 = WAFER_TILE_CELL_AT(1, 2);
    WAFER_TILE_CELL_TAIL;
    const int c_lds0 = WAFER_TILE_CELL_LDS0, c_lds1 = WAFER_TILE_CELL_LDS(1);
    EMIT_HEAD;
    EMIT_ROWS(xl);
    printf(" 0 0 0 0 0");
    EMIT_CELL;
    printf(" %d %d 0 0\n", (int)c_l1, c_lds1);
}

template <class Cfg, typename F>
static void run(int R, int halo, int hc2, int rows2, int lp2, int hx2, int esize, int nx, int ny, int nz, F probe)
{
    const WaferGeom g = wafer_make_geom(nx, ny, nz, R, 3 * R, 0, nz, esize);
    const int ntx = (nx + Cfg::TX - 1) / Cfg::TX, nty = (ny + Cfg::TY - 1) / Cfg::TY;
    printf("C %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", R, halo, Cfg::VEC, Cfg::RY, Cfg::TX, Cfg::TY, Cfg::HC0, Cfg::HC1, hc2,
           Cfg::ROWS0, Cfg::ROWS1, rows2, Cfg::LP0, Cfg::LP1, lp2, Cfg::HX0, Cfg::HX1, hx2, Cfg::NCOL, Cfg::CPW);
    printf("G %d %d %d %d %d %d %lld %lld %lld %d %d\n", g.pitch, g.xoff, g.gy, g.py, g.gz, g.lz, g.plane, g.total, g.base_off, ntx, nty);
    for (int ty = 0; ty < nty; ++ty)
        for (int tx = 0; tx < ntx; ++tx) {
            printf("T %d %d\n", tx * Cfg::TX, ty * Cfg::TY);
            for (int wave = 0; wave < 8; ++wave)
                for (int lane = 0; lane < 64; ++lane) probe(g, tx * Cfg::TX, ty * Cfg::TY, wave, lane);
        }
}

int main(int argc, char **argv)
{
    if (!strcmp(argv[1], "xcd")) {
        for (int n = 1; n <= atoi(argv[2]); ++n) {
            for (int b = 0; b < n; ++b) printf("%d ", wafer_xcd_tile(b, n));
            printf("\n");
        }
        return 0;
    }
    const int nx = atoi(argv[2]), ny = atoi(argv[3]), nz = atoi(argv[4]);
    using F3d = WaferF3Cfg<double>;
    using F3f = WaferF3Cfg<float>;
    using W2d = WaferW2Cfg<double>;
    using W2f = WaferW2Cfg<float>;
    if (!strcmp(argv[1], "f3_f64")) run<F3d>(1, F3d::HALO, F3d::HC2, F3d::ROWS2, F3d::LP2, F3d::HX2, 8, nx, ny, nz, probe_f3<double>);
    else if (!strcmp(argv[1], "f3_f32")) run<F3f>(1, F3f::HALO, F3f::HC2, F3f::ROWS2, F3f::LP2, F3f::HX2, 4, nx, ny, nz, probe_f3<float>);
    else if (!strcmp(argv[1], "w2_f64")) run<W2d>(2, W2d::HALO, 0, 0, 0, 0, 8, nx, ny, nz, probe_w2<double>);
    else if (!strcmp(argv[1], "w2_f32")) run<W2f>(2, W2f::HALO, 0, 0, 0, 0, 4, nx, ny, nz, probe_w2<float>);
    else if (!strcmp(argv[1], "x2_ry1")) run<WaferX2Cfg<1>>(1, WaferX2Cfg<1>::HALO, 0, 0, 0, 0, 8, nx, ny, nz, probe_x2<1>);
    else if (!strcmp(argv[1], "x2_ry2")) run<WaferX2Cfg<2>>(1, WaferX2Cfg<2>::HALO, 0, 0, 0, 0, 8, nx, ny, nz, probe_x2<2>);
    else return 2;
    return 0;
}
"""

# What each kernel does with the roles beyond what the header states (the plane-loop bodies):
#   outer: the waves that stage an outer level-0 row;
#   row_levels[k]: which row waves also compute level k on their halo row ("all" four, or the "inner" two next to the tile);
#   cell_rows[k]: the rows of the level-0 tile (per side: dropped) on which halo-column cells exist at level k.  It is the rows of
#       the level-k LDS tile, except in the two-step excited kernel: its level 1 is the last level that is read, by a cross-shaped
#       stencil from the tile's own rows only ("Y1 on the inner column", wafer_stencil_x2.hip.h), so the cells of the rows above and
#       below the tile (row y0-1 / y0+TY, the corners of the cross) are not computed.
KERNELS = {
    "f3_f64": dict(outer=(1, 6), row_levels={1: "all", 2: "inner"}, cell_drop={1: 1, 2: 2}),
    "f3_f32": dict(outer=(1, 6), row_levels={1: "all", 2: "inner"}, cell_drop={1: 1, 2: 2}),
    "w2_f64": dict(outer=(0, 1, 6, 7), row_levels={1: "all"}, cell_drop={1: 2}),
    "w2_f32": dict(outer=(0, 1, 6, 7), row_levels={1: "all"}, cell_drop={1: 2}),
    "x2_ry1": dict(outer=(), row_levels={1: "inner"}, cell_drop={1: 2}),
    "x2_ry2": dict(outer=(), row_levels={1: "inner"}, cell_drop={1: 2}),
}


def grids(tx, ty):
    """whole, ragged and tiny grids for a TX x TY tile (nz plays no part in the roles)"""
    return [(tx, ty, 4), (2 * tx, 2 * ty, 4), (tx + 1, ty, 4), (5, 2 * ty, 4), (tx, ty - 3, 4), (tx, ty + 1, 4), (37, 50, 23), (130, 6, 5),
            (2 * tx + 3, 2 * ty + 5, 4), (1, 1, 1)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("roles")
    src, exe = d / "roles.hip", d / "roles"
    src.write_text(HARNESS)
    r = subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def call(*args):
        out = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        return out.stdout.splitlines()
    return call


def parse(lines):
    c = dict(zip("R HALO VEC RY TX TY HC0 HC1 HC2 ROWS0 ROWS1 ROWS2 LP0 LP1 LP2 HX0 HX1 HX2 NCOL CPW".split(), map(int, lines[0].split()[1:])))
    g = dict(zip("pitch xoff gy py gz lz plane total base_off ntx nty".split(), map(int, lines[1].split()[1:])))
    tiles = []
    for ln in lines[2:]:
        f = ln.split()
        if f[0] == "T":
            tiles.append(((int(f[1]), int(f[2])), []))
            continue
        v = [int(x) for x in f]
        ry = c["RY"]
        d = dict(zip(("wave", "lane", "xl", "x_row", "inner"), v[:5]))
        d["rows"] = [tuple(v[5 + 3 * r:8 + 3 * r]) for r in range(ry)]   # (y, work, offset)
        rest = v[5 + 3 * ry:]
        d.update(zip(("xy", "xwk", "xy_out", "xoff", "has_o", "oy", "oy_out", "ooff", "olds", "c_ok", "crow", "ckk", "clc", "cxw", "cy", "c_wk",
                      "c_xout", "c_off", "c_lds0", "c_l1", "c_lds1", "c_l2", "c_lds2"), rest))
        assert len(rest) == 23
        tiles[-1][1].append(d)
    return c, g, tiles


def check_tile(kern, c, g, nx, ny, x0, y0, lanes):
    K = KERNELS[kern]
    R, HALO, VEC, RY, TX, TY, HC0 = (c[k] for k in ("R", "HALO", "VEC", "RY", "TX", "TY", "HC0"))
    pitch, xoff = g["pitch"], g["xoff"]
    assert len(lanes) == 512

    def where(off, width):
        """(work row, work column) of an offset; inside the padded allocation (guard rows included) and inside its row"""
        yp, col = divmod(off, pitch)
        assert -g["gy"] <= yp < g["py"] + g["gy"], (off, yp)
        assert col + width <= pitch
        for z in (-g["gz"], g["lz"] + g["gz"] - 1):   # the first and last plane a pointer of this geometry may be moved to
            assert 0 <= g["base_off"] + z * g["plane"] + off and g["base_off"] + z * g["plane"] + off + width <= g["total"]
        return yp - R, col - xoff - R

    # ---- rows: level 0 is covered once by main rows + halo rows + staged outer rows, level k by main rows + the row waves of level k
    level0 = {}          # work row -> wave that requests it
    requested = set()    # rows a wave of this tile really requests (not redirected)
    for d in lanes:
        wave, lane, xl = d["wave"], d["lane"], d["xl"]
        assert xl == lane * VEC and d["x_row"] == (wave in (0, 1, 6, 7)) and d["inner"] == (wave in (0, 7))
        for r, (y, wk, off) in enumerate(d["rows"]):
            assert y == y0 + wave * RY + r and wk == (y < ny)
            assert where(off, VEC) == (y, x0 + xl)
            level0.setdefault(y, set()).add(wave)
            requested.add(y)
        own = d["rows"][0][2]
        slots = [("xy", "xy_out", "xoff", bool(d["x_row"]))]
        if K["outer"]:
            slots.append(("oy", "oy_out", "ooff", wave in K["outer"]))
            assert d["has_o"] == (wave in K["outer"])
        for ky, kout, koff, active in slots:
            if not active:
                continue
            y, out, off = d[ky], d[kout], d[koff]
            assert out == (not 0 <= y < ny)
            level0.setdefault(y, set()).add(wave)
            if out:   # redirected: the request the wave makes for its own first main row
                assert off == own
            else:
                assert where(off, VEC) == (y, x0 + xl)
                requested.add(y)
        if d["x_row"]:
            assert {0: y0 - 1, 1: y0 - 2, 6: y0 + TY + 1, 7: y0 + TY}[wave] == d["xy"]
            assert d["xwk"] == (0 <= d["xy"] < ny) and not (d["xy_out"] and d["xwk"])
        else:
            assert not d["xwk"]
    assert sorted(level0) == list(range(y0 - HALO, y0 + TY + HALO)) and all(len(w) == 1 for w in level0.values())
    for k, who in K["row_levels"].items():
        drop = (c["ROWS0"] - c["ROWS%d" % k]) // 2
        rows = [y for d in lanes if d["lane"] == 0 for y, _, _ in d["rows"]]
        rows += [d["xy"] for d in lanes if d["lane"] == 0 and d["x_row"] and (who == "all" or d["inner"])]
        assert sorted(rows) == list(range(y0 - HALO + drop, y0 + TY + HALO - drop)), (k, rows)

    # ---- halo-column cells: every cell one owner among waves 2..5, nobody else owns one
    owners = {}
    for d in lanes:
        wave, lane = d["wave"], d["lane"]
        idx = (wave - 2) * c["CPW"] + lane
        assert d["c_ok"] == (2 <= wave < 6 and lane < c["CPW"] and idx < c["NCOL"])
        if not d["x_row"]:
            # every lane of a column wave issues the extra slot's requests (the same instructions in every wave), a vector that
            # starts at c_off -- also the lanes beyond the last cell, which ask for the last cell again
            where(d["c_off"], VEC)
            assert 0 <= d["crow"] < c["ROWS0"]
        if not d["c_ok"]:
            assert not d["c_l1"] and not d["c_l2"]
            continue
        side_k = -1 - d["clc"] if d["clc"] < 0 else HC0 + d["clc"] - TX
        assert 0 <= side_k < 2 * HC0 and d["ckk"] == side_k % HC0 and d["crow"] * 2 * HC0 + side_k == idx
        assert (d["cxw"], d["cy"]) == (x0 + d["clc"], y0 - HALO + d["crow"])
        assert d["clc"] in list(range(-HC0, 0)) + list(range(TX, TX + HC0)) and 0 <= d["crow"] < c["ROWS0"]
        owners.setdefault((d["crow"], d["clc"]), []).append((wave, lane))
        inside = 0 <= d["cxw"] < nx and 0 <= d["cy"] < ny
        assert d["c_wk"] == inside and d["c_xout"] == (not inside)   # (out of area is never work)
        y, x = where(d["c_off"], 1)
        if inside:
            assert (y, x) == (d["cy"], d["cxw"])
        else:
            # redirected to a line the tile's own waves ask for in that plane anyway: the cell's row, or the tile's first / last row
            # for a cell above / below the work area; the tile's own edge column for a cell left / right of it.  (A cell above /
            # below the area in a column of the area keeps its column: the line of the halo-column cell of the tile's first /
            # last row, which the tile asks for as well.)
            assert y == (y0 if d["cy"] < 0 else y0 + TY - 1 if d["cy"] >= ny else d["cy"]) and y in requested
            assert x == (d["cxw"] if 0 <= d["cxw"] < nx else x0 if d["clc"] < 0 else x0 + TX - 1)
            assert x0 <= x < x0 + TX or 0 <= x < nx
            if not x0 <= x < x0 + TX:
                assert y in (y0, y0 + TY - 1) and x == d["cxw"]
        for k, dropk in K["cell_drop"].items():
            assert d["c_l%d" % k] == (d["ckk"] < c["HC%d" % k] and dropk <= d["crow"] < c["ROWS0"] - dropk), (k, d)
    assert len(owners) == c["NCOL"] and all(len(o) == 1 for o in owners.values())

    # ---- LDS: every offset inside its tile, no two owners share one
    for k in [0] + sorted(K["cell_drop"]):
        lp, hx, rows_k = c["LP%d" % k], c["HX%d" % k], c["ROWS%d" % k]
        drop = (c["ROWS0"] - rows_k) // 2
        used = {}

        def take(o, width, who):
            for i in range(o, o + width):
                assert 0 <= i < rows_k * lp and i not in used, (k, i, who, used.get(i))
                used[i] = who
        for d in lanes:
            who = (d["wave"], d["lane"])
            ys = [y for y, _, _ in d["rows"]]
            if d["x_row"] and (k == 0 or K["row_levels"][k] == "all" or d["inner"]):
                ys.append(d["xy"])
            for y in ys:   # (a row's vector: the plane-loop bodies form this offset themselves)
                take((y - (y0 - HALO + drop)) * lp + hx + d["xl"], VEC, who)
            if k == 0 and d["wave"] in K["outer"]:
                assert d["olds"] == (d["oy"] - (y0 - HALO)) * lp + hx + d["xl"]
                take(d["olds"], VEC, who)
            if d["c_ok"] and (k == 0 or d["c_l%d" % k]):
                assert d["c_lds%d" % k] == (d["crow"] - drop) * lp + hx + d["clc"]
                take(d["c_lds%d" % k], 1, who)


@pytest.mark.parametrize("kern", sorted(KERNELS))
def test_roles_on_every_tile(harness, kern):
    tx = {"f3_f32": 256, "w2_f32": 256}.get(kern, 128)
    ty = 8 if kern == "x2_ry1" else 16
    for nx, ny, nz in grids(tx, ty):
        c, g, tiles = parse(harness(kern, nx, ny, nz))
        assert (c["TX"], c["TY"]) == (tx, ty) and c["ROWS0"] == ty + 2 * c["HALO"] and c["NCOL"] == 2 * c["HC0"] * c["ROWS0"]
        assert len(tiles) == g["ntx"] * g["nty"] == -(-nx // tx) * -(-ny // ty)
        for (x0, y0), lanes in tiles:
            check_tile(kern, c, g, nx, ny, x0, y0, lanes)


def test_xcd_tile_is_a_permutation(harness):
    for n, line in enumerate(harness("xcd", 600), start=1):
        got = [int(x) for x in line.split()]
        q, r = n >> 3, n & 7
        assert got == [(b & 7) * q + min(b & 7, r) + (b >> 3) for b in range(n)]
        assert sorted(got) == list(range(n))
