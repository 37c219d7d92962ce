// The eight-wave tile layout of the fused stencil kernels, stated once: which rows and cells of a tile a (wave, lane) owns, where
// its requests go in global memory and in LDS, and the XCD-aware order of the tiles.  Used by wafer_k_step3_fused
// (wafer_stencil_fused3.hip.h), wafer_k_step2_wide (wafer_stencil_fused2w.hip.h) and wafer_k_xstep2 (wafer_stencil_x2.hip.h);
// tests/test_tile_roles.py runs it on the host over whole, ragged and tiny grids.
//
// A workgroup is eight waves on a TX x TY tile (TX = 64 VEC columns, one vector per lane; TY = 8 RY rows) at (x0, y0).  The input
// level (level 0) is needed HALO rows and HC0 columns beyond the tile, level k on fewer (Cfg::ROWSk rows, Cfg::HCk columns).  Every
// wave owns the RY MAIN ROWS y0 + wave RY + r of the tile at every level, plus ONE extra slot:
//   wave 0   halo row y0-1          wave 7   halo row y0+TY
//   wave 1   halo row y0-2          wave 6   halo row y0+TY+1
//   (row waves may also STAGE one row further out, level 0 only: which wave which row is the kernel's own table)
//   waves 2..5 (Cfg::HCW0 .. HCW0 + HCWN - 1)   the NCOL = 2 HC0 ROWS0 level-0 halo-column cells, CPW per wave, one per lane:
//            cell c is row c / (2 HC0) of the level-0 LDS tile (work row y0 - HALO + that), k = c % (2 HC0):
//            k < HC0: column x0-1-k, else column x0+TX+(k-HC0); its depth (k or k - HC0) says at which levels it exists
// so every global access stays 128-byte aligned and tiles need no overlap.
//
// REDIRECTION.  A cell left or right of the work area (the Dirichlet frame column and the pad cells behind it: zeros that no kernel
// writes) is not fetched -- its 128-byte line holds nothing anybody else reads, so each such request was an HBM read of its own,
// 44 + 40 lines (phi0, V) per plane and row of tiles, 6 % of the three-step kernel's reads at 512^3 (the halo-attribution runs of
// profiles/NOTES.md, round 3).  The lane requests the tile's own edge cell of that row instead (a line the row's owner requests in
// the same iteration) and the kernel replaces the value by the zero it stands for; V of such a cell is never used (work).  The same
// for a cell above / below the work area: the tile's own first / last row.  A halo or staged ROW above / below the work area --
// frame and guard rows, zeros -- is not fetched either: the wave requests its own first main row again and takes zeros.
//
// An offset is in elements inside a plane, relative to the array pointer the kernels get (WaferGeom).  A row's offset is formed at
// the column the kernel names: x0 where the lane's columns (xl) are added at the request, as an unsigned value; x0 + xl where they
// are folded in.
//
// The roles are TEXT (macros that declare the kernel's locals), not functions: as inlined functions the same expressions reach the
// register allocator in another order, and every instantiation of the three kernels changed its registers (the three-step kernel
// 239 to 245 VGPRs against 241; the FivePoint kernel 90 against 92 SGPRs) -- what wafer_stencil_fused3_iter.inc.h found for lambdas.
// As text they compile to the instructions the kernels had before they shared them.  A host function that expands the same text
// (tests/test_tile_roles.py) is what pins them.  The macros read the enclosing scope's Cfg, R, RY, TX, TY, LP0, HX0, g, x0, y0, xl,
// wave, lane and x_row.
#pragma once
#include <hip/hip_runtime.h>
#include "wafer_geom.h"
#include "wafer_stencil.hip.h"
#include "wafer_storage.h"

// The tile of dispatch slot b of n: workgroup b runs on XCD b % 8 (observed, speed only), and each XCD should work on one
// contiguous range of tiles -- (x, y, z-chunk) order -- so that neighbouring tiles, which re-read each other's halo rows, share
// an L2.  A permutation of [0, n) for every n.
__host__ __device__ __forceinline__ int wafer_xcd_tile(int b, int n)
{
    const int q = n >> 3, r = n & 7, k = b & 7;
    return k * q + (k < r ? k : r) + (b >> 3);
}

// what the extra slot of a wave is
#define WAFER_TILE_ROW_WAVE (wave < 2 || wave >= 6)          /* a halo row (else: halo-column cells) */
#define WAFER_TILE_INNER_ROW_WAVE (wave == 0 || wave == 7)   /* ... the one next to the tile */
#define WAFER_TILE_OUTER_ROW_WAVE (wave == 1 || wave == 6)

// ---- main rows: yrow (the work row), rowwk ("is a work row"), rowoff (its offset at column COL_); MORE_: a statement of the
//      kernel's own per row r
#define WAFER_TILE_MAIN_ROWS(COL_, MORE_)                                                                                          \
    int yrow[RY];                                                                                                                  \
    bool rowwk[RY];                                                                                                                \
    long long rowoff[RY];                                                                                                          \
    _Pragma("unroll") for (int r = 0; r < RY; ++r)                                                                                 \
    {                                                                                                                              \
        const int y = y0 + wave * RY + r;                                                                                          \
        yrow[r] = y;                                                                                                               \
        rowwk[r] = y < g.ny;                                                                                                       \
        rowoff[r] = (long long)(y + R) * g.pitch + g.xoff + R + COL_;                                                              \
        MORE_;                                                                                                                     \
    }
// offset of the request for work row Y_ at column COL_: a row outside the work area is redirected to the wave's own first row
#define WAFER_TILE_ROW_OUTSIDE(Y_) ((Y_) < 0 || (Y_) >= g.ny)
#define WAFER_TILE_ROW_REQUEST(Y_, OUT_, COL_) ((OUT_) ? rowoff[0] : (long long)((Y_) + R) * g.pitch + g.xoff + R + (COL_))
// offset of work row Y_ inside the level-0 LDS tile, at the lane's columns
#define WAFER_TILE_LDS0_ROW(Y_) (((Y_) - (y0 - Cfg::HALO)) * LP0 + HX0 + xl)
// ---- the extra halo row: xy, xwk ("a work row of a row wave"), xy_out, xoff_row
#define WAFER_TILE_HALO_ROW_Y (wave == 0 ? y0 - 1 : wave == 1 ? y0 - 2 : wave == 6 ? y0 + TY + 1 : y0 + TY)
#define WAFER_TILE_HALO_ROW(COL_)                                                                                                  \
    const int xy = WAFER_TILE_HALO_ROW_Y;                                                                                          \
    const bool xwk = x_row && xy >= 0 && xy < g.ny;                                                                                \
    const bool xy_out = WAFER_TILE_ROW_OUTSIDE(xy);                                                                                \
    const long long xoff_row = WAFER_TILE_ROW_REQUEST(xy, xy_out, COL_)
// ---- the halo-column cell of this lane: crow (row of the level-0 LDS tile), ckk (its depth: columns between it and the tile), clc
//      (column relative to x0), cxw / cy (work column and row), c_ok (this lane owns a cell at all), c_wk (inside the work area),
//      c_xout (outside: redirected, stands for zero), c_off (of the request), c_lds0
#define WAFER_TILE_CELL_RY (cy < 0 ? y0 : cy >= g.ny ? y0 + TY - 1 : cy)                                  /* the row ... */
#define WAFER_TILE_CELL_RX ((cxw < 0 || cxw >= g.nx) ? (ck < Cfg::HC0 ? x0 : x0 + TX - 1) : cxw)          /* and column asked for */
#define WAFER_TILE_CELL_HEAD                                                                                                       \
    const int cidx = min((wave - Cfg::HCW0) * Cfg::CPW + lane, Cfg::NCOL - 1);                                                     \
    const int crow = cidx / (2 * Cfg::HC0), ck = cidx % (2 * Cfg::HC0);                                                            \
    const int ckk = (ck < Cfg::HC0) ? ck : ck - Cfg::HC0;                                                                          \
    const int clc = (ck < Cfg::HC0) ? (-1 - ckk) : (TX + ckk);                                                                     \
    const int cxw = x0 + clc, cy = y0 - Cfg::HALO + crow;                                                                          \
    const bool c_ok = !x_row && lane < Cfg::CPW && (wave - Cfg::HCW0) * Cfg::CPW + lane < Cfg::NCOL;                               \
    const bool c_wk = cy >= 0 && cy < g.ny && cxw >= 0 && cxw < g.nx
#define WAFER_TILE_CELL_TAIL                                                                                                       \
    const bool c_xout = cxw < 0 || cxw >= g.nx || cy < 0 || cy >= g.ny;                                                            \
    const long long c_off = (long long)(WAFER_TILE_CELL_RY + R) * g.pitch + g.xoff + R + WAFER_TILE_CELL_RX
// the cell also exists at level K_ (Cfg::HC<K> halo columns), on the rows that drop DROP_ of the level-0 tile's on either side
#define WAFER_TILE_CELL_AT(K_, DROP_) (c_ok && ckk < Cfg::HC##K_ && crow >= DROP_ && crow < Cfg::ROWS0 - DROP_)
// ... and where in the LDS tile of level 0 / of that level (Cfg::ROWS<K> rows around the tile's)
#define WAFER_TILE_CELL_LDS0 (crow * LP0 + HX0 + clc)
#define WAFER_TILE_CELL_LDS(K_) ((crow - (Cfg::ROWS0 - Cfg::ROWS##K_) / 2) * LP##K_ + HX##K_ + clc)

// ---- the small helpers the three kernels share ----------------------------------------------------------------------
// local plane p is a plane of the global work range
__host__ __device__ __forceinline__ bool wafer_work_plane(const WaferGeom &g, int p)
{
    const int kg = g.z_begin + (p - g.G);
    return kg >= 0 && kg < g.nz;
}

// A lane's request of N cells: arrays of ST in HBM, T in registers / LDS.
template <typename ST, typename T, int N>
struct WaferStored {
    typedef ST __attribute__((ext_vector_type(N))) SVT;
    typedef T __attribute__((ext_vector_type(N))) VT;
    struct Raw {
        __device__ __forceinline__ SVT operator()(const ST *p) const { return *reinterpret_cast<const SVT *>(p); }
    };
    struct Widen {
        __device__ __forceinline__ VT operator()(const SVT &x) const { return wafer_f3_widen<SVT, VT, N>(x); }
    };
    struct Load {   // widened to the register type
        __device__ __forceinline__ VT operator()(const ST *p) const { return wafer_f3_widen<SVT, VT, N>(*reinterpret_cast<const SVT *>(p)); }
    };
    // a level's result as the storage type holds it (fp32 storage: rounded once per step, like a store and a load would)
    struct AsStored {
        template <typename C>
        __device__ __forceinline__ T operator()(C x) const { return (T)(ST)x; }
    };
};

template <typename C>
__device__ __forceinline__ void wafer_ab_from_v(C vv, C dt, bool v_in_range, C &ca, C &cb);   // wafer_stencil_fused2.hip.h

// Level 1: a, b from V (potential.rs:104-110); what rides to the later levels is a and the product b * dt -- b enters the update
// (grid.rs:580-589: w * a + b * dt * S / den, left to right) only through that product, which is the same number at every level.
// (VIR: the short reciprocal of a potential inside its range, a compile-time choice -- wafer_stencil_fused2.hip.h)
template <typename ST, typename T, typename C, bool VIR>
struct WaferUpdateKeep {
    C dt;
    const WaferDen<C> &den;
    __device__ __forceinline__ T operator()(C w, C vv, C S, C &ca, C &cbdt) const
    {
        C cb;
        wafer_ab_from_v<C>(vv, dt, VIR, ca, cb);
        cbdt = cb * dt;
        return (T)(ST)(w * ca + wafer_div_invariant<C>(cbdt * S, den));
    }
};
template <typename ST, typename T, typename C>
struct WaferUpdateWith {
    const WaferDen<C> &den;
    __device__ __forceinline__ T operator()(C w, C ca, C cbdt, C S) const { return (T)(ST)(w * ca + wafer_div_invariant<C>(cbdt * S, den)); }
};
