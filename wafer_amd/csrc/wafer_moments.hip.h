// Moment matrices of the stored states (gfx950): for the first k states of a context's w_store the five k x k matrices
//   S_ij = <l_i|l_j>   X_ij = <l_i|x|l_j>   Y_ij = <l_i|y|l_j>   Z_ij = <l_i|z|l_j>   R2_ij = <l_i|r^2|l_j>
// in one sums launch (wafer_moment_matrices; the batch's kernel: wafer_moments_batch.hip.h).  No V and no neighbours are read.
//
// Origin: with 0-based work indices (ix, iy, iz) of a grid nx x ny x nz,
//   dx = (double)ix - ((double)nx + 1.) / 2.     dy, dz likewise     r2c = dx * dx + dy * dy + dz * dz
// -- compute_observables' r^2, letter for letter (wafer_stencil_lds.hip.h, grid.rs:428-437), in index units like wafer_observables_t's
// r2.  That origin lies ONE CELL ABOVE the geometric centre (n - 1) / 2 of the work indices: it is the reference's convention, kept
// so that the diagonal of R2 ties to wafer_observables.  S is there so that a caller can move it: <i|x - c|j> = X_ij - c S_ij.
#pragma once
#include <hip/hip_runtime.h>
#include "wafer_geom.h"
#include "wafer_stencil.hip.h"
#include "wafer_stencil_lds.hip.h"
#include "wafer_tile_roles.hip.h"
#include "wafer_ritz.hip.h"   // WaferRitzPtrs, WaferRitzCfg, WAFER_RITZ_MAX

#ifndef WAFER_MOMENT_COUNT
#define WAFER_MOMENT_COUNT 5   // S, X, Y, Z, R2 (include/wafer_hip.h: WAFER_MOMENT_S ..)
#endif
// rows of partials (and of sums) of one call on k states: the entries i <= j of the five matrices, row (q, j, i) at
// q * k (k + 1) / 2 + j (j + 1) / 2 + i -- a column's rows do not move when k grows
__host__ __device__ inline int wafer_moment_tri(int k) { return k * (k + 1) / 2; }
__host__ __device__ inline int wafer_moment_rows(int k) { return WAFER_MOMENT_COUNT * wafer_moment_tri(k); }

// The per-cell body of the sums kernels, one text for the context's kernel below and the batch's: the lane's cells -- RY = 2 rows
// from work row yw, VEC cells from work column xi, planes [zs, ze) -- in the order plane, row, cell, adding the five
// operators of column j into m[q][i] for i <= j (q: WAFER_MOMENT_S .. WAFER_MOMENT_R2).  lj: the column's state, a logical pointer
// (plane 0, row 0); state i is st.p[i] + moff.  The frame offset is the only place the stencil's reach enters (g.R).  Frame cells are never read.
template <typename T>
__device__ __forceinline__ void wafer_moment_cells(const WaferGeom &g, int xi, int yw, int zs, int ze, int j, const T *__restrict__ lj,
                                                   const WaferRitzPtrs &st, long long moff, double (&m)[WAFER_MOMENT_COUNT][WAFER_RITZ_MAX])
{
    constexpr int RY = 2, KM = WAFER_RITZ_MAX;
    using VT = typename WaferVec<T>::type;
    constexpr int VEC = WaferVec<T>::N;
    const int R = g.R;
    for (int z = zs; z < ze; ++z) {
        const long long zo = (long long)z * g.plane;
        const double dz = (double)(g.z_begin + (z - g.G)) - ((double)g.nz + 1.) / 2.;
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const int y = yw + r;
            if (y >= g.ny || xi >= g.nx) continue;
            const long long c0 = zo + (long long)(y + R) * g.pitch + g.xoff + R + xi;   // 16-byte aligned (wafer_geom.h)
            const VT wv = *reinterpret_cast<const VT *>(lj + c0);
            VT li[KM];
#pragma unroll
            for (int i = 0; i < KM; ++i)
                if (i <= j) li[i] = *reinterpret_cast<const VT *>(static_cast<const T *>(st.p[i]) + moff + c0);
            const double dy = (double)y - ((double)g.ny + 1.) / 2.;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if (xi + v >= g.nx) continue;
                const double w = (double)wv[v];
                const double dx = (double)(xi + v) - ((double)g.nx + 1.) / 2.;
                const double r2c = dx * dx + dy * dy + dz * dz;
#pragma unroll
                for (int i = 0; i < KM; ++i)
                    if (i <= j) {
                        const double l = (double)li[i][v];
                        const double p = l * w;
                        m[0][i] += p;
                        m[1][i] += p * dx;
                        m[2][i] += p * dy;
                        m[3][i] += p * dz;
                        m[4][i] += p * r2c;
                    }
            }
        }
    }
}

// the block sums of a workgroup's accumulators and their places: partials[base + (q * tri + j (j + 1) / 2 + i) * pstride + workgroup]
template <int NW>
__device__ __forceinline__ void wafer_moment_store(const double (&m)[WAFER_MOMENT_COUNT][WAFER_RITZ_MAX], int j, int k, double *red, int tid,
                                                   double *__restrict__ partials, size_t base, long long pstride, int workgroup)
{
    const int tri = wafer_moment_tri(k), col = wafer_moment_tri(j);
#pragma unroll
    for (int q = 0; q < WAFER_MOMENT_COUNT; ++q)
#pragma unroll
        for (int i = 0; i < WAFER_RITZ_MAX; ++i)
            if (i <= j) {   // j is workgroup-uniform: every wave reaches the same barriers
                const double s = wafer_block_sum<NW>(m[q][i], red, tid);
                if (tid == 0) partials[base + (size_t)(q * tri + col + i) * pstride + workgroup] = s;
            }
}

// Column j = blockIdx.y: with w = l_j[c], every work cell c adds, for i <= j,
//   p = l_i[c] * w      S_ji += p    X_ji += p * dx    Y_ji += p * dy    Z_ji += p * dz    R2_ji += p * r2c
// -- every operand widened to double, every operation fp64 and unfused.  The partition is that of wafer_k_ritz_sums and of the
// context's observables launch: NW waves x RY = 2 rows x VEC cells per lane (16 bytes of T), a.zchunk planes per workgroup, the same
// XCD swizzle, a lane's cells in the order plane, row, cell -- so R2_jj and S_jj have the bits of wafer_observables' r2 and norm2
// on state j, and S_ji those of wafer_ritz_matrices' s.  R enters through the partition (NW) and the frame offset only.
// No floating-point atomics; wafer_k_reduce over the 5 k (k + 1) / 2 rows follows.
template <int R, typename T>
__global__ __launch_bounds__(WaferRitzCfg<R>::NW * 64) void wafer_k_moment_sums(WaferStepArgs a, int ntx, int nty, int swz, int k, WaferRitzPtrs st,
                                                                                 double *__restrict__ partials, long long pstride)
{
    constexpr int NW = WaferRitzCfg<R>::NW, RY = 2, KM = WAFER_RITZ_MAX;
    constexpr int VEC = WaferVec<T>::N, TX = 64 * VEC, TY = NW * RY;
    __shared__ double red[NW];
    const WaferGeom &g = a.g;
    int bid = blockIdx.x;
    if (swz) bid = wafer_xcd_tile(bid, gridDim.x);
    const int tx_i = bid % ntx;
    const int ty_i = (bid / ntx) % nty;
    const int tz_i = bid / (ntx * nty);
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int xi = tx_i * TX + lane * VEC;      // work-x of the lane's first cell
    const int yw = ty_i * TY + wave * RY;       // work-y of the lane's first row
    const int zs = a.lz_lo + tz_i * a.zchunk;
    const int ze = min(zs + a.zchunk, a.lz_hi);
    const int j = blockIdx.y;
    // the column's state, by a select chain (an index into the argument block would be a private array)
    const T *__restrict__ lj = static_cast<const T *>(st.p[0]);
#pragma unroll
    for (int i = 1; i < KM; ++i)
        if (j == i) lj = static_cast<const T *>(st.p[i]);
    double m[WAFER_MOMENT_COUNT][KM];
#pragma unroll
    for (int q = 0; q < WAFER_MOMENT_COUNT; ++q)
#pragma unroll
        for (int i = 0; i < KM; ++i) m[q][i] = 0.0;
    wafer_moment_cells<T>(g, xi, yw, zs, ze, j, lj, st, 0, m);
    wafer_moment_store<NW>(m, j, k, red, tid, partials, 0, pstride, (int)blockIdx.x);
}
