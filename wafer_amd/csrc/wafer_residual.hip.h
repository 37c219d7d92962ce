// Residuals r = H l - theta l of stored states and of phi (gfx950): the sums |r|^2, <l|H|l>, <l|l> (wafer_k_residual_sums) and
// r itself as a wavefunction array (wafer_k_residual_write).  The entry points are in wafer_tu_residual.hip; the batch's kernels
// over the member table are in wafer_residual_batch.hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "wafer_geom.h"
#include "wafer_stencil.hip.h"
#include "wafer_stencil_lds.hip.h"
#include "wafer_tile_roles.hip.h"
#include "wafer_ritz.hip.h"

// theta_j of column j, in the argument block like the state pointers (WaferRitzPtrs)
struct WaferResidualTheta {
    double t[WAFER_RITZ_MAX] = {0., 0., 0., 0., 0., 0., 0., 0.};
};

// The per-cell body, one text for the context's kernels below and the batch's (wafer_residual_batch.hip.h): the lane's cells -- RY = 2
// rows from work row yw, VEC cells from work column xi, planes [zs, ze) -- in the order plane, row, cell (wafer_ritz_cells' order).
// Per work cell c of the source l (lj, a logical pointer like pv), every operand widened to double, every operation fp64, unfused:
//   w = l[c]   vv = V[c]   S = the bracketed stencil sum of l at c (frame cells as they are stored)   q = S / den
//   hw = vv * w - q        r = hw - theta * w
//   r2 += r * r            wh += w * hw            s += w * w
// WRITE: (T)r goes to dst[c] instead, a whole 16-byte vector per lane whose cells beyond column nx - 1 are zeros (they are pad or
// frame cells of the destination: the pitch holds whole tiles, wafer_geom.h); nothing is summed.
template <int R, typename T, bool WRITE>
__device__ __forceinline__ void wafer_residual_cells(const WaferGeom &g, int xi, int yw, int zs, int ze, const T *__restrict__ lj,
                                                     const T *__restrict__ pv, const WaferDen<double> &den, double theta,
                                                     T *__restrict__ dst, double &r2, double &wh, double &s)
{
    constexpr int RY = 2;
    using VT = typename WaferVec<T>::type;
    constexpr int VEC = WaferVec<T>::N;
    for (int z = zs; z < ze; ++z) {
        const long long zo = (long long)z * g.plane;
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const int y = yw + r;
            if (y >= g.ny || xi >= g.nx) continue;
            const long long c0 = zo + (long long)(y + R) * g.pitch + g.xoff + R + xi;   // 16-byte aligned (wafer_geom.h)
            const VT wv = *reinterpret_cast<const VT *>(lj + c0);
            VT yv[2 * R + 1], zv[2 * R + 1];
            T xlo[R], xhi[R];   // columns xi-1-m and xi+VEC+m
#pragma unroll
            for (int d = -R; d <= R; ++d) {
                if (d == 0) continue;
                yv[d + R] = *reinterpret_cast<const VT *>(lj + c0 + (long long)d * g.pitch);
                zv[d + R] = *reinterpret_cast<const VT *>(lj + c0 + (long long)d * g.plane);
            }
#pragma unroll
            for (int m = 0; m < R; ++m) {
                xlo[m] = lj[c0 - 1 - m];
                xhi[m] = lj[c0 + VEC + m];
            }
            const VT vv4 = *reinterpret_cast<const VT *>(pv + c0);
            VT out;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if (WRITE) out[v] = (T)0;
                if (xi + v >= g.nx) continue;
                double xs[2 * R + 1], ys[2 * R + 1], zz[2 * R + 1];
                const double w = (double)wv[v];
#pragma unroll
                for (int d = -R; d <= R; ++d) {
                    if (d == 0) {
                        xs[R] = ys[R] = zz[R] = w;
                    } else {
                        xs[d + R] = (v + d >= 0 && v + d < VEC) ? (double)wv[(v + d + VEC) % VEC]
                                    : (v + d < 0)               ? (double)xlo[(-(v + d) - 1 + R) % R]
                                                                : (double)xhi[(v + d - VEC + R) % R];
                        ys[d + R] = (double)yv[d + R][v];
                        zz[d + R] = (double)zv[d + R][v];
                    }
                }
                const double S = wafer_stencil_sum<double, R>(xs, ys, zz, w);
                const double vv = (double)vv4[v];
                const double q = wafer_div_invariant<double>(S, den);
                const double hw = vv * w - q;
                const double res = hw - theta * w;
                if (WRITE) {
                    out[v] = (T)res;
                } else {
                    r2 += res * res;
                    wh += w * hw;
                    s += w * w;
                }
            }
            if (WRITE) *reinterpret_cast<VT *>(dst + c0) = out;
        }
    }
}

// the workgroup's tile on the partition of the context's observables launch (wafer_k_ritz_sums' own lines)
template <int R, typename T>
struct WaferResidualTile {
    static constexpr int NW = WaferRitzCfg<R>::NW, RY = 2;
    static constexpr int VEC = WaferVec<T>::N, TX = 64 * VEC, TY = NW * RY;
};

// Column j = blockIdx.y: the three sums of source j (st.p[j], a stored state or phi) with theta.t[j], over the body above, on the
// partition of wafer_k_ritz_sums and the observables launch: NW waves x 2 rows x VEC cells per lane, a.zchunk planes per
// workgroup, the same XCD swizzle, the same lane order -- so s has the bits of wafer_observables' norm2 and of wafer_ritz_matrices'
// s[j][j] on the same state.  partials[(j * 3 + q) * pstride + workgroup] = the workgroup's r2 (q = 0), wh (1), s (2); no
// floating-point atomics.  wafer_k_reduce over the 3 k rows follows.
template <int R, typename T>
__global__ __launch_bounds__(WaferRitzCfg<R>::NW * 64) void wafer_k_residual_sums(WaferStepArgs a, int ntx, int nty, int swz, WaferRitzPtrs st,
                                                                                   WaferResidualTheta theta, const T *__restrict__ pv,
                                                                                   double *__restrict__ partials, long long pstride)
{
    using Tile = WaferResidualTile<R, T>;
    constexpr int NW = Tile::NW, KM = WAFER_RITZ_MAX;
    __shared__ double red[NW];
    const WaferGeom &g = a.g;
    int bid = blockIdx.x;
    if (swz) bid = wafer_xcd_tile(bid, gridDim.x);
    const int tx_i = bid % ntx;
    const int ty_i = (bid / ntx) % nty;
    const int tz_i = bid / (ntx * nty);
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int xi = tx_i * Tile::TX + lane * Tile::VEC;   // work-x of the lane's first cell
    const int yw = ty_i * Tile::TY + wave * Tile::RY;    // work-y of the lane's first row
    const int zs = a.lz_lo + tz_i * a.zchunk;
    const int ze = min(zs + a.zchunk, a.lz_hi);
    const int j = blockIdx.y;
    // the column's source and theta, by select chains (an index into the argument block would be a private array)
    const T *__restrict__ lj = static_cast<const T *>(st.p[0]);
    double th = theta.t[0];
#pragma unroll
    for (int i = 1; i < KM; ++i)
        if (j == i) {
            lj = static_cast<const T *>(st.p[i]);
            th = theta.t[i];
        }
    const WaferDen<double> den = wafer_den<double>(a, a.v_in_range != 0);

    double r2 = 0.0, wh = 0.0, s = 0.0;
    wafer_residual_cells<R, T, false>(g, xi, yw, zs, ze, lj, pv, den, th, nullptr, r2, wh, s);
    const double r2s = wafer_block_sum<NW>(r2, red, tid);
    if (tid == 0) partials[(size_t)(j * 3 + 0) * pstride + blockIdx.x] = r2s;
    const double whs = wafer_block_sum<NW>(wh, red, tid);
    if (tid == 0) partials[(size_t)(j * 3 + 1) * pstride + blockIdx.x] = whs;
    const double ss = wafer_block_sum<NW>(s, red, tid);
    if (tid == 0) partials[(size_t)(j * 3 + 2) * pstride + blockIdx.x] = ss;
}

// The writer: dst = r of the source lj with theta, a valid wavefunction array.  The work cells come from the body above on the
// same partition (grid: its workgroups); every 16-byte vector of dst's allocation that holds no work cell -- frame, pad and guard
// cells; n16 vectors from the allocation's base dst - g.base_off -- gets zeros from a grid-stride loop.  A vector either begins
// at a work column xi < nx of a work row (the first loop stores it whole) or holds no work cell at all (rows begin on 128 bytes
// and the first work column too): no element is stored twice.  lj and dst are different arrays.
template <int R, typename T>
__global__ __launch_bounds__(WaferRitzCfg<R>::NW * 64) void wafer_k_residual_write(WaferStepArgs a, int ntx, int nty, int swz, const T *__restrict__ lj,
                                                                                    double theta, const T *__restrict__ pv, T *__restrict__ dst,
                                                                                    long long n16)
{
    using Tile = WaferResidualTile<R, T>;
    using VT = typename WaferVec<T>::type;
    constexpr int NW = Tile::NW, VEC = Tile::VEC;
    const WaferGeom &g = a.g;
    int bid = blockIdx.x;
    if (swz) bid = wafer_xcd_tile(bid, gridDim.x);
    const int tx_i = bid % ntx;
    const int ty_i = (bid / ntx) % nty;
    const int tz_i = bid / (ntx * nty);
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int xi = tx_i * Tile::TX + lane * VEC;
    const int yw = ty_i * Tile::TY + wave * Tile::RY;
    const int zs = a.lz_lo + tz_i * a.zchunk;
    const int ze = min(zs + a.zchunk, a.lz_hi);
    const WaferDen<double> den = wafer_den<double>(a, a.v_in_range != 0);
    double r2 = 0.0, wh = 0.0, s = 0.0;
    wafer_residual_cells<R, T, true>(g, xi, yw, zs, ze, lj, pv, den, theta, dst, r2, wh, s);

    VT *__restrict__ base = reinterpret_cast<VT *>(dst - g.base_off);
    const int x0 = g.xoff + R;   // the first work column of a row, in elements from the row's start
    VT zero;
#pragma unroll
    for (int v = 0; v < VEC; ++v) zero[v] = (T)0;
    for (long long q = (long long)blockIdx.x * (NW * 64) + tid; q < n16; q += (long long)gridDim.x * (NW * 64)) {
        const long long e = q * VEC;
        const int zp = (int)(e / g.plane) - g.gz;           // local plane, row and column of the vector's first element
        const long long rem = e % g.plane;
        const int yp = (int)(rem / g.pitch) - g.gy;
        const int col = (int)(rem % g.pitch);
        const bool work = zp >= a.lz_lo && zp < a.lz_hi && yp >= R && yp < R + g.ny && col >= x0 && col < x0 + g.nx;
        if (!work) base[q] = zero;
    }
}
