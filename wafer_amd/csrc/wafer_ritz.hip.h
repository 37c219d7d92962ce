// Rayleigh-Ritz on the stored states (gfx950): the sums H_ij = <l_i|H|l_j>, S_ij = <l_i|l_j> over the first k states of a
// context's w_store, and the rotation of those states by a k x k matrix.  The host solver between the two is wafer_ritz.h.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "wafer_geom.h"
#include "wafer_stencil.hip.h"
#include "wafer_stencil_lds.hip.h"
#include "wafer_tile_roles.hip.h"

#ifndef WAFER_RITZ_MAX
#define WAFER_RITZ_MAX 8
#endif

struct WaferRitzPtrs {
    void *p[WAFER_RITZ_MAX] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};

// waves per workgroup of the context's observables launch (wafer_launch_observables_lds)
template <int R>
struct WaferRitzCfg {
    static constexpr int NW = R <= 2 ? 8 : 4;
};

// The per-cell body of the sums kernels, one text for the context's kernel below and the batch's (wafer_ritz_batch.hip.h): the lane's
// cells -- RY = 2 rows from work row yw, VEC cells from work column xi, planes [zs, ze) -- in the order plane, row, cell, adding
// into h[i], s[i] for i < k.  lj: the column's state, pv: V, both logical pointers (plane 0, row 0); state i is st.p[i] + moff.
template <int R, typename T>
__device__ __forceinline__ void wafer_ritz_cells(const WaferGeom &g, int xi, int yw, int zs, int ze, int k, const T *__restrict__ lj,
                                                 const WaferRitzPtrs &st, long long moff, const T *__restrict__ pv,
                                                 const WaferDen<double> &den, double (&h)[WAFER_RITZ_MAX], double (&s)[WAFER_RITZ_MAX])
{
    constexpr int RY = 2, KM = WAFER_RITZ_MAX;
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
            VT li[KM];
#pragma unroll
            for (int i = 0; i < KM; ++i)
                if (i < k) li[i] = *reinterpret_cast<const VT *>(static_cast<const T *>(st.p[i]) + moff + c0);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
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
#pragma unroll
                for (int i = 0; i < KM; ++i)
                    if (i < k) {
                        const double l = (double)li[i][v];
                        h[i] += vv * l * w - wafer_div_invariant<double>(l * S, den);
                        s[i] += l * w;
                    }
            }
        }
    }
}

// Column j = blockIdx.y: with w = l_j[c], S = the bracketed sum of l_j at c and vv = V[c], every work cell c adds
//   h_i += vv * l_i[c] * w - (l_i[c] * S) / den        s_i += l_i[c] * w         for i < k
// -- every operand widened to double, every operation fp64 and unfused.  For i == j the h term is the energy integrand of
// wafer_k_step_lds<NLOW = -2> (grid.rs:325-332) and the s term its w * w, letter for letter, and the partition is that launch's:
// NW waves x RY = 2 rows x VEC cells per lane (16 bytes of T), a.zchunk planes per workgroup, the same XCD swizzle, a lane's
// cells taken in the order plane, row, cell -- so the diagonal sums have the bits of wafer_observables on the same state.
// The frame cells of l_j enter S as they are stored (zeros in every state the engine itself produces); nothing outside the work
// area is summed.  x neighbours outside the lane's own vector and the y, z neighbours come straight from global memory (L1 / L2):
// the kernel runs a handful of times after a solve.
// partials[(j * k + i) * pstride + workgroup] = the workgroup's h_i, partials[(k * k + j * k + i) * pstride + workgroup] = s_i;
// no floating-point atomics.  wafer_k_reduce over the 2 k^2 rows follows.
template <int R, typename T>
__global__ __launch_bounds__(WaferRitzCfg<R>::NW * 64) void wafer_k_ritz_sums(WaferStepArgs a, int ntx, int nty, int swz, int k, WaferRitzPtrs st,
                                                                               const T *__restrict__ pv, double *__restrict__ partials,
                                                                               long long pstride)
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
    const WaferDen<double> den = wafer_den<double>(a, a.v_in_range != 0);

    double h[KM], s[KM];
#pragma unroll
    for (int i = 0; i < KM; ++i) h[i] = s[i] = 0.0;
    wafer_ritz_cells<R, T>(g, xi, yw, zs, ze, k, lj, st, 0, pv, den, h, s);
#pragma unroll
    for (int i = 0; i < KM; ++i)
        if (i < k) {   // k is workgroup-uniform: every wave reaches the same barriers
            const double hs = wafer_block_sum<NW>(h[i], red, tid);
            if (tid == 0) partials[(size_t)(j * k + i) * pstride + blockIdx.x] = hs;
            const double ss = wafer_block_sum<NW>(s[i], red, tid);
            if (tid == 0) partials[(size_t)(k * k + j * k + i) * pstride + blockIdx.x] = ss;
        }
}

// l'_a = sum_j coef[j * k + a] l_j for the first k states, in place, over every element of the allocations -- work cells, frame,
// pad and guard cells alike (n16 vectors of 16 bytes from the allocations' bases in st.p): zeros stay zeros.  A thread loads its k
// vectors, then forms per output state acc = coef[0 * k + a] * l_0, acc = acc + coef[j * k + a] * l_j for j = 1 .. k-1 in that
// order (fp64, unfused) and stores (T)acc; it touches no other thread's cells.  coef: k * k doubles in device memory.
template <typename T>
__global__ __launch_bounds__(256) void wafer_k_rotate_states(long long n16, int k, WaferRitzPtrs st, const double *__restrict__ coef)
{
    constexpr int KM = WAFER_RITZ_MAX;
    using VT = typename WaferVec<T>::type;
    constexpr int VEC = WaferVec<T>::N;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n16; q += (long long)gridDim.x * 256) {
        VT l[KM];
#pragma unroll
        for (int j = 0; j < KM; ++j)
            if (j < k) l[j] = static_cast<const VT *>(st.p[j])[q];
#pragma unroll
        for (int a = 0; a < KM; ++a)
            if (a < k) {
                VT o;
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    double acc = coef[a] * (double)l[0][v];
#pragma unroll
                    for (int j = 1; j < KM; ++j)
                        if (j < k) acc = acc + coef[j * k + a] * (double)l[j][v];
                    o[v] = (T)acc;
                }
                static_cast<VT *>(st.p[a])[q] = o;
            }
    }
}
