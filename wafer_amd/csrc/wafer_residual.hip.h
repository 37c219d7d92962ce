// Residuals r = H l - theta l of stored states and of phi (gfx950): the sums |r|^2, <l|H|l>, <l|l> (wafer_k_residual_sums) and
// r itself as a wavefunction array (wafer_k_residual_write).  On the writer's partition and body: one step of the Chebyshev filter
// of a stored state (wafer_k_filter_step); and the largest V over the work cells, for the filter's upper bound (wafer_k_v_max).
// The entry points are in wafer_tu_residual.hip; the batch's kernels over the member table are in wafer_residual_batch.hip.h
// and wafer_store_filter_batch.hip.h.
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
// MODE 1 (WRITE): (T)r goes to dst[c] instead, a whole 16-byte vector per lane whose cells beyond column nx - 1 are zeros (they are
// pad or frame cells of the destination: the pitch holds whole tiles, wafer_geom.h); nothing is summed.
// MODE 2, 3: a step of the Chebyshev filter (wafer_k_filter_step below; wafer_filter.h) with cc = theta,
//   t = hw - cc * w        y = al * t        MODE 3: y = y - be * prev[c]
// MODE 2 (the first step) stores (T)y as MODE 1 stores (T)r -- the residual writer is this step with al = 1.  MODE 3 takes prev[c]
// from dst itself, loaded before the store, and writes work cells only: the new iterate goes over the one before last, in place.
enum { WAFER_CELLS_SUMS = 0, WAFER_CELLS_WRITE = 1, WAFER_CELLS_FILTER_FIRST = 2, WAFER_CELLS_FILTER_NEXT = 3 };
template <int R, typename T, int MODE>
__device__ __forceinline__ void wafer_residual_cells(const WaferGeom &g, int xi, int yw, int zs, int ze, const T *__restrict__ lj,
                                                     const T *__restrict__ pv, const WaferDen<double> &den, double theta,
                                                     T *__restrict__ dst, double &r2, double &wh, double &s, double al = 1.0, double be = 0.0)
{
    constexpr int RY = 2;
    constexpr bool WRITE = MODE != WAFER_CELLS_SUMS, NEXT = MODE == WAFER_CELLS_FILTER_NEXT;
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
            if (NEXT) out = *reinterpret_cast<const VT *>(dst + c0);   // prev, and what the cells beyond column nx - 1 keep
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if (WRITE && !NEXT) out[v] = (T)0;
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
                if (MODE == WAFER_CELLS_WRITE) {
                    out[v] = (T)res;
                } else if (WRITE) {
                    double y = al * res;
                    if (NEXT) y = y - be * (double)out[v];
                    out[v] = (T)y;
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
    wafer_residual_cells<R, T, WAFER_CELLS_SUMS>(g, xi, yw, zs, ze, lj, pv, den, th, nullptr, r2, wh, s);
    const double r2s = wafer_block_sum<NW>(r2, red, tid);
    if (tid == 0) partials[(size_t)(j * 3 + 0) * pstride + blockIdx.x] = r2s;
    const double whs = wafer_block_sum<NW>(wh, red, tid);
    if (tid == 0) partials[(size_t)(j * 3 + 1) * pstride + blockIdx.x] = whs;
    const double ss = wafer_block_sum<NW>(s, red, tid);
    if (tid == 0) partials[(size_t)(j * 3 + 2) * pstride + blockIdx.x] = ss;
}

// Zeros into every 16-byte vector of dst's allocation that holds no work cell (n16 vectors from the allocation's base
// dst - g.base_off), by a grid-stride loop of workgroups of NT threads.
template <int R, typename T, int NT>
__device__ __forceinline__ void wafer_zero_outside_work(const WaferStepArgs &a, T *__restrict__ dst, long long n16, int tid)
{
    using VT = typename WaferVec<T>::type;
    constexpr int VEC = WaferVec<T>::N;
    const WaferGeom &g = a.g;
    VT *__restrict__ base = reinterpret_cast<VT *>(dst - g.base_off);
    const int x0 = g.xoff + R;   // the first work column of a row, in elements from the row's start
    VT zero;
#pragma unroll
    for (int v = 0; v < VEC; ++v) zero[v] = (T)0;
    for (long long q = (long long)blockIdx.x * NT + tid; q < n16; q += (long long)gridDim.x * NT) {
        const long long e = q * VEC;
        const int zp = (int)(e / g.plane) - g.gz;           // local plane, row and column of the vector's first element
        const long long rem = e % g.plane;
        const int yp = (int)(rem / g.pitch) - g.gy;
        const int col = (int)(rem % g.pitch);
        const bool work = zp >= a.lz_lo && zp < a.lz_hi && yp >= R && yp < R + g.ny && col >= x0 && col < x0 + g.nx;
        if (!work) base[q] = zero;
    }
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
    wafer_residual_cells<R, T, WAFER_CELLS_WRITE>(g, xi, yw, zs, ze, lj, pv, den, theta, dst, r2, wh, s);
    wafer_zero_outside_work<R, T, NW * 64>(a, dst, n16, tid);
}

// One step of the Chebyshev filter on one stored state (wafer_filter_states; the coefficients: wafer_filter.h), on the writer's
// partition and per-cell body: per work cell c, fp64 and unfused whatever T,
//   hw = V[c] cur[c] - S / den        t = hw - cc cur[c]        y = al t        not FIRST: y = y - be prev[c]        out[c] = (T)y
// FIRST: out is another array than cur and every vector of it that holds no work cell gets zeros, as from the writer.  Otherwise out
// IS prev: the lane loads prev[c] before it stores, nobody else reads or writes that cell, and only work cells change.
template <int R, typename T, bool FIRST>
__global__ __launch_bounds__(WaferRitzCfg<R>::NW * 64) void wafer_k_filter_step(WaferStepArgs a, int ntx, int nty, int swz, const T *__restrict__ cur,
                                                                                 const T *__restrict__ pv, T *__restrict__ out, double al, double be,
                                                                                 double cc, long long n16)
{
    using Tile = WaferResidualTile<R, T>;
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
    wafer_residual_cells<R, T, FIRST ? WAFER_CELLS_FILTER_FIRST : WAFER_CELLS_FILTER_NEXT>(g, xi, yw, zs, ze, cur, pv, den, cc, out, r2, wh, s, al, be);
    if (FIRST) wafer_zero_outside_work<R, T, NW * 64>(a, out, n16, tid);
}

// ---- the largest V over the work cells (wafer_spectral_bound, wafer_batch_spectral_bound) -------------------------------------
// A double as a 64-bit key whose unsigned order is the numeric order (a NaN sorts beyond the infinity of its sign),
// and back.  The maximum of keys is exact, so the bound's V term has the bits of the largest stored value, widened.
__host__ __device__ __forceinline__ unsigned long long wafer_order_key(double x)
{
    unsigned long long u;
    __builtin_memcpy(&u, &x, 8);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__host__ __device__ __forceinline__ double wafer_order_value(unsigned long long k)
{
    const unsigned long long u = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
    double x;
    __builtin_memcpy(&x, &u, 8);
    return x;
}

// One 64 x 4 tile of one work plane of v (a logical pointer): the workgroup's largest key into *word by at most one integer
// atomicMax, skipped where the word, read first, is already as large (it only ever rises; the host starts it at 0, below every
// key).  A workgroup beyond the geometry's tiles or planes leaves as a whole before any load or barrier.  Block (64, 4).
template <typename T>
__device__ __forceinline__ void wafer_v_max_tile(const WaferGeom &g, const T *__restrict__ v, int tile, int plane, unsigned long long *word)
{
    const int ntx = (g.nx + 63) / 64;
    if (plane >= g.nzl || tile >= ntx * ((g.ny + 3) / 4)) return;
    const int i = (tile % ntx) * 64 + threadIdx.x, j = (tile / ntx) * 4 + threadIdx.y;
    unsigned long long key = 0;
    if (i < g.nx && j < g.ny) key = wafer_order_key((double)v[(long long)(g.G + plane) * g.plane + (long long)(j + g.R) * g.pitch + g.xoff + g.R + i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long k2 = __shfl_down(key, off, 64);
        key = k2 > key ? k2 : key;
    }
    __shared__ unsigned long long part[4];
    if (threadIdx.x == 0) part[threadIdx.y] = key;
    __syncthreads();
    if (threadIdx.x != 0 || threadIdx.y != 0) return;
#pragma unroll
    for (int w = 1; w < 4; ++w) key = part[w] > key ? part[w] : key;
    if (key > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, key);
}

// a context's: grid (tiles, planes)
template <typename T>
__global__ __launch_bounds__(256) void wafer_k_v_max(WaferGeom g, const T *__restrict__ v, unsigned long long *__restrict__ word)
{
    wafer_v_max_tile<T>(g, v, blockIdx.x, blockIdx.y, word);
}
