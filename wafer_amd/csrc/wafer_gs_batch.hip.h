// Batched excited states (wafer_batch_evolve_state, wafer_batch_orthogonalise, wafer_batch_norm2): the per-step tail of
// grid.rs:674-681 for every active member of a batch -- norm2 of the new phi, phi /= sqrt(norm2), then modified Gram-Schmidt
// against the member's stored states in storage order, each overlap taken on the phi the previous projection left.
//
// Schedule of one step (wnum lower states), every scalar on the device:
//   wafer_k_batch_step                                   (wafer_stencil_batch.hip.h, unchanged)
//   wafer_k_batch_gs<NORM2>  + wafer_k_batch_gs_reduce   norm2 partials, norm2
//   wafer_k_batch_gs<SCALE>  + reduce                    phi /= sqrt(norm2) while summing lower_0 . phi
//   wafer_k_batch_gs<AXPY>   + reduce   (l = 0 .. wnum-2) phi -= lower_l s_l while summing lower_{l+1} . phi
//   wafer_k_batch_gs<AXPY>                               phi -= lower_{wnum-1} s_{wnum-1}
// 1 + 2 (1 + wnum) + 1 launches, whatever the number of members.
//
// Determinism and independence: the partition of a member is fixed by the geometry alone -- tiles of 64 x 4 work cells, chunks
// of WAFER_GS_ZC planes, one partial per workgroup at partials[member * nb + workgroup] -- and the reduce sums a member's nb
// partials in wafer_k_reduce's order.  The grid is (nb, active members): which other members run, how many there are and where
// the member sits in the batch change blockIdx.y and nothing a sum sees.  No floating-point atomics.
//
// Work cells only: frame cells are zero in phi and in every stored state, so the reference's whole-padded-array sums agree.
// Per cell the arithmetic is the single context's (wafer_k_row_op): x / sqrt(norm2) by wafer_div_invariant, x - l * s unfused.
//
// Float storage (T = float: dtype f32 and f32fast alike): phi and the stored states are float arrays, every operand is widened and
// every operation is fp64 (scalars, partials and sums stay double), and phi is rounded to float where a kernel writes it -- after
// the scale, after each projection -- BEFORE the overlap that rides along is summed: the sum sees what the next kernel loads.
#pragma once
#include <hip/hip_runtime.h>
#include "wafer_geom.h"
#include "wafer_stencil.hip.h"
#include "wafer_stencil_batch.hip.h"
#include "wafer_rowwalk.h"

#define WAFER_GS_ZC 4   // planes per workgroup: four independent loads per lane and array in flight

enum { WAFER_GS_NORM2 = 0, WAFER_GS_DOT = 1, WAFER_GS_SCALE = 2, WAFER_GS_AXPY = 3 };

struct WaferBatchGsArgs {
    WaferGeom g;
    int ntx, nty;               // tiles of 64 x 4 work cells per plane
    int flip;                   // the wavefunction of member m is phi[m.cur ^ flip]
    int scal_stride;            // doubles per member in scal
    int coef_slot;              // SCALE: norm2 at scal[member * scal_stride + coef_slot]; AXPY: the overlap with `lower`
    long long mstride;          // elements per member in a store slot's allocation
    const void *lower;          // AXPY: the state to project out (member 0's logical pointer, of the storage type), else unused
    const void *dotwith;        // DOT, SCALE, AXPY: the state whose overlap with the resulting phi is summed; null: none
};

// workgroups per member
static inline int wafer_gs_blocks(const WaferGeom &g)
{
    const int ntx = (g.nx + WAFER_BATCH_TX - 1) / WAFER_BATCH_TX, nty = (g.ny + WAFER_BATCH_TY - 1) / WAFER_BATCH_TY;
    return ntx * nty * ((g.nzl + WAFER_GS_ZC - 1) / WAFER_GS_ZC);
}

// Block (64, 4), grid (wafer_gs_blocks, active members).
template <int MODE, typename T = double>
__global__ __launch_bounds__(256) void wafer_k_batch_gs(WaferBatchGsArgs a, const WaferBatchMember *__restrict__ mem,
                                                        const int *__restrict__ act, const double *__restrict__ scal,
                                                        double *__restrict__ partials)
{
    __shared__ double red[4];
    const WaferGeom &g = a.g;
    const int member = act[blockIdx.y];
    const WaferBatchMember &m = mem[member];
    T *__restrict__ phi = static_cast<T *>(m.phi[(m.cur ^ a.flip) & 1]);
    const long long moff = (long long)member * a.mstride;
    const T *__restrict__ lower = (MODE == WAFER_GS_AXPY) ? static_cast<const T *>(a.lower) + moff : nullptr;
    const T *__restrict__ dotw = (MODE != WAFER_GS_NORM2 && a.dotwith) ? static_cast<const T *>(a.dotwith) + moff : nullptr;
    const int bid = blockIdx.x;
    const int i = (bid % a.ntx) * WAFER_BATCH_TX + threadIdx.x;
    const int j = ((bid / a.ntx) % a.nty) * WAFER_BATCH_TY + threadIdx.y;
    const int z0 = g.G + (bid / (a.ntx * a.nty)) * WAFER_GS_ZC;
    const int tid = threadIdx.y * WAFER_BATCH_TX + threadIdx.x;
    double coef = 0.0;
    if (MODE == WAFER_GS_SCALE) coef = sqrt(scal[(size_t)member * a.scal_stride + a.coef_slot]);
    if (MODE == WAFER_GS_AXPY) coef = scal[(size_t)member * a.scal_stride + a.coef_slot];
    double acc = 0.0;
    if (i < g.nx && j < g.ny) {
        const long long col = (long long)(j + g.R) * g.pitch + g.xoff + (i + g.R);
        double w[WAFER_GS_ZC], l[WAFER_GS_ZC], d[WAFER_GS_ZC];
#pragma unroll
        for (int k = 0; k < WAFER_GS_ZC; ++k) {
            const bool in = z0 + k < g.G + g.nzl;
            const long long p = col + (long long)(z0 + k) * g.plane;
            w[k] = in ? (double)phi[p] : 0.0;
            l[k] = (in && MODE == WAFER_GS_AXPY) ? (double)__builtin_nontemporal_load(lower + p) : 0.0;
            d[k] = (in && dotw) ? (double)__builtin_nontemporal_load(dotw + p) : 0.0;
        }
#pragma unroll
        for (int k = 0; k < WAFER_GS_ZC; ++k) {
            const bool in = z0 + k < g.G + g.nzl;
            const long long p = col + (long long)(z0 + k) * g.plane;
            double x = w[k];
            if (MODE == WAFER_GS_SCALE) x = wafer_div_invariant<double>(x, coef);   // grid.rs:467
            if (MODE == WAFER_GS_AXPY) x = x - l[k] * coef;                         // grid.rs:488-490
            if constexpr (MODE >= WAFER_GS_SCALE && !std::is_same_v<T, double>) x = (double)(T)x;   // what the array will hold
            if (MODE >= WAFER_GS_SCALE && in) phi[p] = (T)x;
            if (!in) continue;
            if (MODE == WAFER_GS_NORM2) acc += x * x;                               // grid.rs:454-457
            else acc += d[k] * x;                                                   // grid.rs:482-487
        }
    }
    if (MODE == WAFER_GS_NORM2 || a.dotwith) {   // (uniform: a kernel argument)
        const double s = wafer_block_sum<4>(acc, red, tid);
        if (tid == 0) partials[(size_t)member * gridDim.x + blockIdx.x] = s;
    }
}

// wafer_k_reduce for every active member at once: block `slot` sums the n partials of member act[slot] in wafer_k_reduce's
// order into scal[member * scal_stride + out_slot].
static __global__ __launch_bounds__(256) void wafer_k_batch_gs_reduce(const double *__restrict__ partials, const int *__restrict__ act,
                                                                      int n, double *__restrict__ scal, int scal_stride, int out_slot)
{
    __shared__ double sh[256];
    const int member = act[blockIdx.x];
    const double *p = partials + (size_t)member * n;
    double s = 0.0;
    for (int q = threadIdx.x; q < n; q += 256) s += p[q];
    sh[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) scal[(size_t)member * scal_stride + out_slot] = sh[0];
}

// wafer_batch_norm2 on float storage: get_norm_squared on the partition of a single context's wafer_norm2 -- wafer_k_row_op<T, double, 0>
// (wafer_elementwise.hip.h) on the row walk, four waves per workgroup, 16 bytes per lane, gridDim.x = wafer_rownorm2_blocks workgroups
// per member, each lane adding the squares of its cells in the same order, the same wafer_block_sum, one partial per workgroup at
// partials[member * gridDim.x + workgroup]; wafer_k_batch_gs_reduce then sums them in wafer_k_reduce's order.  So the double is
// the one wafer_norm2 returns for a context of that dtype.  The partition follows the shape, the element size and the device's CU
// count: nothing of the batch (B, index, active set).  Grid (wafer_rownorm2_blocks, members), block 256.
static inline int wafer_rownorm2_blocks(const WaferGeom &g, int esz, int num_cus)   // launch_row_op's grid (wafer_engine_schedules.hip)
{
    const long long segs = (long long)g.nzl * g.ny * ((g.nx + 1024 / esz - 1) / (1024 / esz));
    const long long nb = (long long)num_cus * 8 < (segs + 3) / 4 ? (long long)num_cus * 8 : (segs + 3) / 4;
    return (int)(nb > 1 ? nb : 1);
}

template <typename T>
__global__ __launch_bounds__(256) void wafer_k_batch_rownorm2(WaferRowArgs a, const WaferBatchMember *__restrict__ mem,
                                                              const int *__restrict__ act, double *__restrict__ partials)
{
    using VT = typename WaferRowVec<T>::type;
    constexpr int VEC = WaferRowVec<T>::N;
    __shared__ double red[4];
    const WaferGeom &g = a.g;
    const int member = act[blockIdx.y];
    const WaferBatchMember &m = mem[member];
    const T *__restrict__ phi = static_cast<const T *>(m.phi[m.cur]);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nsegx = (g.nx + 64 * VEC - 1) / (64 * VEC);
    const int wlim = g.pitch - g.xoff - g.R;
    double acc = 0.0;
    WAFER_ROW_WALK_BEGIN(a, g)
    for (int xs = 0; xs < nsegx; ++xs) {
        const int xi = xs * 64 * VEC + lane * VEC;
        if (xi >= wlim || xi >= g.nx) continue;
        const VT w = *reinterpret_cast<const VT *>(phi + rowp + xi);   // (whole 16 bytes: the row's pad cells exist, xi < wlim)
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            if (xi + v < g.nx) acc += (double)w[v] * (double)w[v];
    }
    WAFER_ROW_WALK_END(g)
    const double s = wafer_block_sum<4>(acc, red, threadIdx.x);
    if (threadIdx.x == 0) partials[(size_t)member * gridDim.x + blockIdx.x] = s;
}

// entry points (wafer_tu_gs_batch.hip).  One elementwise launch of `mode` over the active members and, where it sums
// (NORM2, or dotwith given), the reduce into scal[member * scal_stride + out_slot].  f32: float storage.
hipError_t wafer_entry_batch_gs(bool f32, int mode, const WaferBatchGsArgs &a, const WaferBatchMember *mem, const int *act, int nact,
                                double *scal, int out_slot, double *partials, hipStream_t s);
// float storage: norm2 of the members in act into scal[member * scal_stride + out_slot] on the single context's partition (nb =
// wafer_rownorm2_blocks workgroups per member; partials holds nb doubles per member of the batch)
hipError_t wafer_entry_batch_rownorm2(const WaferGeom &g, const WaferBatchMember *mem, const int *act, int nact, int nb, double *scal,
                                      int scal_stride, int out_slot, double *partials, hipStream_t s);
