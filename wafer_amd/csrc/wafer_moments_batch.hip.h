// Moment matrices of the stored states of every listed member of a batch (wafer_batch_moment_matrices): the single context's sums
// (wafer_moments.hip.h) for all listed members in one launch, whatever their number and shapes.
//   wafer_k_batch_moment_sums    grid (largest obs_nb, largest k, listed members): the workgroups' sums of column j, i <= j
//   wafer_k_batch_moment_reduce  grid (5 WAFER_RITZ_MAX (WAFER_RITZ_MAX + 1) / 2, listed members): every member's computed rows
//   one read-back; the host mirrors the entries i > j
//
// Parity: a member gets the bits a wafer_ctx of its wafer_params gets from wafer_moment_matrices on the same states.  The sums run
// on the member's own observables partition (WaferBatchMember::obs_*), the per-cell body is the context kernel's own text
// (wafer_moment_cells) with the centres of the member's own nx, ny, nz, the block sums and the places within a row are the same,
// and the reduce is wafer_k_reduce's order (wafer_batch_reduce_tree).  Nothing a sum sees depends on the number of members, the
// member's index or the listed set.  No floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>
#include "wafer_geom.h"
#include "wafer_stencil.hip.h"
#include "wafer_stencil_batch.hip.h"
#include "wafer_moments.hip.h"

// One listed member of a call (the per-call table, one small pinned upload): the member, its k and where its 5 k (k + 1) / 2 rows
// of obs_nb partials begin (the prefix sum over the listed members before it).
struct WaferBatchMomentRec {
    int member;
    int k;
    long long poff;   // doubles
};

// wafer_k_moment_sums for the member act[blockIdx.z].member and the column blockIdx.y of its k.  The geometry comes through
// wafer_batch_geom, the states are the slot allocations in st plus the member's slot_off, and the swizzle takes the member's own
// obs_nb as its extent.  A workgroup beyond the member's partition or beyond its k leaves as a whole before any load or barrier.
// partials[poff + (q * k (k + 1) / 2 + j (j + 1) / 2 + i) * obs_nb + workgroup]
template <int R, int NW, typename T, typename GS>
__global__ __launch_bounds__(NW * 64) void wafer_k_batch_moment_sums(GS gs, const WaferBatchMember *__restrict__ mem,
                                                                     const WaferBatchMomentRec *__restrict__ act, int swz, WaferRitzPtrs st,
                                                                     double *__restrict__ partials)
{
    static_assert(NW == WaferRitzCfg<R>::NW, "the context's waves per workgroup");
    constexpr int RY = 2, KM = WAFER_RITZ_MAX;
    constexpr int VEC = WaferVec<T>::N, TX = 64 * VEC, TY = NW * RY;
    __shared__ double red[NW];
    const int member = act[blockIdx.z].member, k = act[blockIdx.z].k;
    const long long poff = act[blockIdx.z].poff;
    const WaferBatchMember &m = mem[member];
    const int nb = m.obs_nb;
    const int j = blockIdx.y;
    if ((int)blockIdx.x >= nb || j >= k) return;
    const WaferGeom &g = wafer_batch_geom(gs, m.shape);
    const int ntx = m.obs_ntx, nty = m.obs_nty, zchunk = m.obs_zchunk;
    int bid = blockIdx.x;
    if (swz) bid = wafer_xcd_tile(bid, nb);
    const int tx_i = bid % ntx;
    const int ty_i = (bid / ntx) % nty;
    const int tz_i = bid / (ntx * nty);
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int xi = tx_i * TX + lane * VEC;      // work-x of the lane's first cell
    const int yw = ty_i * TY + wave * RY;       // work-y of the lane's first row
    const int zs = g.G + tz_i * zchunk;
    const int ze = min(zs + zchunk, g.G + g.nzl);
    const long long moff = m.slot_off;
    // the column's state, by a select chain (an index into the argument block would be a private array)
    const T *__restrict__ lj = static_cast<const T *>(st.p[0]);
#pragma unroll
    for (int i = 1; i < KM; ++i)
        if (j == i) lj = static_cast<const T *>(st.p[i]);
    lj += moff;
    double acc[WAFER_MOMENT_COUNT][KM];
#pragma unroll
    for (int q = 0; q < WAFER_MOMENT_COUNT; ++q)
#pragma unroll
        for (int i = 0; i < KM; ++i) acc[q][i] = 0.0;
    wafer_moment_cells<T>(g, xi, yw, zs, ze, j, lj, st, moff, acc);
    wafer_moment_store<NW>(acc, j, k, red, tid, partials, (size_t)poff, nb, (int)blockIdx.x);
}

// wafer_k_reduce for every listed member and computed row at once: block (row, slot) sums the obs_nb partials of row `row` of
// member act[slot] in wafer_k_reduce's order; rows beyond the member's 5 k (k + 1) / 2 leave.
// out[member * WAFER_MOMENT_COUNT * WAFER_RITZ_MAX^2 + row] = the sum (the host unpacks the triangles: wafer_moment_tri).
static __global__ __launch_bounds__(256) void wafer_k_batch_moment_reduce(const double *__restrict__ partials,
                                                                          const WaferBatchMomentRec *__restrict__ act,
                                                                          const WaferBatchMember *__restrict__ mem, double *__restrict__ out)
{
    constexpr int KK = WAFER_RITZ_MAX * WAFER_RITZ_MAX;
    __shared__ double sh[256];
    const int member = act[blockIdx.y].member, k = act[blockIdx.y].k;
    const int row = blockIdx.x;
    if (row >= wafer_moment_rows(k)) return;
    const long long n = mem[member].obs_nb;
    const double s = wafer_batch_reduce_tree(partials + act[blockIdx.y].poff + (long long)row * n, n, sh);
    if (threadIdx.x != 0) return;
    out[(size_t)member * WAFER_MOMENT_COUNT * KK + row] = s;
}

// entry points (wafer_tu_moments_batch.hip), once per geometry source GS like WAFER_BATCH_RITZ_ENTRIES.  f32: float storage.
// The sums launch over the nact members in act (max_nb, max_k: the largest obs_nb and k among them) and the reduce into sums
// ([member][WAFER_MOMENT_COUNT * WAFER_RITZ_MAX^2], the member's computed rows first).
#define WAFER_BATCH_MOMENT_ENTRIES(GS)                                                                                                               \
    hipError_t wafer_entry_batch_moment_sums(bool f32, int R, const GS &gs, const WaferBatchMember *mem, const WaferBatchMomentRec *act, int nact,   \
                                             int max_nb, int max_k, int swz, const WaferRitzPtrs &st, double *partials, double *sums, hipStream_t s);
WAFER_BATCH_MOMENT_ENTRIES(WaferGeom)
WAFER_BATCH_MOMENT_ENTRIES(WaferBatchGeomTable)
#undef WAFER_BATCH_MOMENT_ENTRIES
