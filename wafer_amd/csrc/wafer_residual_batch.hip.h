// Residual sums of every listed member of a batch (wafer_batch_residuals): the single context's sums (wafer_residual.hip.h) for all
// listed members in one launch, whatever their number and shapes, over the member table as wafer_ritz_batch.hip.h does for Ritz.
//   wafer_k_batch_residual_sums    grid (largest obs_nb, largest k, listed members): the workgroups' r2, wh, s of column j
//   wafer_k_batch_residual_reduce  grid (3 WAFER_RITZ_MAX, listed members): every member's 3 k sums
//
// Parity: a member gets the bits a wafer_ctx of its wafer_params gets from wafer_residuals on the same source, potential and theta.
// The sums run on the member's own observables partition (WaferBatchMember::obs_*), the per-cell body is the context kernel's own
// text (wafer_residual_cells), the block sums and the places within a row are the same, and the reduce is wafer_k_reduce's order
// (wafer_batch_reduce_tree).  Nothing a sum sees depends on the number of members, the member's index or the listed set.  No
// floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>
#include "wafer_geom.h"
#include "wafer_stencil.hip.h"
#include "wafer_stencil_batch.hip.h"
#include "wafer_residual.hip.h"

// One listed member of a call (the per-call table, one small pinned upload): the member, its k, where its 3 k rows of obs_nb
// partials begin (the prefix sum over the listed members before it), and theta of each of its columns.
struct WaferBatchResidualRec {
    int member;
    int k;
    long long poff;   // doubles
    double theta[WAFER_RITZ_MAX];
};

// wafer_k_residual_sums for the member act[blockIdx.z].member and the column blockIdx.y of its k.  phi != 0: the source is the
// member's current wavefunction (k == 1); else stored state j, the slot allocation st.p[j] plus the member's slot_off.  A workgroup
// beyond the member's partition or beyond its k leaves as a whole before any load or barrier.
// partials[poff + (j * 3 + q) * obs_nb + workgroup] = r2 (q = 0), wh (1), s (2).
template <int R, int NW, typename T, typename GS>
__global__ __launch_bounds__(NW * 64) void wafer_k_batch_residual_sums(GS gs, const WaferBatchMember *__restrict__ mem,
                                                                       const WaferBatchResidualRec *__restrict__ act, int swz, int phi,
                                                                       WaferRitzPtrs st, double *__restrict__ partials)
{
    static_assert(NW == WaferRitzCfg<R>::NW, "the context's waves per workgroup");
    using Tile = WaferResidualTile<R, T>;
    constexpr int KM = WAFER_RITZ_MAX;
    __shared__ double red[NW];
    const WaferBatchResidualRec &rec = act[blockIdx.z];
    const int member = rec.member, k = rec.k;
    const long long poff = rec.poff;
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
    const int xi = tx_i * Tile::TX + lane * Tile::VEC;   // work-x of the lane's first cell
    const int yw = ty_i * Tile::TY + wave * Tile::RY;    // work-y of the lane's first row
    const int zs = g.G + tz_i * zchunk;
    const int ze = min(zs + zchunk, g.G + g.nzl);
    // the column's source and theta, by select chains (an index into the argument block or the record would be a private array)
    const T *__restrict__ lj = static_cast<const T *>(st.p[0]);
    double th = rec.theta[0];
#pragma unroll
    for (int i = 1; i < KM; ++i)
        if (j == i) {
            lj = static_cast<const T *>(st.p[i]);
            th = rec.theta[i];
        }
    if (phi) lj = static_cast<const T *>(m.cur ? m.phi[1] : m.phi[0]);
    else lj += m.slot_off;
    const WaferDen<double> den{m.den, m.zh, m.zl, m.short_forms != 0};

    double r2 = 0.0, wh = 0.0, s = 0.0;
    wafer_residual_cells<R, T, WAFER_CELLS_SUMS>(g, xi, yw, zs, ze, lj, static_cast<const T *>(m.v), den, th, nullptr, r2, wh, s);
    const double r2s = wafer_block_sum<NW>(r2, red, tid);
    if (tid == 0) partials[(size_t)poff + (size_t)(j * 3 + 0) * nb + blockIdx.x] = r2s;
    const double whs = wafer_block_sum<NW>(wh, red, tid);
    if (tid == 0) partials[(size_t)poff + (size_t)(j * 3 + 1) * nb + blockIdx.x] = whs;
    const double ss = wafer_block_sum<NW>(s, red, tid);
    if (tid == 0) partials[(size_t)poff + (size_t)(j * 3 + 2) * nb + blockIdx.x] = ss;
}

// wafer_k_reduce for every listed member and row at once: block (row, slot) sums the obs_nb partials of row `row` = j * 3 + q of
// member act[slot] in wafer_k_reduce's order; rows beyond 3 k leave.  out[member * 3 WAFER_RITZ_MAX + row] = the sum.
static __global__ __launch_bounds__(256) void wafer_k_batch_residual_reduce(const double *__restrict__ partials,
                                                                            const WaferBatchResidualRec *__restrict__ act,
                                                                            const WaferBatchMember *__restrict__ mem, double *__restrict__ out)
{
    __shared__ double sh[256];
    const int member = act[blockIdx.y].member, k = act[blockIdx.y].k;
    const int row = blockIdx.x;
    if (row >= 3 * k) return;
    const long long n = mem[member].obs_nb;
    const double s = wafer_batch_reduce_tree(partials + act[blockIdx.y].poff + (long long)row * n, n, sh);
    if (threadIdx.x == 0) out[(size_t)member * 3 * WAFER_RITZ_MAX + row] = s;
}

// entry point (wafer_tu_residual_batch.hip), once per geometry source GS like WAFER_BATCH_ENTRIES.  f32: float storage.  The sums
// launch over the nact members in act (max_nb, max_k: the largest obs_nb and k among them) and the reduce into sums
// ([member][3 WAFER_RITZ_MAX]).
#define WAFER_BATCH_RESIDUAL_ENTRIES(GS)                                                                                                             \
    hipError_t wafer_entry_batch_residual_sums(bool f32, int R, const GS &gs, const WaferBatchMember *mem, const WaferBatchResidualRec *act,         \
                                               int nact, int max_nb, int max_k, int swz, int phi, const WaferRitzPtrs &st, double *partials,        \
                                               double *sums, hipStream_t s);
WAFER_BATCH_RESIDUAL_ENTRIES(WaferGeom)
WAFER_BATCH_RESIDUAL_ENTRIES(WaferBatchGeomTable)
#undef WAFER_BATCH_RESIDUAL_ENTRIES
