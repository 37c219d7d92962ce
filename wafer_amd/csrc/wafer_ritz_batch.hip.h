// Rayleigh-Ritz on the stored states of every listed member of a batch (wafer_batch_ritz_matrices, wafer_batch_rotate_states,
// wafer_batch_ritz): the single context's sums and rotation (wafer_ritz.hip.h) for all listed members in one launch each, whatever
// their number and shapes.  Schedule of wafer_batch_ritz:
//   wafer_k_batch_ritz_sums     grid (largest obs_nb, largest k, listed members): the workgroups' h_i, s_i of column j
//   wafer_k_batch_ritz_reduce   grid (2 WAFER_RITZ_MAX^2, listed members): every member's 2 k^2 sums
//   one read-back, the solves on the host (wafer_ritz.h)
//   wafer_k_batch_rotate_states grid (blocks, members that solved)
//
// Parity: a member gets the bits a wafer_ctx of its wafer_params gets from wafer_ritz_matrices and wafer_rotate_states on the same
// states and potential.  The sums run on the member's own observables partition (WaferBatchMember::obs_*: the one
// ritz_sums_launch gives a context of that shape), the per-cell body is the context kernel's own text (wafer_ritz_cells), the block
// sums and the places within a row are the same, and the reduce is wafer_k_reduce's order (wafer_batch_reduce_tree).  The rotation
// forms every element from the same operands in the same order.  Nothing a sum sees depends on the number of members, the member's
// index or the listed set: those change blockIdx.z and the place of the member's partials only.  No floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>
#include "wafer_geom.h"
#include "wafer_stencil.hip.h"
#include "wafer_stencil_batch.hip.h"
#include "wafer_ritz.hip.h"

// One listed member of a call (the per-call table, one small pinned upload): the member, its k, where its 2 k^2 rows of obs_nb
// partials begin (the prefix sum over the listed members before it), and its span in a store slot's allocation -- the elements a
// context's allocation of its shape holds, work cells, frame, pad and guard cells -- in vectors of 16 bytes from the allocation's
// base (wafer_batch_layout checks that every span starts and ends on 16 bytes).
struct WaferBatchRitzRec {
    int member;
    int k;
    long long poff;   // doubles
    long long v0;     // the span's first vector
    long long n16;    // its vectors
};

// wafer_k_ritz_sums for the member act[blockIdx.z].member and the column blockIdx.y of its k.  The geometry comes through
// wafer_batch_geom, V, the denominator and the short-form flag from the member record, the states are the slot allocations in st
// plus the member's slot_off, and the swizzle takes the member's own obs_nb as its extent.  A workgroup beyond the member's
// partition or beyond its k leaves as a whole before any load or barrier.
// partials[poff + (j * k + i) * obs_nb + workgroup] = h_i, partials[poff + (k * k + j * k + i) * obs_nb + workgroup] = s_i.
template <int R, int NW, typename T, typename GS>
__global__ __launch_bounds__(NW * 64) void wafer_k_batch_ritz_sums(GS gs, const WaferBatchMember *__restrict__ mem,
                                                                   const WaferBatchRitzRec *__restrict__ act, int swz, WaferRitzPtrs st,
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
    const WaferDen<double> den{m.den, m.zh, m.zl, m.short_forms != 0};

    double h[KM], s[KM];
#pragma unroll
    for (int i = 0; i < KM; ++i) h[i] = s[i] = 0.0;
    wafer_ritz_cells<R, T>(g, xi, yw, zs, ze, k, lj, st, moff, static_cast<const T *>(m.v), den, h, s);
#pragma unroll
    for (int i = 0; i < KM; ++i)
        if (i < k) {   // k is workgroup-uniform: every wave reaches the same barriers
            const double hs = wafer_block_sum<NW>(h[i], red, tid);
            if (tid == 0) partials[(size_t)poff + (size_t)(j * k + i) * nb + blockIdx.x] = hs;
            const double ss = wafer_block_sum<NW>(s[i], red, tid);
            if (tid == 0) partials[(size_t)poff + (size_t)(k * k + j * k + i) * nb + blockIdx.x] = ss;
        }
}

// wafer_k_reduce for every listed member and row at once: block (row, slot) sums the obs_nb partials of row `row` of member
// act[slot] in wafer_k_reduce's order.  Rows [0, k^2) are h, [k^2, 2 k^2) are s; rows beyond leave.
// out[(member * 2 + 0) * WAFER_RITZ_MAX^2 + q] = h[q], out[(member * 2 + 1) * WAFER_RITZ_MAX^2 + q] = s[q], q < k^2.
static __global__ __launch_bounds__(256) void wafer_k_batch_ritz_reduce(const double *__restrict__ partials,
                                                                        const WaferBatchRitzRec *__restrict__ act,
                                                                        const WaferBatchMember *__restrict__ mem, double *__restrict__ out)
{
    constexpr int KK = WAFER_RITZ_MAX * WAFER_RITZ_MAX;
    __shared__ double sh[256];
    const int member = act[blockIdx.y].member, k = act[blockIdx.y].k;
    const int row = blockIdx.x;
    if (row >= 2 * k * k) return;
    const long long n = mem[member].obs_nb;
    const double s = wafer_batch_reduce_tree(partials + act[blockIdx.y].poff + (long long)row * n, n, sh);
    if (threadIdx.x != 0) return;
    const int which = row >= k * k ? 1 : 0;
    out[((size_t)member * 2 + which) * KK + (row - which * k * k)] = s;
}

// wafer_k_rotate_states for the members act[blockIdx.y]: l'_a = sum_j coef[j * k + a] l_j for the member's first k states, in place,
// over every vector of its span in the slot allocations st.p.  A thread loads its k vectors, then forms per output state
// acc = coef[0 * k + a] * l_0, acc = acc + coef[j * k + a] * l_j for j = 1 .. k-1 in that order (fp64, unfused) and stores (T)acc.
// coef: the member's k * k doubles at coefs + member * WAFER_RITZ_MAX^2.  No scalar tail: the span is whole vectors.
template <typename T>
__global__ __launch_bounds__(256) void wafer_k_batch_rotate_states(const WaferBatchRitzRec *__restrict__ act, WaferRitzPtrs st,
                                                                   const double *__restrict__ coefs)
{
    constexpr int KM = WAFER_RITZ_MAX;
    using VT = typename WaferVec<T>::type;
    constexpr int VEC = WaferVec<T>::N;
    const int k = act[blockIdx.y].k;
    const long long v0 = act[blockIdx.y].v0, n16 = act[blockIdx.y].n16;
    const double *__restrict__ coef = coefs + (size_t)act[blockIdx.y].member * (KM * KM);
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n16; q += (long long)gridDim.x * 256) {
        VT l[KM];
#pragma unroll
        for (int j = 0; j < KM; ++j)
            if (j < k) l[j] = static_cast<const VT *>(st.p[j])[v0 + q];
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
                static_cast<VT *>(st.p[a])[v0 + q] = o;
            }
    }
}

// entry points (wafer_tu_ritz_batch.hip), the sums once per geometry source GS like WAFER_BATCH_ENTRIES.  f32: float storage.
// ritz_sums: the sums launch over the nact members in act (max_nb, max_k: the largest obs_nb and k among them) and the reduce into
// sums ([member][2][WAFER_RITZ_MAX^2]).  rotate: one launch of `blocks` x nact workgroups; coefs: [member][WAFER_RITZ_MAX^2].
#define WAFER_BATCH_RITZ_ENTRIES(GS)                                                                                                                 \
    hipError_t wafer_entry_batch_ritz_sums(bool f32, int R, const GS &gs, const WaferBatchMember *mem, const WaferBatchRitzRec *act, int nact,       \
                                           int max_nb, int max_k, int swz, const WaferRitzPtrs &st, double *partials, double *sums, hipStream_t s);
WAFER_BATCH_RITZ_ENTRIES(WaferGeom)
WAFER_BATCH_RITZ_ENTRIES(WaferBatchGeomTable)
#undef WAFER_BATCH_RITZ_ENTRIES
hipError_t wafer_entry_batch_rotate_states(bool f32, const WaferBatchRitzRec *act, int nact, int blocks, const WaferRitzPtrs &st,
                                           const double *coefs, hipStream_t s);
