// Stepping the state stores of a batch (wafer_batch_evolve_states): one launch advances states 0 .. k[m] - 1 of every listed member by
// one plain imaginary-time step -- no projection, no normalisation -- from one set of slot allocations into another (the store's
// slots and their shadows, ping-pong; the host ends a call of an odd number of steps with one batched copy back into the slots).
//
// Parity: after n launches a state holds, bit for bit, what phi of a single context of the member's wafer_params holds after
// wafer_evolve(ctx, 0, n) had phi started as that state.  The per-state text is wafer_k_batch_step's, call for call: one work cell
// per lane of a 64 x 4 tile, a z-queue of 2R+1 planes in registers, x and y neighbours from global memory, wafer_stencil_sum, then
// wafer_update with a, b from wafer_ab_from_v -- operation for operation wafer_update_v (wafer_stencil_fused2.hip.h), which is what
// every ground-state kernel of the engine rounds like.
//
// What is new: a workgroup steps up to WAFER_STORE_SG states of its tile, and V is loaded and a, b are formed ONCE per cell for all
// of them -- the reciprocal and its products are not repeated per state and V's bytes are read once per cell and group.  The grid is
// (workgroup table, groups): group blockIdx.y holds states [SG blockIdx.y, SG blockIdx.y + SG) of the entry's member, and a group
// at or beyond the member's k leaves as a whole before any load.  SG = 4: the queues of four states are 4 (2R+1) values per lane --
// 56 VGPRs for SevenPoint in fp64, the largest case -- and with the neighbour loads the compiler keeps in flight every instantiation
// stays free of scratch at 64 .. 166 VGPRs, three to eight waves per SIMD (the table in DESIGN.md section 5); a member with k = 8 is
// two groups.  All eight states in one workgroup would put SevenPoint's queues alone at 112 VGPRs.
// The state pointers come from two argument blocks (WaferRitzPtrs: the slot allocations, as wafer_k_batch_ritz_sums takes them) by
// select chains on the workgroup-uniform group index, and every loop over the group's states is fully unrolled with a uniform
// q < nq test: no private array is indexed at run time.
#pragma once
#include <hip/hip_runtime.h>
#include "wafer_geom.h"
#include "wafer_batch_plan.h"
#include "wafer_stencil.hip.h"
#include "wafer_stencil_fused2.hip.h"
#include "wafer_stencil_batch.hip.h"
#include "wafer_ritz.hip.h"
#include "wafer_ritz_batch.hip.h"

static_assert(WAFER_RITZ_MAX % WAFER_STORE_SG == 0, "whole groups");

// state SG * grp + q of an argument block, by a select chain over the groups (grp is workgroup-uniform)
template <int Q>
__device__ __forceinline__ void *wafer_store_ptr(const WaferRitzPtrs &st, int grp)
{
    void *p = st.p[Q];
#pragma unroll
    for (int gi = 1; gi < WAFER_RITZ_MAX / WAFER_STORE_SG; ++gi)
        if (grp == gi) p = st.p[gi * WAFER_STORE_SG + Q];
    return p;
}

// One time step of states [SG blockIdx.y, ...) below kk[member] of every entry's member: src -> dst (slot allocations; a member's
// states begin at its slot_off).  Block (64, 4), the table of wafer_batch_step_table over the listed members with k > 0.
template <int R, typename T = double, typename C = double, typename GS = WaferGeom>
__global__ __launch_bounds__(256) void wafer_k_batch_store_step(GS gs, const WaferBatchMember *__restrict__ mem,
                                                                const WaferBatchBlock *__restrict__ blocks, const int *__restrict__ kk,
                                                                WaferRitzPtrs src, WaferRitzPtrs dst)
{
    constexpr int SG = WAFER_STORE_SG, NQ = 2 * R + 1;
    const WaferBatchBlock bk = blocks[blockIdx.x];
    const int grp = blockIdx.y;
    const int nq = __builtin_amdgcn_readfirstlane(kk[bk.member]) - grp * SG;   // this group's states: 1 .. SG, or none
    if (nq <= 0) return;
    const WaferGeom &g = wafer_batch_geom(gs, bk.shape);
    const WaferBatchMember &m = mem[bk.member];
    const T *__restrict__ pv = static_cast<const T *>(m.v);
    const int i = bk.x0 + threadIdx.x;
    const int j = bk.y0 + threadIdx.y;
    if (i >= g.nx || j >= g.ny) return;
    const bool sf = m.short_forms != 0;   // (a scalar load: the branches it selects are scalar too)
    const WaferDen<C> den = wafer_batch_den<C>(m, sf);
    const C dt = (C)m.dt;
    const long long col = (long long)(j + R) * g.pitch + g.xoff + (i + R);
    const long long moff = m.slot_off + col;
    const T *__restrict__ p0 = static_cast<const T *>(wafer_store_ptr<0>(src, grp)) + moff;
    const T *__restrict__ p1 = static_cast<const T *>(wafer_store_ptr<1>(src, grp)) + moff;
    const T *__restrict__ p2 = static_cast<const T *>(wafer_store_ptr<2>(src, grp)) + moff;
    const T *__restrict__ p3 = static_cast<const T *>(wafer_store_ptr<3>(src, grp)) + moff;
    T *__restrict__ o0 = static_cast<T *>(wafer_store_ptr<0>(dst, grp)) + moff;
    T *__restrict__ o1 = static_cast<T *>(wafer_store_ptr<1>(dst, grp)) + moff;
    T *__restrict__ o2 = static_cast<T *>(wafer_store_ptr<2>(dst, grp)) + moff;
    T *__restrict__ o3 = static_cast<T *>(wafer_store_ptr<3>(dst, grp)) + moff;
    static_assert(SG == 4, "the four pointer pairs above");
    const T *const p[SG] = {p0, p1, p2, p3};   // (constant indices only, below: registers)
    T *const o[SG] = {o0, o1, o2, o3};
    C zq[SG][NQ];
#pragma unroll
    for (int q = 0; q < SG; ++q)
        if (q < nq) {
#pragma unroll
            for (int d = 1; d <= 2 * R; ++d) zq[q][d] = (C)p[q][(long long)(bk.z0 + d - 1 - R) * g.plane];
        }
    for (int z = bk.z0; z < bk.z1; ++z) {
        const long long zo = (long long)z * g.plane;
        C ca, cb;
        wafer_ab_from_v<C>((C)pv[col + zo], dt, sf, ca, cb);   // once per cell, for every state of the group
#pragma unroll
        for (int q = 0; q < SG; ++q)
            if (q < nq) {
#pragma unroll
                for (int d = 0; d < 2 * R; ++d) zq[q][d] = zq[q][d + 1];
                zq[q][2 * R] = (C)p[q][zo + (long long)R * g.plane];
                C xs[NQ], ys[NQ];
#pragma unroll
                for (int d = -R; d <= R; ++d) {
                    xs[d + R] = (d == 0) ? zq[q][R] : (C)p[q][zo + d];
                    ys[d + R] = (d == 0) ? zq[q][R] : (C)p[q][zo + (long long)d * g.pitch];
                }
                const C w = zq[q][R];
                const C S = wafer_stencil_sum<C, R>(xs, ys, zq[q], w);
                o[q][zo] = (T)wafer_update<C>(w, ca, cb, dt, S, den);
            }
    }
}

// The listed members' first k states from one set of slot allocations into another, over every 16-byte vector of the member's span
// (WaferBatchRitzRec: v0, n16) -- work cells, frame, pad and guard cells alike, which are zeros in both.  Grid (blocks, listed members).
static __global__ __launch_bounds__(256) void wafer_k_batch_store_copy(const WaferBatchRitzRec *__restrict__ act, WaferRitzPtrs src, WaferRitzPtrs dst)
{
    constexpr int KM = WAFER_RITZ_MAX;
    using VT = WaferVec<double>::type;   // 16 bytes, whatever the store holds
    const int k = act[blockIdx.y].k;
    const long long v0 = act[blockIdx.y].v0, n16 = act[blockIdx.y].n16;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n16; q += (long long)gridDim.x * 256) {
#pragma unroll
        for (int j = 0; j < KM; ++j)
            if (j < k) static_cast<VT *>(dst.p[j])[v0 + q] = static_cast<const VT *>(src.p[j])[v0 + q];
    }
}

// entry points (wafer_tu_store_step_batch.hip / wafer_tu_store_step_batch_mixed.hip), the step once per geometry source GS like
// WAFER_BATCH_ENTRIES.  dtype: 0 f64 <double, double>, 1 f32 <float, double>, 2 f32fast <float, float>.  groups: the grid's extent
// along y, ceil(largest k / WAFER_STORE_SG).  copy: one launch of `blocks` x nact workgroups.
#define WAFER_BATCH_STORE_ENTRIES(GS)                                                                                                                \
    hipError_t wafer_entry_batch_store_step(int dtype, int R, const GS &gs, const WaferBatchMember *mem, const WaferBatchBlock *blocks, int nblocks, \
                                            int groups, const int *kk, const WaferRitzPtrs &src, const WaferRitzPtrs &dst, hipStream_t s);
WAFER_BATCH_STORE_ENTRIES(WaferGeom)
WAFER_BATCH_STORE_ENTRIES(WaferBatchGeomTable)
#undef WAFER_BATCH_STORE_ENTRIES
hipError_t wafer_entry_batch_store_copy(const WaferBatchRitzRec *act, int nact, int blocks, const WaferRitzPtrs &src, const WaferRitzPtrs &dst,
                                        hipStream_t s);
