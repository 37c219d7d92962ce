// Filtering the state stores of a batch (wafer_batch_filter_states): one launch applies one step of the three-term recurrence of a
// scaled Chebyshev polynomial in H itself (wafer_filter.h) to states 0 .. k[m] - 1 of every listed member.
//
// Per work cell c, fp64 and unfused whatever the storage type T (double, or float for f32 and f32fast), operands widened from T:
//   w  = cur[c]          vv = V[c]
//   S  = wafer_stencil_sum<double, R>(neighbours of cur at c, frame cells as stored)
//   q  = wafer_div_invariant<double>(S, den)          hw = vv * w - q          t = hw - cc * w          y = al * t
//   not first:  y = y - be * prev[c]                  out[c] = (T)y            (work cells only)
// -- the per-cell text of wafer_residual_cells' filter modes (wafer_residual.hip.h), so a one-member batch and a context hold the
// same bits after the same call.  prev is read at the lane's own cell only, so out IS prev's array: the new iterate goes over the
// one before last, in place, prev[c] loaded before the store; cur and out are never marked __restrict__ against prev.
//
// The shape is wafer_k_batch_store_step's (wafer_store_step_batch.hip.h): the one-step workgroup table over the listed members with
// k > 0, block 64 x 4, one work cell per lane marching its z-chunk with a register queue of 2R+1 planes per state, groups of
// WAFER_STORE_SG states on blockIdx.y, the state pointers by select chains on the group index, every loop over the group's states
// unrolled with a uniform q < nq test.  V's load and the member's al, be, cc -- this step's, from a per-call device table indexed by
// member -- are shared by the group's states.
#pragma once
#include <hip/hip_runtime.h>
#include "wafer_geom.h"
#include "wafer_batch_plan.h"
#include "wafer_filter.h"
#include "wafer_stencil.hip.h"
#include "wafer_stencil_batch.hip.h"
#include "wafer_ritz.hip.h"
#include "wafer_residual.hip.h"
#include "wafer_store_step_batch.hip.h"

// One filter step of states [SG blockIdx.y, ...) below kk[member] of every entry's member: cur -> out (slot allocations; a member's
// states begin at its slot_off).  coef[member]: the member's al, be, cc of this step.  first: the recurrence's step 1 (workgroup-
// uniform): prev is neither loaded nor subtracted.
template <int R, typename T = double, typename GS = WaferGeom>
__global__ __launch_bounds__(256) void wafer_k_batch_store_filter(GS gs, const WaferBatchMember *__restrict__ mem,
                                                                  const WaferBatchBlock *__restrict__ blocks, const int *__restrict__ kk,
                                                                  const WaferFilterCoef *__restrict__ coef, int first, WaferRitzPtrs cur,
                                                                  WaferRitzPtrs out)
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
    const WaferDen<double> den{m.den, m.zh, m.zl, m.short_forms != 0};
    const double al = coef[bk.member].al, be = coef[bk.member].be, cc = coef[bk.member].cc;   // (scalar loads)
    const long long col = (long long)(j + R) * g.pitch + g.xoff + (i + R);
    const long long moff = m.slot_off + col;
    const T *p0 = static_cast<const T *>(wafer_store_ptr<0>(cur, grp)) + moff;
    const T *p1 = static_cast<const T *>(wafer_store_ptr<1>(cur, grp)) + moff;
    const T *p2 = static_cast<const T *>(wafer_store_ptr<2>(cur, grp)) + moff;
    const T *p3 = static_cast<const T *>(wafer_store_ptr<3>(cur, grp)) + moff;
    T *o0 = static_cast<T *>(wafer_store_ptr<0>(out, grp)) + moff;
    T *o1 = static_cast<T *>(wafer_store_ptr<1>(out, grp)) + moff;
    T *o2 = static_cast<T *>(wafer_store_ptr<2>(out, grp)) + moff;
    T *o3 = static_cast<T *>(wafer_store_ptr<3>(out, grp)) + moff;
    static_assert(SG == 4, "the four pointer pairs above");
    const T *const p[SG] = {p0, p1, p2, p3};   // (constant indices only, below: registers)
    T *const o[SG] = {o0, o1, o2, o3};
    double zq[SG][NQ];
#pragma unroll
    for (int q = 0; q < SG; ++q)
        if (q < nq) {
#pragma unroll
            for (int d = 1; d <= 2 * R; ++d) zq[q][d] = (double)p[q][(long long)(bk.z0 + d - 1 - R) * g.plane];
        }
    for (int z = bk.z0; z < bk.z1; ++z) {
        const long long zo = (long long)z * g.plane;
        const double vv = (double)pv[col + zo];   // once per cell, for every state of the group
#pragma unroll
        for (int q = 0; q < SG; ++q)
            if (q < nq) {
#pragma unroll
                for (int d = 0; d < 2 * R; ++d) zq[q][d] = zq[q][d + 1];
                zq[q][2 * R] = (double)p[q][zo + (long long)R * g.plane];
                double xs[NQ], ys[NQ];
#pragma unroll
                for (int d = -R; d <= R; ++d) {
                    xs[d + R] = (d == 0) ? zq[q][R] : (double)p[q][zo + d];
                    ys[d + R] = (d == 0) ? zq[q][R] : (double)p[q][zo + (long long)d * g.pitch];
                }
                const double w = zq[q][R];
                const double S = wafer_stencil_sum<double, R>(xs, ys, zq[q], w);
                const double qd = wafer_div_invariant<double>(S, den);
                const double hw = vv * w - qd;
                const double t = hw - cc * w;
                double y = al * t;
                if (!first) y = y - be * (double)o[q][zo];   // prev[c], before the store below
                o[q][zo] = (T)y;
            }
    }
}

// The largest V over the work cells of every member in act (wafer_batch_spectral_bound): wafer_v_max_tile (wafer_residual.hip.h)
// for member act[blockIdx.z] into words[blockIdx.z].  Grid (largest tile count, largest plane count, listed members).
template <typename T, typename GS>
__global__ __launch_bounds__(256) void wafer_k_batch_v_max(GS gs, const WaferBatchMember *__restrict__ mem, const int *__restrict__ act,
                                                           unsigned long long *__restrict__ words)
{
    const WaferBatchMember &m = mem[__builtin_amdgcn_readfirstlane(act[blockIdx.z])];
    const WaferGeom &g = wafer_batch_geom(gs, m.shape);
    wafer_v_max_tile<T>(g, static_cast<const T *>(m.v), blockIdx.x, blockIdx.y, words + blockIdx.z);
}

// entry points (wafer_tu_store_filter_batch.hip / wafer_tu_store_filter_batch_mixed.hip), once per geometry source GS like
// WAFER_BATCH_STORE_ENTRIES.  f32: float storage (f32 and f32fast alike: the arithmetic is fp64).  groups: the grid's extent along
// y, ceil(largest k / WAFER_STORE_SG).  v_max: nact members in act, max_tiles x max_planes 64 x 4 tiles of their work boxes.
#define WAFER_BATCH_FILTER_ENTRIES(GS)                                                                                                                \
    hipError_t wafer_entry_batch_store_filter(bool f32, int R, const GS &gs, const WaferBatchMember *mem, const WaferBatchBlock *blocks, int nblocks, \
                                              int groups, const int *kk, const WaferFilterCoef *coef, int first, const WaferRitzPtrs &cur,           \
                                              const WaferRitzPtrs &out, hipStream_t s);                                                               \
    hipError_t wafer_entry_batch_v_max(bool f32, const GS &gs, const WaferBatchMember *mem, const int *act, int nact, int max_tiles, int max_planes,  \
                                       unsigned long long *words, hipStream_t s);
WAFER_BATCH_FILTER_ENTRIES(WaferGeom)
WAFER_BATCH_FILTER_ENTRIES(WaferBatchGeomTable)
#undef WAFER_BATCH_FILTER_ENTRIES
