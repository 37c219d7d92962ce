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
// Determinism and independence: the partition of a member is fixed by its geometry alone -- tiles of 64 x 4 work cells, chunks
// of WAFER_GS_ZC planes, gs_nb workgroups, one partial per workgroup at partials[gs_off + workgroup] (one shape: gs_off ==
// member * gs_nb) -- and the reduce sums a member's gs_nb partials in wafer_k_reduce's order.  The grid is (the largest gs_nb
// among the launched members, active members): which other members run, how many there are and where the member sits in the
// batch change blockIdx.y and nothing a sum sees.  No floating-point atomics.
//
// One shape or several: the kernels take the geometry source GS first (wafer_batch_geom, wafer_stencil_batch.hip.h -- the one
// place the two instantiations differ) and everything that depends on the member from its WaferBatchMember record: gs_nb, gs_off,
// and slot_off, its logical origin in a store slot's allocation.  The slot pointers in the arguments are the ALLOCATIONS.
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
    int flip;                   // the wavefunction of member m is phi[m.cur ^ flip]
    int scal_stride;            // doubles per member in scal
    int coef_slot;              // SCALE: norm2 at scal[member * scal_stride + coef_slot]; AXPY: the overlap with `lower`
    const void *lower;          // AXPY: the store slot to project out (its allocation, of the storage type), else unused
    const void *dotwith;        // DOT, SCALE, AXPY: the store slot whose overlap with the resulting phi is summed; null: none
};

// workgroups per member
static inline int wafer_gs_blocks(const WaferGeom &g) { return wafer_gs_blocks_of(g, WAFER_BATCH_TX, WAFER_BATCH_TY, WAFER_GS_ZC); }

// What a workgroup of these kernels works on: the tile counts of its member's geometry and, from the member's record, its
// workgroup count, its place in a store slot and the start of its `rows` rows of partials (wafer_batch_gs_partition,
// wafer_batch_plan.h).  A partial of row q lies at p0 + q * nb + blockIdx.x.
struct WaferGsPart {
    int ntx, nty, nb;
    long long moff;   // the member's element offset from the slot pointers of the arguments
    size_t p0;
};
// A workgroup beyond its member's partition (blockIdx.x >= nb, on a grid as wide as a larger member needs) has its z-chunk past
// the member's last plane -- nb == ntx * nty * ceil(nzl / WAFER_GS_ZC), wafer_gs_blocks_of -- so the plane predicate `in` of the
// kernels below is false for each of its planes: it loads and stores no cell.  The summing kernels send it away as a whole with
// wafer_gs_beyond BEHIND that body: before the barrier of the block sum, and before it could write a partial outside its
// member's rows.  Not at the top: a test of the record's gs_nb there put the act -> record loads and a branch in front of
// everything else the prologue does (the geometry's loads, the tile divisions), two more dependent scalar round trips per
// workgroup, measured as +1 % per excited step of a one-shape batch of 32 x 64^3 ("One member addressing").
__device__ __forceinline__ void wafer_gs_part(const WaferGeom &g, const WaferBatchMember &m, int rows, WaferGsPart &w)
{
    w.ntx = (g.nx + WAFER_BATCH_TX - 1) / WAFER_BATCH_TX;
    w.nty = (g.ny + WAFER_BATCH_TY - 1) / WAFER_BATCH_TY;
    w.nb = m.gs_nb;
    w.moff = m.slot_off;
    w.p0 = (size_t)m.gs_off * rows;
}
__device__ __forceinline__ bool wafer_gs_beyond(const WaferGsPart &w) { return (int)blockIdx.x >= w.nb; }

// The wavefunction of member m at step parity `flip`, phi[(cur ^ flip) & 1]: both pointers are loaded beside cur and one is
// selected, where a load indexed by cur would be one more dependent scalar round trip in front of the workgroup's first vector load.
template <typename T>
__device__ __forceinline__ T *wafer_gs_phi(const WaferBatchMember &m, int flip)
{
    void *const p0 = m.phi[0], *const p1 = m.phi[1];
    return static_cast<T *>(((m.cur ^ flip) & 1) ? p1 : p0);
}

// Block (64, 4), grid (the largest gs_nb among the launched members, active members).
template <int MODE, typename T = double, typename GS = WaferGeom>
__global__ __launch_bounds__(256) void wafer_k_batch_gs(GS gs, WaferBatchGsArgs a, const WaferBatchMember *__restrict__ mem,
                                                        const int *__restrict__ act, const double *__restrict__ scal,
                                                        double *__restrict__ partials)
{
    __shared__ double red[4];
    const int member = act[blockIdx.y];
    const WaferBatchMember &m = mem[member];
    const WaferGeom &g = wafer_batch_geom(gs, m.shape);
    WaferGsPart wg;
    wafer_gs_part(g, m, 1, wg);
    T *__restrict__ phi = wafer_gs_phi<T>(m, a.flip);
    const long long moff = wg.moff;
    const T *__restrict__ lower = (MODE == WAFER_GS_AXPY) ? static_cast<const T *>(a.lower) + moff : nullptr;
    const T *__restrict__ dotw = (MODE != WAFER_GS_NORM2 && a.dotwith) ? static_cast<const T *>(a.dotwith) + moff : nullptr;
    const int bid = blockIdx.x;
    const int i = (bid % wg.ntx) * WAFER_BATCH_TX + threadIdx.x;
    const int j = ((bid / wg.ntx) % wg.nty) * WAFER_BATCH_TY + threadIdx.y;
    const int z0 = g.G + (bid / (wg.ntx * wg.nty)) * WAFER_GS_ZC;
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
    if (wafer_gs_beyond(wg)) return;
    if (MODE == WAFER_GS_NORM2 || a.dotwith) {   // (uniform: a kernel argument)
        const double s = wafer_block_sum<4>(acc, red, tid);
        if (tid == 0) partials[wg.p0 + blockIdx.x] = s;
    }
}

// wafer_k_reduce for every active member at once: block `slot` sums the partials of member act[slot] in wafer_k_reduce's order
// into scal[member * scal_stride + out_slot] -- the member's own partials, at its own offset.  ROWWALK: the n2_nb of the row-walk
// norm2 (float storage) at n2_off; else the gs_nb of wafer_k_batch_gs at gs_off (on doubles the two partitions are one).
template <bool ROWWALK>
__global__ __launch_bounds__(256) void wafer_k_batch_gs_reduce(const double *__restrict__ partials, const int *__restrict__ act,
                                                               const WaferBatchMember *__restrict__ mem, double *__restrict__ scal,
                                                               int scal_stride, int out_slot)
{
    __shared__ double sh[256];
    const int member = act[blockIdx.x];
    const double s = ROWWALK ? wafer_batch_reduce_tree(partials + mem[member].n2_off, mem[member].n2_nb, sh)
                             : wafer_batch_reduce_tree(partials + mem[member].gs_off, mem[member].gs_nb, sh);
    if (threadIdx.x == 0) scal[(size_t)member * scal_stride + out_slot] = s;
}

// wafer_batch_norm2 on float storage: get_norm_squared on the partition of a single context's wafer_norm2 -- wafer_k_row_op<T, double, 0>
// (wafer_elementwise.hip.h) on the row walk over the whole slab (local planes [G, G + nzl)), four waves per workgroup, 16 bytes per
// lane, the walk dealt over the member's own n2_nb = wafer_rownorm2_blocks workgroups, each lane adding the squares of its cells in
// the same order, the same wafer_block_sum, one partial per workgroup at partials[n2_off + workgroup] (one shape: n2_off ==
// member * n2_nb); wafer_k_batch_gs_reduce<true> then sums them in wafer_k_reduce's order.  So the double is the one wafer_norm2
// returns for a context of that dtype.  The partition follows the shape, the element size and the device's CU count: nothing of
// the batch (B, index, active set).  Grid (the largest n2_nb among the launched members, members), block 256.
static inline int wafer_rownorm2_blocks(const WaferGeom &g, int esz, int num_cus)   // launch_row_op's grid (wafer_engine_schedules.hip)
{
    const long long segs = (long long)g.nzl * g.ny * ((g.nx + 1024 / esz - 1) / (1024 / esz));
    const long long nb = (long long)num_cus * 8 < (segs + 3) / 4 ? (long long)num_cus * 8 : (segs + 3) / 4;
    return (int)(nb > 1 ? nb : 1);
}

template <typename T, typename GS = WaferGeom>
__global__ __launch_bounds__(256) void wafer_k_batch_rownorm2(GS gs, const WaferBatchMember *__restrict__ mem,
                                                              const int *__restrict__ act, double *__restrict__ partials)
{
    using VT = typename WaferRowVec<T>::type;
    constexpr int VEC = WaferRowVec<T>::N;
    __shared__ double red[4];
    const int member = act[blockIdx.y];
    const WaferBatchMember &m = mem[member];
    const WaferGeom &g = wafer_batch_geom(gs, m.shape);
    const int nb = m.n2_nb;
    if ((int)blockIdx.x >= nb) return;
    const int lz_lo = g.G, lz_hi = g.G + g.nzl;
    const T *__restrict__ phi = static_cast<const T *>(m.phi[m.cur]);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nsegx = (g.nx + 64 * VEC - 1) / (64 * VEC);
    const int wlim = g.pitch - g.xoff - g.R;
    double acc = 0.0;
    WAFER_ROW_WALK_BEGIN_N(lz_lo, lz_hi, g, nb)
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
    if (threadIdx.x == 0) partials[(size_t)m.n2_off + blockIdx.x] = s;
}

// ---- the one-pass form (wafer_batch_set_gs_variant(b, 1), wnum <= WAFER_MAX_LOW) ---------------------------------------------------
// The single context's wafer_k_gs_apply for every active member: raw sums on the un-normalised phi', the Gram matrix of the
// member's stored states, one apply pass.  Schedule of one step, 4 launches whatever wnum and B:
//   wafer_k_batch_step                      (unchanged)
//   wafer_k_batch_gs_sums<NLOW>             sum phi'^2 and t_j = sum l_j phi', j < NLOW: 1 + NLOW partials per workgroup
//   wafer_k_batch_gs_reduce_sums            grid (active members, 1 + NLOW): scal[member * scal_stride + q], q = 0: norm2, 1 + j: t_j
//   wafer_k_batch_gs_apply<NLOW>            norm = sqrt(scal[0]), s_j = t_j / norm - sum_{i<j} s_i G_ji (every thread, identically),
//                                           x = phi' / norm, x = x - l_j s_j (j = 0 .. NLOW-1, unfused), one store
// Bytes per cell on doubles: 24 (step) + 8 (1 + wnum) (sums) + 8 (2 + wnum) (apply), against 48 + 32 wnum of the chain.
// The partition is the chain's (tiles of 64 x 4 work cells x WAFER_GS_ZC planes, gs_nb workgroups per member), a partial of row
// q lies at partials[gs_off * (1 + WAFER_MAX_LOW) + q * gs_nb + workgroup], and a member's Gram matrix at
// gram[member * WAFER_MAX_LOW^2 + j * WAFER_MAX_LOW + i] (i < j) is summed over the same partition (wafer_k_batch_gram): nothing a
// sum sees depends on B, the member's index or the active set.  No floating-point atomics.
// Float storage: every operand widened, every operation fp64; phi is rounded to float ONCE per step after the step kernel's own
// store -- at the apply kernel's store -- where the chain rounds it 1 + wnum times.  Not the chain's bits on any dtype: the
// overlaps are formed by the recurrence instead of on the projected phi (rel ~1e-16 on the scalars).
struct WaferBatchGsOneArgs {
    int flip;                           // the wavefunction of member m is phi[m.cur ^ flip]
    int scal_stride;                    // doubles per member in scal
    const void *low[WAFER_MAX_LOW];     // store slot j (its allocation, of the storage type)
};

#define WAFER_GS_ONE_ROWS (1 + WAFER_MAX_LOW)                        // partial rows per member of the sums kernel
#define WAFER_GRAM_PAIRS (WAFER_MAX_LOW * (WAFER_MAX_LOW - 1) / 2)   // partial rows per member of the Gram kernel

// Block (64, 4), grid (largest gs_nb, active members).  All loads of a lane before the arithmetic: 4 planes x (1 + NLOW) arrays.
template <int NLOW, typename T, typename GS = WaferGeom>
__global__ __launch_bounds__(256) void wafer_k_batch_gs_sums(GS gs, WaferBatchGsOneArgs a, const WaferBatchMember *__restrict__ mem,
                                                             const int *__restrict__ act, double *__restrict__ partials)
{
    __shared__ double red[4];
    const int member = act[blockIdx.y];
    const WaferBatchMember &m = mem[member];
    const WaferGeom &g = wafer_batch_geom(gs, m.shape);
    WaferGsPart wg;
    wafer_gs_part(g, m, WAFER_GS_ONE_ROWS, wg);
    const T *__restrict__ phi = wafer_gs_phi<T>(m, a.flip);
    const long long moff = wg.moff;
    const int bid = blockIdx.x;
    const int i = (bid % wg.ntx) * WAFER_BATCH_TX + threadIdx.x;
    const int j = ((bid / wg.ntx) % wg.nty) * WAFER_BATCH_TY + threadIdx.y;
    const int z0 = g.G + (bid / (wg.ntx * wg.nty)) * WAFER_GS_ZC;
    const int tid = threadIdx.y * WAFER_BATCH_TX + threadIdx.x;
    double acc[1 + NLOW];
#pragma unroll
    for (int q = 0; q <= NLOW; ++q) acc[q] = 0.0;
    if (i < g.nx && j < g.ny) {
        const long long col = (long long)(j + g.R) * g.pitch + g.xoff + (i + g.R);
        double w[WAFER_GS_ZC], l[NLOW][WAFER_GS_ZC];
#pragma unroll
        for (int k = 0; k < WAFER_GS_ZC; ++k) {
            const bool in = z0 + k < g.G + g.nzl;
            const long long p = col + (long long)(z0 + k) * g.plane;
            w[k] = in ? (double)phi[p] : 0.0;
#pragma unroll
            for (int s = 0; s < NLOW; ++s) l[s][k] = in ? (double)__builtin_nontemporal_load(static_cast<const T *>(a.low[s]) + moff + p) : 0.0;
        }
#pragma unroll
        for (int k = 0; k < WAFER_GS_ZC; ++k) {
            if (!(z0 + k < g.G + g.nzl)) continue;
            acc[0] += w[k] * w[k];                                  // grid.rs:454-457, as wafer_k_batch_gs<NORM2>
#pragma unroll
            for (int s = 0; s < NLOW; ++s) acc[1 + s] += l[s][k] * w[k];   // grid.rs:482-487 on the un-normalised phi'
        }
    }
    if (wafer_gs_beyond(wg)) return;
#pragma unroll
    for (int q = 0; q <= NLOW; ++q) {
        const double s = wafer_block_sum<4>(acc[q], red, tid);
        if (tid == 0) partials[wg.p0 + (size_t)q * wg.nb + blockIdx.x] = s;
    }
}

// Block (64, 4), grid (largest gs_nb, active members).  NORMALISE = false (wafer_batch_orthogonalise): no division, norm = 1.
template <int NLOW, typename T, bool NORMALISE, typename GS = WaferGeom>
__global__ __launch_bounds__(256) void wafer_k_batch_gs_apply(GS gs, WaferBatchGsOneArgs a, const WaferBatchMember *__restrict__ mem,
                                                              const int *__restrict__ act, const double *__restrict__ scal,
                                                              const double *__restrict__ gram)
{
    const int member = act[blockIdx.y];
    const WaferBatchMember &m = mem[member];
    const WaferGeom &g = wafer_batch_geom(gs, m.shape);
    WaferGsPart wg;
    wafer_gs_part(g, m, 0, wg);   // (no sum, no barrier: a workgroup beyond the member's partition falls through the `in` predicates)
    T *__restrict__ phi = wafer_gs_phi<T>(m, a.flip);
    const long long moff = wg.moff;
    const double *__restrict__ sc = scal + (size_t)member * a.scal_stride;
    const double *__restrict__ gm = gram + (size_t)member * (WAFER_MAX_LOW * WAFER_MAX_LOW);
    const double norm = NORMALISE ? sqrt(sc[0]) : 1.0;
    double sj[NLOW];
#pragma unroll
    for (int jj = 0; jj < NLOW; ++jj) {   // the recurrence of wafer_k_gs_apply
        double s = NORMALISE ? sc[1 + jj] / norm : sc[1 + jj];
#pragma unroll
        for (int ii = 0; ii < jj; ++ii) s -= sj[ii] * gm[jj * WAFER_MAX_LOW + ii];
        sj[jj] = s;
    }
    const int bid = blockIdx.x;
    const int i = (bid % wg.ntx) * WAFER_BATCH_TX + threadIdx.x;
    const int j = ((bid / wg.ntx) % wg.nty) * WAFER_BATCH_TY + threadIdx.y;
    const int z0 = g.G + (bid / (wg.ntx * wg.nty)) * WAFER_GS_ZC;
    if (i >= g.nx || j >= g.ny) return;
    const long long col = (long long)(j + g.R) * g.pitch + g.xoff + (i + g.R);
    double w[WAFER_GS_ZC], l[NLOW][WAFER_GS_ZC];
#pragma unroll
    for (int k = 0; k < WAFER_GS_ZC; ++k) {
        const bool in = z0 + k < g.G + g.nzl;
        const long long p = col + (long long)(z0 + k) * g.plane;
        w[k] = in ? (double)phi[p] : 0.0;
#pragma unroll
        for (int s = 0; s < NLOW; ++s) l[s][k] = in ? (double)__builtin_nontemporal_load(static_cast<const T *>(a.low[s]) + moff + p) : 0.0;
    }
#pragma unroll
    for (int k = 0; k < WAFER_GS_ZC; ++k) {
        if (!(z0 + k < g.G + g.nzl)) continue;
        double x = w[k];
        if (NORMALISE) x = wafer_div_invariant<double>(x, norm);   // grid.rs:467
#pragma unroll
        for (int s = 0; s < NLOW; ++s) x = x - l[s][k] * sj[s];    // grid.rs:488-490
        phi[col + (long long)(z0 + k) * g.plane] = (T)x;
    }
}

// G_ji = sum l_j l_i, i < j < cnt[blockIdx.y] <= NL, of the members in list: every stored state read once, all pairs formed.
// Partial row q = j (j - 1) / 2 + i at partials[gs_off * WAFER_GRAM_PAIRS + q * gs_nb + workgroup]; rows with j >= the member's
// count come out zero.  Block (64, 4), grid (largest gs_nb, listed members).
template <int NL, typename T, typename GS = WaferGeom>
__global__ __launch_bounds__(256) void wafer_k_batch_gram(GS gs, WaferBatchGsOneArgs a, const WaferBatchMember *__restrict__ mem,
                                                          const int *__restrict__ list, const int *__restrict__ cnt,
                                                          double *__restrict__ partials)
{
    __shared__ double red[4];
    constexpr int NP = NL * (NL - 1) / 2;
    const int member = list[blockIdx.y], count = cnt[blockIdx.y];
    const WaferBatchMember &m = mem[member];
    const WaferGeom &g = wafer_batch_geom(gs, m.shape);
    WaferGsPart wg;
    wafer_gs_part(g, m, WAFER_GRAM_PAIRS, wg);
    const long long moff = wg.moff;
    const int bid = blockIdx.x;
    const int i = (bid % wg.ntx) * WAFER_BATCH_TX + threadIdx.x;
    const int j = ((bid / wg.ntx) % wg.nty) * WAFER_BATCH_TY + threadIdx.y;
    const int z0 = g.G + (bid / (wg.ntx * wg.nty)) * WAFER_GS_ZC;
    const int tid = threadIdx.y * WAFER_BATCH_TX + threadIdx.x;
    double acc[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) acc[q] = 0.0;
    if (i < g.nx && j < g.ny) {
        const long long col = (long long)(j + g.R) * g.pitch + g.xoff + (i + g.R);
        double l[NL][WAFER_GS_ZC];
#pragma unroll
        for (int k = 0; k < WAFER_GS_ZC; ++k) {
            const bool in = z0 + k < g.G + g.nzl;
            const long long p = col + (long long)(z0 + k) * g.plane;
#pragma unroll
            for (int s = 0; s < NL; ++s) l[s][k] = (in && s < count) ? (double)__builtin_nontemporal_load(static_cast<const T *>(a.low[s]) + moff + p) : 0.0;
        }
#pragma unroll
        for (int k = 0; k < WAFER_GS_ZC; ++k)
#pragma unroll
            for (int jj = 1; jj < NL; ++jj)
#pragma unroll
                for (int ii = 0; ii < jj; ++ii) acc[jj * (jj - 1) / 2 + ii] += l[jj][k] * l[ii][k];
    }
    if (wafer_gs_beyond(wg)) return;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const double s = wafer_block_sum<4>(acc[q], red, tid);
        if (tid == 0) partials[wg.p0 + (size_t)q * wg.nb + blockIdx.x] = s;
    }
}

// wafer_k_reduce for every listed member and partial row at once: block (slot, q) sums the gs_nb partials of row q of member
// act[slot], its rows from gs_off * rows on, in wafer_k_reduce's order.  GRAM = false: `rows` = WAFER_GS_ONE_ROWS, into
// out[member * out_stride + q] (the scalars); GRAM = true: `rows` = WAFER_GRAM_PAIRS, row q = j (j - 1) / 2 + i into
// out[member * out_stride + j * WAFER_MAX_LOW + i].
template <bool GRAM>
__global__ __launch_bounds__(256) void wafer_k_batch_gs_reduce_sums(const double *__restrict__ partials, const int *__restrict__ act,
                                                                    int rows, double *__restrict__ out, int out_stride,
                                                                    const WaferBatchMember *__restrict__ mem)
{
    __shared__ double sh[256];
    const int member = act[blockIdx.x], q = blockIdx.y;
    const int n = mem[member].gs_nb;
    const double *p = partials + (size_t)mem[member].gs_off * rows + (size_t)q * n;
    double s = 0.0;
    for (int r = threadIdx.x; r < n; r += 256) s += p[r];
    sh[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    int slot = q;
    if (GRAM) {
        static_assert(WAFER_MAX_LOW == 4, "the row -> (j, i) mapping below lists the six pairs of four states");
        const int jj = q < 1 ? 1 : (q < 3 ? 2 : 3);
        slot = jj * WAFER_MAX_LOW + (q - jj * (jj - 1) / 2);
    }
    out[(size_t)member * out_stride + slot] = sh[0];
}

// entry points (wafer_tu_gs_batch.inc), each once per geometry source GS like WAFER_BATCH_ENTRIES (wafer_tu_gs_batch.hip: WaferGeom,
// wafer_tu_gs_batch_mixed.hip: WaferBatchGeomTable).  f32: float storage.  max_nb: the largest gs_nb among the launched members,
// the grid's extent.
// gs: one elementwise launch of `mode` over the active members and, where it sums (NORM2, or dotwith given), the reduce into
// scal[member * scal_stride + out_slot].
// gs_onepass: sums, reduce and apply (normalise: evolve; else orthogonalise) over the members in act.  1 <= nlow <= WAFER_MAX_LOW;
// partials holds WAFER_GS_ONE_ROWS * gs_nb doubles per member of the batch, gram WAFER_MAX_LOW^2.
// gram: the Gram matrices of the nlist members in list (cnt: states of each, 2 <= cnt <= nl <= WAFER_MAX_LOW) into gram; partials
// holds WAFER_GRAM_PAIRS * gs_nb doubles per member of the batch.
#define WAFER_BATCH_GS_ENTRIES(GS)                                                                                                                   \
    hipError_t wafer_entry_batch_gs(bool f32, int mode, const GS &gs, const WaferBatchGsArgs &a, const WaferBatchMember *mem, const int *act,        \
                                    int nact, int max_nb, double *scal, int out_slot, double *partials, hipStream_t s);                              \
    hipError_t wafer_entry_batch_gs_onepass(bool f32, int nlow, bool normalise, const GS &gs, const WaferBatchGsOneArgs &a,                         \
                                            const WaferBatchMember *mem, const int *act, int nact, int max_nb, double *scal, const double *gram,    \
                                            double *partials, hipStream_t s);                                                                        \
    hipError_t wafer_entry_batch_gram(bool f32, int nl, const GS &gs, const WaferBatchGsOneArgs &a, const WaferBatchMember *mem, const int *list,   \
                                      const int *cnt, int nlist, int max_nb, double *gram, double *partials, hipStream_t s);
WAFER_BATCH_GS_ENTRIES(WaferGeom)
WAFER_BATCH_GS_ENTRIES(WaferBatchGeomTable)
#undef WAFER_BATCH_GS_ENTRIES
