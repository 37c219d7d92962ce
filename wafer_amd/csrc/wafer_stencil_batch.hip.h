// Batched ensembles (wafer_batch_*, include/wafer_hip.h): B independent ground-state problems of one shape on one device,
// advanced by one launch per step over a workgroup table of (member, tile, z-chunk) entries built from the ACTIVE members only.
// Ground-state steps may instead run as passes of K steps per launch (wafer_k_batch_stepk below; the same bits).
//
// Parity: every member gets exactly what a single wafer_ctx with its wafer_params computes.
//  - step: the arithmetic of wafer_k_step2_fused, per cell -- wafer_stencil_sum, then a and b formed from V in registers and the
//    update (wafer_update_v, wafer_stencil_fused2.hip.h) with the member's planned division (WaferDen) and its short-form flag.
//    Every ground-state kernel of the engine rounds the same way, so the bits are those of any single context.
//  - observables: the single context's partition (wafer_k_step_lds in its observables mode, NLOW = -2): the same 128 x TY
//    tiles, z-chunks and workgroup swizzle, each lane summing the same cells in the same order, the same wafer_block_sum, one
//    partial per workgroup at the same index -- then wafer_k_reduce's tree, per member.  The values are loaded straight from
//    global memory instead of through the LDS tile; the sums see the same operands.
//  - normalise: wafer_k_row_op<2>'s expression, x / sqrt(norm2) by wafer_div_invariant.
//
// Storage and arithmetic types.  T is what the arrays hold, C what the step computes in: <double, double> (dtype f64),
// <float, double> (f32: float arrays, every operand widened, the result of EVERY step rounded to float) and <float, float>
// (f32fast: dt, den, V, a, b and every operation of the step are float; the member's own fp32 division plan).  a and b are formed
// from the stored V in C, as the single context's default kernels form them.  Observables, normalise and the sums compute in
// double on whatever the arrays hold; normalise rounds its quotient to T.
#pragma once
#include <hip/hip_runtime.h>
#include "wafer_geom.h"
#include "wafer_batch_plan.h"
#include "wafer_stencil.hip.h"
#include "wafer_stencil_fused2.hip.h"
#include "wafer_symmetry.hip.h"

// one member of a batch, as the kernels read it (device table, one entry per member)
struct WaferBatchMember {
    void *phi[2];            // logical pointers (plane 0, row 0) of the member's ping-pong buffers
    const void *v;           // V
    const void *potsub;      // pot_sub array (potsub_kind == WAFER_POTSUB_ARRAY)
    double dt;
    double den, zh, zl;      // the member's division plan (WaferDivPlan of c dn^2 m)
    double potsub_scalar;
    float den_f, zh_f, zl_f; // the member's fp32 plan (f32fast: WaferDivPlanF of (float)den; zh_f == 0: none, or not checked)
    int short_forms;         // v_in_range && the plan is checked (WaferStepArgs::v_in_range of a single context)
    int potsub_kind;
    int cur;                 // which phi buffer holds the wavefunction
    // what depends on the member beside its arrays, for every batch, one shape or several: the kernels below take a member's
    // partition, its workgroup count, the place of its partials and its place in a store slot from here and from nowhere else
    int shape;               // the member's entry in the batch's table of distinct geometries (one shape: 0, not read -- wafer_batch_geom)
    int obs_ntx, obs_nty, obs_zchunk, obs_nb;   // its observables partition: a single context's of that shape
    int n2_nb;               // workgroups of its wafer_batch_norm2 (wafer_rownorm2_blocks on float storage, wafer_gs_blocks on doubles)
    long long obs_off;       // where its [4][obs_nb] partials begin in the observables' partials buffer (doubles)
    long long n2_off;        // where its n2_nb partials begin in the norm2 partials buffer
    // the excited-state kernels' partition of its shape (wafer_batch_gs_partition, wafer_batch_plan.h) and its place in a store slot
    int gs_nb;               // its workgroups: wafer_gs_blocks of its shape (float storage: not n2_nb, which is the row walk's there)
    long long gs_off;        // the workgroups of the members before it: its `rows` rows of gs_nb partials begin at gs_off * rows
    long long slot_off;      // its logical origin (plane 0, row 0) in a store slot's allocation, in elements
};

// Where a kernel takes its geometry from (the template parameter GS of the kernels below).  WaferGeom: the batch's one geometry, a
// kernel argument -- a batch of one shape.  WaferBatchGeomTable: the batch's table of distinct geometries in device memory,
// indexed by the workgroup's shape index -- a batch of several shapes.  The index is workgroup-uniform (it comes from the
// workgroup's table entry or its member record), so the copy below is scalar loads into SGPRs, made once before any loop.
// Everything after that copy is one text for both: this function is the ONLY place where the two instantiations of a batched
// kernel differ.  Whatever depends on the member comes from its WaferBatchMember record; gridDim.x is the grid's extent (the
// largest count among the launched members), and a workgroup at or beyond its member's own count leaves as a whole before any
// load or barrier -- which never happens on one shape, where every member's count is the extent.  (The excited-state kernels place
// that exit behind a body whose plane predicate already keeps such a workgroup from touching a cell: wafer_gs_part.)
struct WaferBatchGeomTable {
    const WaferGeom *geoms;
};
__device__ __forceinline__ const WaferGeom &wafer_batch_geom(const WaferGeom &g, int) { return g; }
__device__ __forceinline__ WaferGeom wafer_batch_geom(const WaferBatchGeomTable &t, int shape)
{
    return t.geoms[__builtin_amdgcn_readfirstlane(shape)];
}

// the member's division by c dn^2 m in the arithmetic type C (wafer_den of a single context's WaferStepArgs)
template <typename C>
__device__ __forceinline__ WaferDen<C> wafer_batch_den(const WaferBatchMember &m, bool sf)
{
    if constexpr (std::is_same_v<C, double>) return WaferDen<double>{m.den, m.zh, m.zl, sf};
    else return WaferDen<float>{m.den_f, m.zh_f, m.zl_f, sf && m.zh_f != 0.f};
}

// one workgroup of a batched step: WaferBatchBlock (wafer_batch_plan.h); the one-step kernel's tiles are 64 x 4 work cells

#define WAFER_BATCH_TX 64
#define WAFER_BATCH_TY 4

// One time step of every member in the table.  Block (64, 4): one work cell per lane, marching its z-chunk with a register
// queue of 2R+1 planes along z; x and y neighbours come from global memory (the rows of the tile and its halo are L1 / L2
// hits).  flip: the step's parity within the call (the source buffer of a member is phi[cur ^ flip]).
template <int R, typename T = double, typename C = double, typename GS = WaferGeom>
__global__ __launch_bounds__(256) void wafer_k_batch_step(GS gs, const WaferBatchMember *__restrict__ mem,
                                                          const WaferBatchBlock *__restrict__ blocks, int flip)
{
    const WaferBatchBlock bk = blocks[blockIdx.x];
    const WaferGeom &g = wafer_batch_geom(gs, bk.shape);
    const WaferBatchMember &m = mem[bk.member];
    const int sel = (m.cur ^ flip) & 1;
    const T *__restrict__ phi = static_cast<const T *>(m.phi[sel]);
    T *__restrict__ out = static_cast<T *>(m.phi[sel ^ 1]);
    const T *__restrict__ pv = static_cast<const T *>(m.v);
    const int i = bk.x0 + threadIdx.x;
    const int j = bk.y0 + threadIdx.y;
    if (i >= g.nx || j >= g.ny) return;
    const bool sf = m.short_forms != 0;   // (a scalar load: the branches it selects are scalar too)
    const WaferDen<C> den = wafer_batch_den<C>(m, sf);
    const C dt = (C)m.dt;
    const long long col = (long long)(j + R) * g.pitch + g.xoff + (i + R);
    const T *p = phi + col;
    C zq[2 * R + 1];
#pragma unroll
    for (int q = 1; q <= 2 * R; ++q) zq[q] = (C)p[(long long)(bk.z0 + q - 1 - R) * g.plane];
    for (int z = bk.z0; z < bk.z1; ++z) {
#pragma unroll
        for (int q = 0; q < 2 * R; ++q) zq[q] = zq[q + 1];
        const long long o = (long long)z * g.plane;
        zq[2 * R] = (C)p[o + (long long)R * g.plane];
        C xs[2 * R + 1], ys[2 * R + 1];
#pragma unroll
        for (int d = -R; d <= R; ++d) {
            xs[d + R] = (d == 0) ? zq[R] : (C)p[o + d];
            ys[d + R] = (d == 0) ? zq[R] : (C)p[o + (long long)d * g.pitch];
        }
        const C w = zq[R];
        const C S = wafer_stencil_sum<C, R>(xs, ys, zq, w);
        out[col + o] = (T)wafer_update_v<C>(w, (C)pv[col + o], dt, S, den, sf);
    }
}

// ---- K steps per launch ----------------------------------------------------------------------------------------------------
// wafer_k_batch_stepk<R, K>: phi0 --step--> phi1 ... --step--> phiK for every entry of a table built by wafer_batch_fused_table,
// with phi1 .. phi(K-1) in registers and LDS only (the temporal blocking of wafer_k_step2_fused / wafer_k_step3_fused, in a
// compact form for grids of 50^3 .. 128^3).
//
// Cells, not roles.  Level k (phi k) is needed on the tile grown by (K-k) R cells on every side; these regions are nested, so
// the cells of the phi0 region are put in ONE order in which every region is a prefix: first the tile itself row by row (one
// wave across a 64-cell row), then ring after ring outwards, each ring R cells thick.  Thread t owns the cells t, t + 256,
// t + 512, ... of that order for every level: it carries the z-queues of its cells in registers (2R+1 planes of each of
// phi0 .. phi(K-1), and V), computes level k for its cells below N_k = cells of level k's region, and so needs no halo-row or
// halo-column role: a level's halo is the tail of the same list.  Waves whose cells all lie beyond N_k skip the level.
// x and y neighbours come from LDS: phi0's plane z double-buffered, every intermediate level as a ring of R+1 planes, all in
// the phi0 region's layout (W0 x H0).  One barrier per plane:
//   iteration z:  prefetch phi0 plane z+R+1 and V plane z+1;  stage phi0 plane z+1 into the other buffer;
//                 level 1 plane z, level 2 plane z-R, ..., level K plane z-(K-1)R -> global;  barrier;  rotate the queues.
// The arithmetic per cell is the one-step kernel's, call for call: wafer_stencil_sum then wafer_update_v with the member's
// WaferDen and its short-form flag, so the bits are those of K launches of wafer_k_batch_step.
// Dirichlet frame: a cell of an intermediate level outside the work area (frame, pad, planes outside [G, G + nzl)) is set to 0,
// never computed; the last level writes work cells only.
// z-chunks: level k is computed on planes [z0 - (K-k) R, z1 + (K-k) R); phi0 is loaded from [z0 - K R, z1 + K R).
// Float storage (T = float): global loads and stores are float, the queues and the LDS planes hold the arithmetic type C --
// double for f32 (the arrangement of wafer_f32_wide, wafer_storage.h: nothing inside the CU differs from the fp64 kernel),
// float for f32fast (half the LDS) -- and every level's result is rounded to float AS IT IS PRODUCED, before it enters a queue or
// a ring: the next level reads what a single step would have stored and loaded again, so the bits are those of K single steps.
// QB: bytes of a queue / LDS element (sizeof(C)).
template <int R, int K, int QB = 8>
struct WaferBatchKCfg {
    static constexpr int TX = WAFER_BATCHK_TX, TY = WAFER_BATCHK_TY, NT = 256;
    static constexpr int H = K * R;                              // phi0 halo per side
    static constexpr int W0 = TX + 2 * H, H0 = TY + 2 * H;       // the LDS layout of every level: the phi0 region
    static constexpr int PLANE = W0 * H0;
    static constexpr int NB = R + 1;                             // ring depth of an intermediate level
    static constexpr int ncells(int k) { return (TX + 2 * (K - k) * R) * (TY + 2 * (K - k) * R); }   // level k's region
    static constexpr int cpt(int k) { return (ncells(k) + NT - 1) / NT; }                            // cells per thread
    static constexpr int LDS_BYTES = QB * PLANE * (2 + (K - 1) * NB);
    // Loads carry no bounds predicates; the tile's overhang lies in the allocation's zero guard zone (wafer_geom.h), checked by
    // hand for K R <= 6 (R <= 3, K <= 3 with K R <= gz = 3 R):
    //  rows:    work rows y0 - K R .. y0 + TY - 1 + K R with y0 + TY - 1 <= ny + TY - 2, i.e. padded rows -(K-1) R .. ny + TY - 2
    //           + (K+1) R; the allocation holds padded rows -gy .. ny + 2 R + gy - 1 with gy = 16 + 3 R: needs TY - 2 + (K+1) R
    //           <= 5 R + 15, true for TY <= 16.
    //  columns: (8-byte elements, wafer_make_geom(..., 8)) element xoff + R + x = 16 + x for work x in -K R .. 64 ceil(nx / 64)
    //           + K R - 1: at least 16 - K R >= 10, at most 15 + 64 ceil(nx / 64) + K R <= 21 + 128 ceil(nx / 128) < pitch =
    //           32 + 128 ceil(nx / 128).
    //           (4-byte elements, wafer_make_geom(..., 4): xoff = 32 - R, rows of 256-element tiles, pitch = 64 + 256 ceil(nx /
    //           256)) element 32 + x: at least 32 - K R >= 26, at most 31 + 64 ceil(nx / 64) + K R <= 37 + 256 ceil(nx / 256)
    //           < pitch.
    //  rows and planes count elements, not bytes (gy, gz, G do not depend on the element size): the same for both geometries.
    //  planes:  z0 - K R >= G - K R >= -gz and z1 + K R - 1 <= G + nzl + K R - 1 < lz + gz = nzl + 2 G + 3 R.
    static_assert(TX == 64 && TY <= 16 && K * R <= 6 && K <= 3, "the guard-zone check above (both the 8-byte and the 4-byte geometry)");
    static_assert(QB == 8 || QB == 4, "queues and LDS hold double or float");
    static_assert(LDS_BYTES <= 65536, "static LDS");
};

template <int R, int K, typename T = double, typename C = double, typename GS = WaferGeom>
__global__ __launch_bounds__(256) void wafer_k_batch_stepk(GS gs, const WaferBatchMember *__restrict__ mem,
                                                           const WaferBatchBlock *__restrict__ blocks, int flip)
{
    using Cfg = WaferBatchKCfg<R, K, (int)sizeof(C)>;
    constexpr int NT = Cfg::NT, W0 = Cfg::W0, PLANE = Cfg::PLANE, NB = Cfg::NB, H = Cfg::H;
    constexpr int C0 = Cfg::cpt(0), C1 = Cfg::cpt(1), NQ = 2 * R + 1, NV = (K - 1) * R + 1;
    __shared__ C lds0[2 * PLANE];
    __shared__ C ldsk[(K - 1) * NB * PLANE];

    const WaferBatchBlock bk = blocks[blockIdx.x];
    const WaferGeom &g = wafer_batch_geom(gs, bk.shape);
    const WaferBatchMember &m = mem[bk.member];
    const int sel = (m.cur ^ flip) & 1;
    const T *__restrict__ phi = static_cast<const T *>(m.phi[sel]);
    T *__restrict__ out = static_cast<T *>(m.phi[sel ^ 1]);
    const T *__restrict__ pv = static_cast<const T *>(m.v);
    const bool sf = m.short_forms != 0;   // (workgroup-uniform: a scalar branch)
    const WaferDen<C> den = wafer_batch_den<C>(m, sf);
    const C dt = (C)m.dt;
    const int tid = threadIdx.x;

    // ---- this thread's cells ---------------------------------------------------------------------
    int lpos[C0], goff[C0];
    unsigned work = 0;   // bit q: cell q is a work cell
#pragma unroll
    for (int q = 0; q < C0; ++q) {
        const int c = min(tid + q * NT, Cfg::ncells(0) - 1);   // surplus threads repeat the last cell (same value, same place)
        int lx, ly;
        wafer_batchk_cell(R, K, c, lx, ly);   // (wafer_batch_plan.h)
        const int x = bk.x0 - H + lx, y = bk.y0 - H + ly;
        lpos[q] = ly * W0 + lx;
        goff[q] = (y + R) * g.pitch + g.xoff + R + x;
        if (x >= 0 && x < g.nx && y >= 0 && y < g.ny) work |= 1u << q;
    }

    // ---- prologue: level 1's first plane is zf; the phi0 queue holds planes zf - R .. zf + R ------
    const int zf = bk.z0 - (K - 1) * R, zend = bk.z1 + (K - 1) * R;
    C q0[NQ][C0];
    C qk[K - 1][NQ][C1];   // levels 1 .. K-1, planes p - R .. p + R around the plane p the next level is computed on
    C vq[NV][C1];          // V of planes z - (K-1) R .. z
#pragma unroll
    for (int mq = 0; mq < NQ; ++mq)
#pragma unroll
        for (int q = 0; q < C0; ++q) q0[mq][q] = (C)phi[(long long)(zf - R + mq) * g.plane + goff[q]];
#pragma unroll
    for (int l = 0; l < K - 1; ++l)
#pragma unroll
        for (int mq = 0; mq < NQ; ++mq)
#pragma unroll
            for (int q = 0; q < C1; ++q) qk[l][mq][q] = C(0);   // (zeros that never reach an output: a level starts on its first valid plane)
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int q = 0; q < C1; ++q) vq[j][q] = C(0);
#pragma unroll
    for (int q = 0; q < C1; ++q) vq[NV - 1][q] = (C)pv[(long long)zf * g.plane + goff[q]];
    {
        C *t0 = lds0 + (zf & 1) * PLANE;
#pragma unroll
        for (int q = 0; q < C0; ++q) t0[lpos[q]] = q0[R][q];
    }
    __syncthreads();

    for (int z = zf; z < zend; ++z) {
        const bool more = z + 1 < zend;
        const long long zo = (long long)z * g.plane;
        // ---- 1. prefetch phi0 plane z + R + 1 and V plane z + 1 ------------------------------------
        C pre[C0], pre_v[C1];
#pragma unroll
        for (int q = 0; q < C0; ++q) pre[q] = C(0);
#pragma unroll
        for (int q = 0; q < C1; ++q) pre_v[q] = C(0);
        if (more) {
#pragma unroll
            for (int q = 0; q < C0; ++q) pre[q] = (C)phi[zo + (long long)(R + 1) * g.plane + goff[q]];
#pragma unroll
            for (int q = 0; q < C1; ++q) pre_v[q] = (C)pv[zo + g.plane + goff[q]];
            // ---- 2. stage phi0 plane z + 1 ----------------------------------------------------------
            C *nt = lds0 + ((z + 1) & 1) * PLANE;
#pragma unroll
            for (int q = 0; q < C0; ++q) nt[lpos[q]] = q0[R + 1][q];
        }
        // ---- 3. level k on plane p = z - (k-1) R, k = 1 .. K ------------------------------------------
#pragma unroll
        for (int k = 1; k <= K; ++k) {
            const int p = z - (k - 1) * R;
            const int Ck = Cfg::cpt(k), Nk = Cfg::ncells(k);
            const int kw = g.z_begin + (p - g.G);
            // the plane is one this chunk needs of level k, and (intermediate levels) a work plane
            const bool on = p >= bk.z0 - (K - k) * R && (k == K || (kw >= 0 && kw < g.nz));
            const C *src = k == 1 ? lds0 + (z & 1) * PLANE : ldsk + ((k - 2) * NB + ((p % NB) + NB) % NB) * PLANE;
            C *ring = ldsk + ((k - 1 < K - 1 ? k - 1 : 0) * NB + ((p % NB) + NB) % NB) * PLANE;
            if (k < K) {
#pragma unroll
                for (int mq = 0; mq + 1 < NQ; ++mq)
#pragma unroll
                    for (int q = 0; q < C1; ++q) qk[k - 1 < K - 1 ? k - 1 : 0][mq][q] = qk[k - 1 < K - 1 ? k - 1 : 0][mq + 1][q];
            }
#pragma unroll
            for (int q = 0; q < Ck; ++q) {
                C val = C(0);
                const bool act = on && tid + q * NT < Nk && ((work >> q) & 1u);
                if (act) {
                    C xs[NQ], ys[NQ], zz[NQ];
#pragma unroll
                    for (int d = 0; d < NQ; ++d) zz[d] = k == 1 ? q0[d][q] : qk[k >= 2 ? k - 2 : 0][d][q];
                    const C w = zz[R];
#pragma unroll
                    for (int d = -R; d <= R; ++d) {
                        xs[d + R] = d == 0 ? w : src[lpos[q] + d];
                        ys[d + R] = d == 0 ? w : src[lpos[q] + d * W0];
                    }
                    const C S = wafer_stencil_sum<C, R>(xs, ys, zz, w);
                    const T stored = (T)wafer_update_v<C>(w, vq[(K - k) * R][q], dt, S, den, sf);   // every level rounds to the storage type
                    val = (C)stored;
                    if (k == K) out[(long long)p * g.plane + goff[q]] = stored;
                }
                if (k < K) {
                    qk[k - 1 < K - 1 ? k - 1 : 0][NQ - 1][q] = val;
                    ring[lpos[q]] = val;
                }
            }
        }
        __syncthreads();
        // ---- 4. rotate ----------------------------------------------------------------------------------
#pragma unroll
        for (int mq = 0; mq + 1 < NQ; ++mq)
#pragma unroll
            for (int q = 0; q < C0; ++q) q0[mq][q] = q0[mq + 1][q];
#pragma unroll
        for (int q = 0; q < C0; ++q) q0[NQ - 1][q] = pre[q];
#pragma unroll
        for (int j = 0; j + 1 < NV; ++j)
#pragma unroll
            for (int q = 0; q < C1; ++q) vq[j][q] = vq[j + 1][q];
#pragma unroll
        for (int q = 0; q < C1; ++q) vq[NV - 1][q] = pre_v[q];
    }
}

// compute_observables (grid.rs:303-445) for the members act[blockIdx.y], on the partition of the single context's observables
// launch (wafer_launch_observables_lds: NW waves x RY = 2 rows x VEC cells per lane -- 16 bytes of the storage type T: 2 doubles,
// 4 floats -- so tiles of 64 VEC x 2 NW, i.e. 128 x 2 NW (fp64) or 256 x 2 NW (float storage), z-chunks of obs_zchunk planes,
// swizzled as wafer_k_step_lds swizzles them).  Float values are widened; every product and sum is fp64, as in the context's
// kernel (its C is double for every dtype).
// The partition is the member's own (WaferBatchMember::obs_*: ntx, nty, zchunk and nb workgroups, what a context of ITS shape
// gets), gridDim.x is the largest nb among the launched members, and the four sums energy, norm2, pot_sub, r2 of a workgroup lie
// at partials[obs_off + q * nb + workgroup] (one shape: obs_off == member * 4 * nb).
template <int R, int NW, typename T = double, typename GS = WaferGeom>
__global__ __launch_bounds__(NW * 64) void wafer_k_batch_observables(GS gs, const WaferBatchMember *__restrict__ mem,
                                                                     const int *__restrict__ act, int swz, double *__restrict__ partials)
{
    constexpr int VEC = 16 / (int)sizeof(T), RY = 2, TX = 64 * VEC, TY = NW * RY;
    __shared__ double red[NW];
    const int member = act[blockIdx.y];
    const WaferBatchMember &m = mem[member];
    const WaferGeom &g = wafer_batch_geom(gs, m.shape);
    const int nb = m.obs_nb;   // workgroups of this member
    if ((int)blockIdx.x >= nb) return;
    const int ntx = m.obs_ntx, nty = m.obs_nty, zchunk = m.obs_zchunk;
    int bid = blockIdx.x;
    if (swz) bid = wafer_xcd_tile(bid, nb);
    const int tx_i = bid % ntx;
    const int ty_i = (bid / ntx) % nty;
    const int tz_i = bid / (ntx * nty);
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int x0 = tx_i * TX, y0 = ty_i * TY;
    const int xl = lane * VEC, yl = wave * RY;
    const int xi = x0 + xl;
    const int zs = g.G + tz_i * zchunk;
    const int ze = min(zs + zchunk, g.G + g.nzl);
    const T *__restrict__ phi = static_cast<const T *>(m.phi[m.cur]);
    const T *__restrict__ pv = static_cast<const T *>(m.v);
    const T *__restrict__ ps = static_cast<const T *>(m.potsub);
    const WaferDen<double> den{m.den, m.zh, m.zl, m.short_forms != 0};
    const int pk = m.potsub_kind;
    const double pscal = m.potsub_scalar;
    double ob_e = 0.0, ob_n = 0.0, ob_v = 0.0, ob_r = 0.0;
    for (int z = zs; z < ze; ++z) {
        const long long zo = (long long)z * g.plane;
        const double ob_dz = (double)(g.z_begin + (z - g.G)) - ((double)g.nz + 1.) / 2.;
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const int y = y0 + yl + r;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if (y < g.ny && xi + v < g.nx) {
                    const long long c = zo + (long long)(y + R) * g.pitch + g.xoff + R + xi + v;
                    double xs[2 * R + 1], ys[2 * R + 1], zz[2 * R + 1];
                    const double w = (double)phi[c];
#pragma unroll
                    for (int d = -R; d <= R; ++d) {
                        xs[d + R] = d == 0 ? w : (double)phi[c + d];
                        ys[d + R] = d == 0 ? w : (double)phi[c + (long long)d * g.pitch];
                        zz[d + R] = d == 0 ? w : (double)phi[c + (long long)d * g.plane];
                    }
                    const double S = wafer_stencil_sum<double, R>(xs, ys, zz, w);
                    const double vv = (double)pv[c];
                    ob_e += vv * w * w - wafer_div_invariant<double>(w * S, den); // grid.rs:325-332
                    ob_n += w * w;                                                // grid.rs:407
                    if (pk == 2) ob_v += w * w * (double)ps[c];                          // grid.rs:410-418
                    else if (pk == 1) ob_v += w * w * pscal;                     // grid.rs:419-424
                    const double dx = (double)(xi + v) - ((double)g.nx + 1.) / 2.;
                    const double dy = (double)y - ((double)g.ny + 1.) / 2.;
                    ob_r += w * w * (dx * dx + dy * dy + ob_dz * ob_dz);          // grid.rs:428-437
                }
            }
        }
    }
    const double sums[4] = {ob_e, ob_n, ob_v, ob_r};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double s = wafer_block_sum<NW>(sums[q], red, tid);
        if (tid == 0) partials[(size_t)m.obs_off + (size_t)q * nb + blockIdx.x] = s;
    }
}

// wafer_k_reduce for every active member at once: block (q, slot) sums the obs_nb partials of quantity q of member act[slot],
// from its obs_off on, in wafer_k_reduce's order into out[member * 4 + q].
// wafer_k_reduce's order over the n doubles at p, by one workgroup of 256 threads: the sum, valid in thread 0
template <typename I>
__device__ __forceinline__ double wafer_batch_reduce_tree(const double *__restrict__ p, I n, double *sh)
{
    double s = 0.0;
    for (I q = threadIdx.x; q < n; q += 256) s += p[q];
    sh[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    return sh[0];
}

static __global__ __launch_bounds__(256) void wafer_k_batch_reduce(const double *__restrict__ partials, const int *__restrict__ act,
                                                                   const WaferBatchMember *__restrict__ mem, double *__restrict__ out)
{
    __shared__ double sh[256];
    const int member = act[blockIdx.y];
    const long long n = mem[member].obs_nb;
    const double s = wafer_batch_reduce_tree(partials + mem[member].obs_off + (long long)blockIdx.x * n, n, sh);
    if (threadIdx.x == 0) out[(size_t)member * 4 + blockIdx.x] = s;
}

// normalise_wavefunction (grid.rs:465-468) of the members act[blockIdx.z]: phi /= sqrt(norm2[member * n2_stride]), the
// expression of wafer_k_row_op<2> (the quotient in fp64, rounded to the storage type).  Block (64, 4) over a 64 x 4 tile of one
// work plane (blockIdx.y).  The grid has the largest tile and plane counts among the launched members, and a workgroup beyond its
// member's own leaves as a whole.
template <typename T = double, typename GS = WaferGeom>
static __global__ __launch_bounds__(256) void wafer_k_batch_normalise(GS gs, const WaferBatchMember *__restrict__ mem,
                                                                      const int *__restrict__ act,
                                                                      const double *__restrict__ norm2, int n2_stride)
{
    const int member = act[blockIdx.z];
    const WaferBatchMember &m = mem[member];
    const WaferGeom &g = wafer_batch_geom(gs, m.shape);
    const int ntx = (g.nx + WAFER_BATCH_TX - 1) / WAFER_BATCH_TX;
    if ((int)blockIdx.y >= g.nzl || (int)blockIdx.x >= ntx * ((g.ny + WAFER_BATCH_TY - 1) / WAFER_BATCH_TY)) return;
    const int i = (blockIdx.x % ntx) * WAFER_BATCH_TX + threadIdx.x;
    const int j = (blockIdx.x / ntx) * WAFER_BATCH_TY + threadIdx.y;
    if (i >= g.nx || j >= g.ny) return;
    const double coef = sqrt(norm2[(size_t)member * n2_stride]);
    T *p = static_cast<T *>(m.phi[m.cur]) + g.at(g.G + (int)blockIdx.y, j + g.R, i + g.R);
    *p = (T)wafer_div_invariant<double>((double)*p, coef);
}

// symmetrise_wavefunction (config.rs:691-728) of the members act[blockIdx.z], each with its own constraint sym[member] (WAFER_SYM_*,
// never NotConstrained here: the host launches the constrained members only): wafer_k_symmetrise's arithmetic per cell
// (wafer_symmetrise_cell, wafer_symmetry.hip.h) from the OLD values in phi[cur] into the member's other buffer; the host flips cur.
// Block (64, 4) over a 64 x 4 tile of one plane (blockIdx.y) of the member's PADDED box -- px x py cells, all lz planes: the
// context's grid.  The other buffer is scratch between steps, so the kernel writes the whole box: the new value inside the frame,
// zero on it -- what a context gets from clearing the allocation first (the guard rows and planes and the row pads outside the box
// are zeros from creation on and nothing writes them: DESIGN.md section 5).  The constraint is workgroup-uniform (a scalar load).
// The grid has the largest tile and plane counts among the launched members, and a workgroup beyond its member's own leaves as a
// whole before any load.
template <typename T = double, typename GS = WaferGeom>
static __global__ __launch_bounds__(256) void wafer_k_batch_symmetrise(GS gs, const WaferBatchMember *__restrict__ mem,
                                                                       const int *__restrict__ act, const int *__restrict__ sym)
{
    const int member = __builtin_amdgcn_readfirstlane(act[blockIdx.z]);
    const WaferBatchMember &m = mem[member];
    const WaferGeom &g = wafer_batch_geom(gs, m.shape);
    const int ntx = (g.px + WAFER_BATCH_TX - 1) / WAFER_BATCH_TX;
    if ((int)blockIdx.y >= g.lz || (int)blockIdx.x >= ntx * ((g.py + WAFER_BATCH_TY - 1) / WAFER_BATCH_TY)) return;
    const int cons = __builtin_amdgcn_readfirstlane(sym[member]);
    const int axis = cons <= 2 ? 0 : 1;                     // AboutZ, AntisymAboutZ | AboutY, AntisymAboutY
    const double sign = (cons & 1) ? 1.0 : -1.0;            // the odd constraints are the symmetric ones
    const int xp = (blockIdx.x % ntx) * WAFER_BATCH_TX + threadIdx.x;
    const int yp = (blockIdx.x / ntx) * WAFER_BATCH_TY + threadIdx.y;
    const int lzp = blockIdx.y;
    if (xp >= g.px || yp >= g.py) return;
    const int cur = m.cur & 1;
    const T *__restrict__ in = static_cast<const T *>(m.phi[cur]);
    T *__restrict__ out = static_cast<T *>(m.phi[cur ^ 1]);
    out[g.at(lzp, yp, xp)] = wafer_symmetrise_inside(g, lzp, yp, xp) ? wafer_symmetrise_cell<T>(g, axis, sign, in, lzp, yp, xp) : T(0);
}

// entry points (wafer_tu_batch.inc), each once per geometry source GS: const WaferGeom & (a batch of one shape: wafer_tu_batch.hip)
// and const WaferBatchGeomTable & (several: wafer_tu_batch_mixed.hip).  dtype: the batch's wafer_dtype as an int -- 0 f64, 1 f32
// (float storage, fp64 arithmetic), 2 f32fast (float storage, float arithmetic in the ground-state step).  f32 is true for float
// storage (dtype 1 and 2 alike: observables and normalise compute in fp64).
// stepk: the fused pass of K steps; hipErrorInvalidValue where wafer_batch_stepk_lds_bytes(dtype, R, K) is 0 (no such instantiation).
// observables, normalise: max_*: the largest per-member count among the launched members -- the grid's extent, and for one shape
// every member's count.
// symmetrise: sym[member] is the member's WAFER_SYM_* constraint; max_tiles and max_planes count tiles and planes of the padded
// boxes (px x py, lz).
// norm2 (wafer_batch_norm2; kernels: wafer_gs_batch.hip.h): norm2 of the members in act into scal[member * scal_stride + out_slot], each
// on its own partition of WaferBatchMember::n2_nb workgroups -- float storage: wafer_k_batch_rownorm2 on a single context's wafer_norm2
// partition, the same double; doubles: wafer_k_batch_gs<NORM2>.  partials holds every member's n2_nb doubles, end to end.
#define WAFER_BATCH_ENTRIES(GS)                                                                                                                      \
    hipError_t wafer_entry_batch_step(int dtype, int R, const GS &gs, const WaferBatchMember *mem, const WaferBatchBlock *blocks, int nblocks,      \
                                      int flip, hipStream_t s);                                                                                      \
    hipError_t wafer_entry_batch_stepk(int dtype, int R, int K, const GS &gs, const WaferBatchMember *mem, const WaferBatchBlock *blocks,           \
                                       int nblocks, int flip, hipStream_t s);                                                                        \
    hipError_t wafer_entry_batch_observables(bool f32, int R, const GS &gs, const WaferBatchMember *mem, const int *act, int nact, int max_nb,         \
                                             int swz, double *partials, double *out, hipStream_t s);                                                \
    hipError_t wafer_entry_batch_normalise(bool f32, const GS &gs, const WaferBatchMember *mem, const int *act, int nact, int max_tiles,             \
                                           int max_planes, const double *norm2, int n2_stride, hipStream_t s);                                      \
    hipError_t wafer_entry_batch_symmetrise(bool f32, const GS &gs, const WaferBatchMember *mem, const int *act, int nact, const int *sym,           \
                                            int max_tiles, int max_planes, hipStream_t s);                                                           \
    hipError_t wafer_entry_batch_norm2(bool f32, const GS &gs, const WaferBatchMember *mem, const int *act, int nact, int max_nb, double *scal,     \
                                       int scal_stride, int out_slot, double *partials, hipStream_t s);
WAFER_BATCH_ENTRIES(WaferGeom)
WAFER_BATCH_ENTRIES(WaferBatchGeomTable)
#undef WAFER_BATCH_ENTRIES
int wafer_batch_stepk_lds_bytes(int dtype, int R, int K);
