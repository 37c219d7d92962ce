// Batched ensembles (wafer_batch_*, include/wafer_hip.h): B independent ground-state problems of one shape on one device,
// advanced by one launch per step over a workgroup table of (member, tile, z-chunk) entries built from the ACTIVE members only.
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
#pragma once
#include <hip/hip_runtime.h>
#include "wafer_geom.h"
#include "wafer_stencil.hip.h"
#include "wafer_stencil_fused2.hip.h"

// one member of a batch, as the kernels read it (device table, one entry per member)
struct WaferBatchMember {
    void *phi[2];            // logical pointers (plane 0, row 0) of the member's ping-pong buffers
    const void *v;           // V
    const void *potsub;      // pot_sub array (potsub_kind == WAFER_POTSUB_ARRAY)
    double dt;
    double den, zh, zl;      // the member's division plan (WaferDivPlan of c dn^2 m)
    double potsub_scalar;
    int short_forms;         // v_in_range && the plan is checked (WaferStepArgs::v_in_range of a single context)
    int potsub_kind;
    int cur;                 // which phi buffer holds the wavefunction
    int pad;
};

// one workgroup of a batched step: tile (x0, y0) of 64 x 4 work cells, local planes [z0, z1) of member `member`
struct WaferBatchBlock {
    int member, x0, y0, z0, z1, pad;
};

#define WAFER_BATCH_TX 64
#define WAFER_BATCH_TY 4

// One time step of every member in the table.  Block (64, 4): one work cell per lane, marching its z-chunk with a register
// queue of 2R+1 planes along z; x and y neighbours come from global memory (the rows of the tile and its halo are L1 / L2
// hits).  flip: the step's parity within the call (the source buffer of a member is phi[cur ^ flip]).
template <int R>
__global__ __launch_bounds__(256) void wafer_k_batch_step(WaferGeom g, const WaferBatchMember *__restrict__ mem,
                                                          const WaferBatchBlock *__restrict__ blocks, int flip)
{
    const WaferBatchBlock bk = blocks[blockIdx.x];
    const WaferBatchMember &m = mem[bk.member];
    const int sel = (m.cur ^ flip) & 1;
    const double *__restrict__ phi = static_cast<const double *>(m.phi[sel]);
    double *__restrict__ out = static_cast<double *>(m.phi[sel ^ 1]);
    const double *__restrict__ pv = static_cast<const double *>(m.v);
    const int i = bk.x0 + threadIdx.x;
    const int j = bk.y0 + threadIdx.y;
    if (i >= g.nx || j >= g.ny) return;
    const bool sf = m.short_forms != 0;   // (a scalar load: the branches it selects are scalar too)
    const WaferDen<double> den{m.den, m.zh, m.zl, sf};
    const double dt = m.dt;
    const long long col = (long long)(j + R) * g.pitch + g.xoff + (i + R);
    const double *p = phi + col;
    double zq[2 * R + 1];
#pragma unroll
    for (int q = 1; q <= 2 * R; ++q) zq[q] = p[(long long)(bk.z0 + q - 1 - R) * g.plane];
    for (int z = bk.z0; z < bk.z1; ++z) {
#pragma unroll
        for (int q = 0; q < 2 * R; ++q) zq[q] = zq[q + 1];
        const long long o = (long long)z * g.plane;
        zq[2 * R] = p[o + (long long)R * g.plane];
        double xs[2 * R + 1], ys[2 * R + 1];
#pragma unroll
        for (int d = -R; d <= R; ++d) {
            xs[d + R] = (d == 0) ? zq[R] : p[o + d];
            ys[d + R] = (d == 0) ? zq[R] : p[o + (long long)d * g.pitch];
        }
        const double w = zq[R];
        const double S = wafer_stencil_sum<double, R>(xs, ys, zq, w);
        out[col + o] = wafer_update_v<double>(w, pv[col + o], dt, S, den, sf);
    }
}

// compute_observables (grid.rs:303-445) for the members act[blockIdx.y], on the partition of the single context's observables
// launch (wafer_launch_observables_lds: NW waves x RY = 2 rows x VEC = 2 cells per lane, tiles of 128 x 2 NW, z-chunks of
// `zchunk` planes, gridDim.x workgroups per member, swizzled as wafer_k_step_lds swizzles them).  partials[(member * 4 + q) *
// gridDim.x + workgroup]: the four sums energy, norm2, pot_sub, r2.
template <int R, int NW>
__global__ __launch_bounds__(NW * 64) void wafer_k_batch_observables(WaferGeom g, const WaferBatchMember *__restrict__ mem,
                                                                     const int *__restrict__ act, int ntx, int nty, int zchunk,
                                                                     int swz, double *__restrict__ partials)
{
    constexpr int VEC = 2, RY = 2, TX = 64 * VEC, TY = NW * RY;
    __shared__ double red[NW];
    const int member = act[blockIdx.y];
    const WaferBatchMember &m = mem[member];
    int bid = blockIdx.x;
    if (swz) {
        const int n = gridDim.x, q = n >> 3, r = n & 7, k = bid & 7;
        bid = k * q + min(k, r) + (bid >> 3);
    }
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
    const double *__restrict__ phi = static_cast<const double *>(m.phi[m.cur]);
    const double *__restrict__ pv = static_cast<const double *>(m.v);
    const double *__restrict__ ps = static_cast<const double *>(m.potsub);
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
                    const double w = phi[c];
#pragma unroll
                    for (int d = -R; d <= R; ++d) {
                        xs[d + R] = d == 0 ? w : phi[c + d];
                        ys[d + R] = d == 0 ? w : phi[c + (long long)d * g.pitch];
                        zz[d + R] = d == 0 ? w : phi[c + (long long)d * g.plane];
                    }
                    const double S = wafer_stencil_sum<double, R>(xs, ys, zz, w);
                    const double vv = pv[c];
                    ob_e += vv * w * w - wafer_div_invariant<double>(w * S, den); // grid.rs:325-332
                    ob_n += w * w;                                                // grid.rs:407
                    if (pk == 2) ob_v += w * w * ps[c];                          // grid.rs:410-418
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
        if (tid == 0) partials[((size_t)member * 4 + q) * gridDim.x + blockIdx.x] = s;
    }
}

// wafer_k_reduce for every active member at once: block (q, slot) sums the n partials of quantity q of member act[slot] in
// wafer_k_reduce's order into out[member * 4 + q].
static __global__ __launch_bounds__(256) void wafer_k_batch_reduce(const double *__restrict__ partials, const int *__restrict__ act,
                                                                   long long n, double *__restrict__ out)
{
    __shared__ double sh[256];
    const int member = act[blockIdx.y];
    const double *p = partials + ((size_t)member * 4 + blockIdx.x) * n;
    double s = 0.0;
    for (long long q = threadIdx.x; q < n; q += 256) s += p[q];
    sh[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[(size_t)member * 4 + blockIdx.x] = sh[0];
}

// normalise_wavefunction (grid.rs:465-468) of the members act[blockIdx.z]: phi /= sqrt(norm2[member * n2_stride]), the
// expression of wafer_k_row_op<2>.  Block (64, 4) over a 64 x 4 tile of one work plane (blockIdx.y).
static __global__ __launch_bounds__(256) void wafer_k_batch_normalise(WaferGeom g, const WaferBatchMember *__restrict__ mem,
                                                                      const int *__restrict__ act, int ntx,
                                                                      const double *__restrict__ norm2, int n2_stride)
{
    const int member = act[blockIdx.z];
    const WaferBatchMember &m = mem[member];
    const int i = (blockIdx.x % ntx) * WAFER_BATCH_TX + threadIdx.x;
    const int j = (blockIdx.x / ntx) * WAFER_BATCH_TY + threadIdx.y;
    if (i >= g.nx || j >= g.ny) return;
    const double coef = sqrt(norm2[(size_t)member * n2_stride]);
    double *p = static_cast<double *>(m.phi[m.cur]) + g.at(g.G + (int)blockIdx.y, j + g.R, i + g.R);
    *p = wafer_div_invariant<double>(*p, coef);
}

// entry points (wafer_tu_batch.hip)
hipError_t wafer_entry_batch_step(int R, const WaferGeom &g, const WaferBatchMember *mem, const WaferBatchBlock *blocks, int nblocks,
                                  int flip, hipStream_t s);
hipError_t wafer_entry_batch_observables(int R, const WaferGeom &g, const WaferBatchMember *mem, const int *act, int nact, int ntx,
                                         int nty, int nblocks, int zchunk, int swz, double *partials, double *out, hipStream_t s);
hipError_t wafer_entry_batch_normalise(const WaferGeom &g, const WaferBatchMember *mem, const int *act, int nact, const double *norm2,
                                       int n2_stride, hipStream_t s);
