// Set-up in a batch (wafer_batch_set_potentials_builtin, wafer_batch_set_initial_conditions and the range check behind every batched
// writer of V; include/wafer_hip.h): the built-in potential, its pot_sub array, the start and the check of V of every LISTED member in
// one launch each, whatever the members' shapes.
//
// Parity: the per-cell arithmetic IS the context kernels' -- wafer_k_batch_potential calls wafer_potential_cell, the pot_sub kernel
// wafer_potsub_fullcornell_at, the start wafer_initial_condition_at (wafer_setup.hip.h), as wafer_k_potential,
// wafer_k_potsub_fullcornell and wafer_k_initial_condition do.  What differs is where the geometry and the scalars come from: the
// geometry through GS (wafer_batch_geom), the scalars from one WaferBatchSetupRec per listed member, uploaded with the call.
//
// Grid of every kernel here: (tiles, planes, listed members) as large as the largest listed member needs -- 64 x 4 tiles of its padded
// box (the check: its own wider tiles, below), its lz planes -- and a workgroup beyond its member's own extent leaves as a whole
// before any load.  The record, and with it the potential type or the start, is workgroup-uniform: its switch is a scalar branch.
#pragma once
#include <hip/hip_runtime.h>
#include "wafer_setup.hip.h"
#include "wafer_stencil_batch.hip.h"

// what a set-up call says about one listed member (device table, entry blockIdx.z)
struct WaferBatchSetupRec {
    int member;
    int kind;                  // wafer_potential, or wafer_initial_condition
    unsigned long long seed;   // initial conditions (the Gaussian's counter RNG)
    double dn, dt, mass, sig;  // the member's wafer_params
    double mu_t, alphas_2pit, xi_coef, xi_fac;   // the FullCornell host constants of a context's WaferPotArgs
    void *pa, *pb;             // the member's a, b arrays where they exist (logical pointers), else null
};

__device__ __forceinline__ WaferPotArgs wafer_batch_pot_args(const WaferGeom &g, const WaferBatchSetupRec &r)
{
    WaferPotArgs a;
    a.g = g;
    a.type = __builtin_amdgcn_readfirstlane(r.kind);
    a.dn = r.dn; a.dt = r.dt; a.mass = r.mass; a.sig = r.sig;
    a.mu_t = r.mu_t; a.alphas_2pit = r.alphas_2pit; a.xi_coef = r.xi_coef; a.xi_fac = r.xi_fac;
    return a;
}

// V (and a, b where the member has them) of every listed member over every padded cell: wafer_k_potential per member.
// Block (64, 4) over a 64 x 4 tile (blockIdx.x) of plane blockIdx.y of the padded box of member rec[blockIdx.z].member.
template <typename T = double, typename GS = WaferGeom>
static __global__ __launch_bounds__(256) void wafer_k_batch_potential(GS gs, const WaferBatchMember *__restrict__ mem,
                                                                      const WaferBatchSetupRec *__restrict__ rec)
{
    const WaferBatchSetupRec &r = rec[blockIdx.z];
    const WaferBatchMember &m = mem[__builtin_amdgcn_readfirstlane(r.member)];
    const WaferGeom &g = wafer_batch_geom(gs, m.shape);
    const int ntx = (g.px + WAFER_BATCH_TX - 1) / WAFER_BATCH_TX;
    if ((int)blockIdx.y >= g.lz || (int)blockIdx.x >= ntx * ((g.py + WAFER_BATCH_TY - 1) / WAFER_BATCH_TY)) return;
    const int xp = (blockIdx.x % ntx) * WAFER_BATCH_TX + threadIdx.x;
    const int yp = (blockIdx.x / ntx) * WAFER_BATCH_TY + threadIdx.y;
    const WaferPotArgs a = wafer_batch_pot_args(g, r);
    wafer_potential_cell<T>(a, (int)blockIdx.y, yp, xp, static_cast<T *>(const_cast<void *>(m.v)), static_cast<T *>(r.pa), static_cast<T *>(r.pb));
}

// pot_sub of the listed FullCornell members (the others' workgroups leave at once): wafer_k_potsub_fullcornell per member, on the
// work cells of the owned planes.  The same grid as the potential's (the padded box covers the work box).
template <typename T = double, typename GS = WaferGeom>
static __global__ __launch_bounds__(256) void wafer_k_batch_potsub_fullcornell(GS gs, const WaferBatchMember *__restrict__ mem,
                                                                               const WaferBatchSetupRec *__restrict__ rec)
{
    const WaferBatchSetupRec &r = rec[blockIdx.z];
    if (__builtin_amdgcn_readfirstlane(r.kind) != 8) return;   // WAFER_POT_FULLCORNELL
    const WaferBatchMember &m = mem[__builtin_amdgcn_readfirstlane(r.member)];
    const WaferGeom &g = wafer_batch_geom(gs, m.shape);
    const int ntx = (g.nx + WAFER_BATCH_TX - 1) / WAFER_BATCH_TX;
    if ((int)blockIdx.y >= g.nzl || (int)blockIdx.x >= ntx * ((g.ny + WAFER_BATCH_TY - 1) / WAFER_BATCH_TY)) return;
    const int i = (blockIdx.x % ntx) * WAFER_BATCH_TX + threadIdx.x;
    const int j = (blockIdx.x / ntx) * WAFER_BATCH_TY + threadIdx.y;
    const int kl = blockIdx.y;
    if (i >= g.nx || j >= g.ny) return;
    const WaferPotArgs a = wafer_batch_pot_args(g, r);
    T *ps = static_cast<T *>(const_cast<void *>(m.potsub));
    ps[g.at(g.lzp_of_work(kl), j + g.R, i + g.R)] = (T)wafer_potsub_fullcornell_at(a, i, j, g.z_begin + kl);
}

// phi[cur] of every listed member over every padded cell: wafer_k_initial_condition per member.
template <typename T = double, typename GS = WaferGeom>
static __global__ __launch_bounds__(256) void wafer_k_batch_initial_condition(GS gs, const WaferBatchMember *__restrict__ mem,
                                                                              const WaferBatchSetupRec *__restrict__ rec)
{
    const WaferBatchSetupRec &r = rec[blockIdx.z];
    const WaferBatchMember &m = mem[__builtin_amdgcn_readfirstlane(r.member)];
    const WaferGeom &g = wafer_batch_geom(gs, m.shape);
    const int ntx = (g.px + WAFER_BATCH_TX - 1) / WAFER_BATCH_TX;
    if ((int)blockIdx.y >= g.lz || (int)blockIdx.x >= ntx * ((g.py + WAFER_BATCH_TY - 1) / WAFER_BATCH_TY)) return;
    const int xp = (blockIdx.x % ntx) * WAFER_BATCH_TX + threadIdx.x;
    const int yp = (blockIdx.x / ntx) * WAFER_BATCH_TY + threadIdx.y;
    const int lzp = blockIdx.y;
    if (xp >= g.px || yp >= g.py) return;
    WaferIcArgs a;
    a.g = g;
    a.ic = __builtin_amdgcn_readfirstlane(r.kind);
    a.seed = r.seed;
    a.dn = r.dn; a.mass = r.mass; a.sig = r.sig;
    static_cast<T *>(m.phi[m.cur & 1])[g.at(lzp, yp, xp)] = (T)wafer_initial_condition_at(a, lzp, yp, xp);
}

// ---- the check of V -----------------------------------------------------------------------------------------------------------
// check_v_range's two questions (wafer_k_v_range, wafer_k_v_ysym) for every member in act, in ONE launch.  Member act[k] gets three
// 64-bit words at words[3 k], started by the host at (~0, 0, 0):
//   [0] the minimum and [1] the maximum of the bit patterns of fabs(1. + dt * (double)v / 2.) over the member's whole allocation
//       (non-negative doubles: their unsigned order is their numeric order, a NaN sorts above +inf);
//   [2] 1 if V[x, y, z] and V[x, ny-1-y, z] differ in any BIT on a work cell of any plane the member holds, else 0.
// What is read.  Every row of the padded box (py rows of all lz planes) in whole 16-byte vectors: the span of a row from the last
// vector boundary at or before padded x = 0 to the first at or behind padded x = px (rows start on a 128-byte boundary, the pitch
// is whole lines: always aligned, always inside the row).  The cells of that span outside the box are row pads.  They, the guard rows
// and the guard planes -- the rest of the allocation -- hold zeros from creation on and nothing writes them; a
// zero gives fabs(1. + dt * 0. / 2.), which every lane starts from, evaluated as written.  So the two words are those of a walk over
// the whole allocation, for a quarter of the traffic on a 64^3 member.  The mirror: a lane on a work row of the lower half
// (y < ny / 2) loads the same vector of the mirrored row and compares the elements that are work cells.
// Tiles: (64 lanes x one vector) x 4 rows -- 128 doubles or 256 floats wide; max_tiles counts these.  One wave64 shuffle reduction,
// one LDS exchange between the four waves, then at most one integer atomicMin / atomicMax / atomicOr per workgroup -- skipped where
// the word, read first, already says as much (it only ever falls, rises, or goes to 1).  No floating-point atomics.
template <typename T>
struct WaferVec16;
template <>
struct WaferVec16<double> {
    using type = double2;
};
template <>
struct WaferVec16<float> {
    using type = float4;
};

template <typename T>
__device__ __forceinline__ unsigned long long wafer_v_bits(T x)
{
    if constexpr (sizeof(T) == 8) return (unsigned long long)__double_as_longlong((double)x);
    else return (unsigned long long)__float_as_uint((float)x);
}

template <typename T = double, typename GS = WaferGeom>
static __global__ __launch_bounds__(256) void wafer_k_batch_v_check(GS gs, const WaferBatchMember *__restrict__ mem,
                                                                    const int *__restrict__ act, unsigned long long *__restrict__ words)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr int TXV = 64 * VEC;
    using V16 = typename WaferVec16<T>::type;
    const int member = __builtin_amdgcn_readfirstlane(act[blockIdx.z]);
    const WaferBatchMember &m = mem[member];
    const WaferGeom &g = wafer_batch_geom(gs, m.shape);
    const int e_lo = (g.xoff / VEC) * VEC;                          // elements from the row's start
    const int e_hi = ((g.xoff + g.px + VEC - 1) / VEC) * VEC;       // <= pitch: a multiple of a line, which holds whole vectors
    const int ntx = (e_hi - e_lo + TXV - 1) / TXV;
    if ((int)blockIdx.y >= g.lz || (int)blockIdx.x >= ntx * ((g.py + WAFER_BATCH_TY - 1) / WAFER_BATCH_TY)) return;
    const int e = e_lo + (blockIdx.x % ntx) * TXV + threadIdx.x * VEC;
    const int yp = (blockIdx.x / ntx) * WAFER_BATCH_TY + threadIdx.y;
    const int lzp = blockIdx.y;
    const double dt = m.dt;
    const T *__restrict__ v = static_cast<const T *>(m.v);
    const double zero = 0.;
    unsigned long long lo = (unsigned long long)__double_as_longlong(fabs(1. + dt * zero / 2.)), hi = lo, differ = 0;
    if (e < e_hi && yp < g.py) {
        const long long row = (long long)lzp * g.plane + (long long)yp * g.pitch;
        const V16 q = *reinterpret_cast<const V16 *>(v + row + e);
        const T *qe = reinterpret_cast<const T *>(&q);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const double x = fabs(1. + dt * (double)qe[k] / 2.);
            const unsigned long long b = (unsigned long long)__double_as_longlong(x);
            lo = b < lo ? b : lo;
            hi = b > hi ? b : hi;
        }
        const int y = yp - g.R;
        if (y >= 0 && y < g.ny / 2) {
            const long long mrow = (long long)lzp * g.plane + (long long)(g.ny - 1 - y + g.R) * g.pitch;
            const V16 w = *reinterpret_cast<const V16 *>(v + mrow + e);
            const T *we = reinterpret_cast<const T *>(&w);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const int x = e + k - g.xoff - g.R;   // the work index
                if (x >= 0 && x < g.nx && wafer_v_bits<T>(qe[k]) != wafer_v_bits<T>(we[k])) differ = 1;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long l2 = __shfl_down(lo, off, 64), h2 = __shfl_down(hi, off, 64), d2 = __shfl_down(differ, off, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
        differ |= d2;
    }
    __shared__ unsigned long long part[3][WAFER_BATCH_TY];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    if (threadIdx.x == 0) {
        part[0][threadIdx.y] = lo;
        part[1][threadIdx.y] = hi;
        part[2][threadIdx.y] = differ;
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 1; w < WAFER_BATCH_TY; ++w) {
        lo = part[0][w] < lo ? part[0][w] : lo;
        hi = part[1][w] > hi ? part[1][w] : hi;
        differ |= part[2][w];
    }
    unsigned long long *out = words + 3 * (size_t)blockIdx.z;
    if (lo < __hip_atomic_load(&out[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&out[0], lo);
    if (hi > __hip_atomic_load(&out[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&out[1], hi);
    if (differ && !__hip_atomic_load(&out[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&out[2], 1ull);
}

// the x extent of the check's grid for one geometry: its tiles of (64 x one 16-byte vector) x 4 rows (host side of the kernel's ntx)
static inline int wafer_v_check_tiles(const WaferGeom &g, int elem_bytes)
{
    const int VEC = 16 / elem_bytes, TXV = 64 * VEC;
    const int e_lo = (g.xoff / VEC) * VEC, e_hi = ((g.xoff + g.px + VEC - 1) / VEC) * VEC;
    return ((e_hi - e_lo + TXV - 1) / TXV) * ((g.py + WAFER_BATCH_TY - 1) / WAFER_BATCH_TY);
}

// entry points (wafer_tu_batch.inc), once per geometry source.  f32: float storage.  nlisted: the records in rec / the members in
// act.  max_tiles, max_planes: the largest counts among the launched members -- 64 x 4 tiles and planes of their padded boxes; for
// the check wafer_v_check_tiles.
#define WAFER_BATCH_SETUP_ENTRIES(GS)                                                                                                               \
    hipError_t wafer_entry_batch_potential(bool f32, const GS &gs, const WaferBatchMember *mem, const WaferBatchSetupRec *rec, int nlisted,         \
                                           int max_tiles, int max_planes, hipStream_t s);                                                           \
    hipError_t wafer_entry_batch_potsub_fullcornell(bool f32, const GS &gs, const WaferBatchMember *mem, const WaferBatchSetupRec *rec,             \
                                                    int nlisted, int max_tiles, int max_planes, hipStream_t s);                                     \
    hipError_t wafer_entry_batch_initial_condition(bool f32, const GS &gs, const WaferBatchMember *mem, const WaferBatchSetupRec *rec,              \
                                                   int nlisted, int max_tiles, int max_planes, hipStream_t s);                                      \
    hipError_t wafer_entry_batch_v_check(bool f32, const GS &gs, const WaferBatchMember *mem, const int *act, int nact, int max_tiles,              \
                                         int max_planes, unsigned long long *words, hipStream_t s);
WAFER_BATCH_SETUP_ENTRIES(WaferGeom)
WAFER_BATCH_SETUP_ENTRIES(WaferBatchGeomTable)
#undef WAFER_BATCH_SETUP_ENTRIES
