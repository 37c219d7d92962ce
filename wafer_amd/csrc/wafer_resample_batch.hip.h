// Resampling in a batch (wafer_batch_resample, wafer_batch_resample_member; include/wafer_hip.h): ONE source -- a host array or the
// work cells of a member's phi or stored state -- trilinearly resampled onto an array of every listed member in one launch,
// whatever the members' shapes.  input::trilerp_resize (input.rs:667-716) per member, as wafer_k_trilerp gives a context.
//
// Parity: the per-cell arithmetic IS wafer_k_trilerp's -- both kernels call wafer_trilerp_cell (wafer_setup.hip.h) and differ only
// in the accessor that reads the source.  Double arithmetic, a float source widened exactly, the result rounded to T at the store.
//
// Source layout.  The lanes of a wave run along the target's x, so the source is read x-FASTEST: the 8 loads of a wave each touch
// the span of source x that 64 consecutive target cells sample, about 64 (sx - 1) / (bx - 1) elements -- one or two cache lines
// when upsampling -- instead of 64 lines a plane stride apart, as a z-fastest host array would give (wafer_k_trilerp, which runs
// once per context).  A member's slice is x-fastest already: WaferResampleSource describes its work cells through its WaferGeom.
// A host array is uploaded once per call and transposed once (wafer_k_transpose<double, true> over a dense geometry) into the
// batch's scratch.
#pragma once
#include <hip/hip_runtime.h>
#include "wafer_setup.hip.h"
#include "wafer_stencil_batch.hip.h"

// an x-fastest source: element (x, y, z) of its (sx, sy, sz) points at base[off0 + z * plane + y * pitch + x]
struct WaferResampleSource {
    const void *base;
    long long off0;      // element offset of point (0, 0, 0)
    long long pitch;     // row stride in elements
    long long plane;     // plane stride in elements
    int sx, sy, sz;
};

// Block (64, 4) over a 64 x 4 tile of one plane (blockIdx.y) of the PADDED box of member act[blockIdx.z] -- px x py cells, all lz
// planes, wafer_k_batch_symmetrise's grid -- one cell per lane: a work cell gets its interpolated value, every other cell of the
// box (the Dirichlet frame, ghost planes outside the global grid) zero.  That is what a context has after resample_into's memset
// of the allocation: the cells outside the box -- guard rows, guard planes, the row pads -- hold zeros from creation on and no
// kernel or copy of the engine writes them, so they need none; the box is everything a set-up call may have
// left non-zero (wafer_k_potential and the uploads write it whole).
// The target array: dst0 (an allocation laid out as the batch's arrays are; the member's origin is WaferBatchMember::slot_off),
// or, with by_cur, dst1 for a member whose current phi buffer is 1.  basis: WAFER_BASIS_PADDED (0) the padded size, WAFER_BASIS_WORK
// (1) the work size.  The grid has the largest tile and plane counts among the launched members, and a workgroup beyond its
// member's own leaves as a whole before any load.  No LDS, no scratch.
template <typename T = double, typename S = double, typename GS = WaferGeom>
static __global__ __launch_bounds__(256) void wafer_k_batch_trilerp(GS gs, const WaferBatchMember *__restrict__ mem,
                                                                    const int *__restrict__ act, WaferResampleSource src,
                                                                    void *dst0, void *dst1, int by_cur, int basis)
{
    const int member = __builtin_amdgcn_readfirstlane(act[blockIdx.z]);
    const WaferBatchMember &m = mem[member];
    const WaferGeom &g = wafer_batch_geom(gs, m.shape);
    const int ntx = (g.px + WAFER_BATCH_TX - 1) / WAFER_BATCH_TX;
    if ((int)blockIdx.y >= g.lz || (int)blockIdx.x >= ntx * ((g.py + WAFER_BATCH_TY - 1) / WAFER_BATCH_TY)) return;
    const int xp = (blockIdx.x % ntx) * WAFER_BATCH_TX + threadIdx.x;
    const int yp = (blockIdx.x / ntx) * WAFER_BATCH_TY + threadIdx.y;
    const int lzp = blockIdx.y;
    if (xp >= g.px || yp >= g.py) return;
    T *__restrict__ dst = static_cast<T *>((by_cur && (m.cur & 1)) ? dst1 : dst0) + m.slot_off;
    const int i = xp - g.R, j = yp - g.R, k = g.z_begin + (lzp - g.G);   // the work index, as wafer_k_trilerp forms it
    double val = 0.;
    if (i >= 0 && i < g.nx && j >= 0 && j < g.ny && k >= 0 && k < g.nz) {
        const S *__restrict__ s = static_cast<const S *>(src.base) + src.off0;
        auto at = [&](int x, int y, int z) { return (double)s[(long long)z * src.plane + (long long)y * src.pitch + x]; };
        const bool work = basis != 0;
        val = wafer_trilerp_cell(src.sx, src.sy, src.sz, work ? g.nx : g.px, work ? g.ny : g.py, work ? g.nz : g.pzg, i, j, k, at);
    }
    dst[g.at(lzp, yp, xp)] = (T)val;
}

// entry points (wafer_tu_batch.inc), once per geometry source.  f32: float storage; src_f32: the source holds floats (a member of
// a float batch; a host source is always double).  max_tiles and max_planes count tiles and planes of the padded boxes of the
// launched members.
#define WAFER_BATCH_RESAMPLE_ENTRY(GS)                                                                                                              \
    hipError_t wafer_entry_batch_trilerp(bool f32, bool src_f32, const GS &gs, const WaferBatchMember *mem, const int *act, int nact,               \
                                         int max_tiles, int max_planes, const WaferResampleSource &src, void *dst0, void *dst1, int by_cur,         \
                                         int basis, hipStream_t s);
WAFER_BATCH_RESAMPLE_ENTRY(WaferGeom)
WAFER_BATCH_RESAMPLE_ENTRY(WaferBatchGeomTable)
#undef WAFER_BATCH_RESAMPLE_ENTRY
