// Symmetry constraints (config.rs:691-728), per cell: the one text of wafer_k_symmetrise (wafer_setup.hip.h, a single context) and
// wafer_k_batch_symmetrise (wafer_stencil_batch.hip.h, every constrained member of a batch in one launch).
//
// The reference walks the SevenPoint frame in place and in ascending order, so cells above the
// mirror plane read cells the same pass has already multiplied by `sign`.  Restated per cell from
// the OLD values (out != in, no ordering between threads): along the constrained axis, padded
// coordinate s in [3, 3 + n), h = (3 + n) / 2, t = n + 4 - s,
//   s <= h or t == s : sign * old[s]
//   t >= 3           : sign * (sign * old[t])
//   t <  3           : sign * old[t]            (t is a frame cell: zero)
// The other cells the reference touches (x frame, the frame row / plane at 3 + n) hold zeros and
// are left alone.  axis 0: z (device plane index), 1: y.
#pragma once
#include <hip/hip_runtime.h>
#include "wafer_geom.h"

// (lzp, yp, xp) is outside the Dirichlet frame: a cell the constraint rewrites
__device__ __forceinline__ bool wafer_symmetrise_inside(const WaferGeom &g, int lzp, int yp, int xp)
{
    const int zp = g.zp_of(lzp);
    return !(xp < g.R || xp >= g.px - g.R || yp < g.R || yp >= g.py - g.R || zp < g.R || zp >= g.pzg - g.R);
}

// the new value of the cell (lzp, yp, xp) inside the frame, from the old values `in`
template <typename T>
__device__ __forceinline__ T wafer_symmetrise_cell(const WaferGeom &g, int axis, double sign, const T *__restrict__ in, int lzp, int yp, int xp)
{
    const int n = axis == 0 ? g.nz : g.ny;
    const int s = axis == 0 ? g.zp_of(lzp) : yp;
    const int h = (3 + n) / 2, t = n + 4 - s;
    double v;
    if (s <= h || t == s) {
        v = sign * (double)in[g.at(lzp, yp, xp)];
    } else {
        const double src = axis == 0 ? (double)in[g.at(lzp + (t - s), yp, xp)] : (double)in[g.at(lzp, t, xp)];
        v = t >= 3 ? sign * (sign * src) : sign * src;
    }
    return (T)v;
}
