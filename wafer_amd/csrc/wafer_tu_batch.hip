// translation unit: the batched ensemble kernels (wafer_stencil_batch.hip.h) for the three dtypes -- 0 f64 <double, double>, 1 f32
// <float, double> (float storage, fp64 arithmetic), 2 f32fast <float, float> (float arithmetic in the ground-state step)
#include "wafer_stencil_batch.hip.h"

template <typename T, typename C>
static hipError_t launch_step(int R, const WaferGeom &g, const WaferBatchMember *mem, const WaferBatchBlock *blocks, int nblocks, int flip,
                              hipStream_t s)
{
    const dim3 grid((unsigned)nblocks), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    switch (R) {
    case 1: hipLaunchKernelGGL((wafer_k_batch_step<1, T, C>), grid, block, 0, s, g, mem, blocks, flip); break;
    case 2: hipLaunchKernelGGL((wafer_k_batch_step<2, T, C>), grid, block, 0, s, g, mem, blocks, flip); break;
    case 3: hipLaunchKernelGGL((wafer_k_batch_step<3, T, C>), grid, block, 0, s, g, mem, blocks, flip); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t wafer_entry_batch_step(int dtype, int R, const WaferGeom &g, const WaferBatchMember *mem, const WaferBatchBlock *blocks,
                                  int nblocks, int flip, hipStream_t s)
{
    if (dtype == 0) return launch_step<double, double>(R, g, mem, blocks, nblocks, flip, s);
    if (dtype == 1) return launch_step<float, double>(R, g, mem, blocks, nblocks, flip, s);
    if (dtype == 2) return launch_step<float, float>(R, g, mem, blocks, nblocks, flip, s);
    return hipErrorInvalidValue;
}

// the instantiations of the fused pass, the same list for every dtype: ThreePoint 3 steps (and 2, for the remainder of a call),
// FivePoint 2 steps.  f64 and f32 keep double queues and LDS, f32fast float ones (half the bytes).
int wafer_batch_stepk_lds_bytes(int dtype, int R, int K)
{
    if (dtype < 0 || dtype > 2) return 0;
    const bool wide = dtype != 2;
    if (R == 1 && K == 3) return wide ? WaferBatchKCfg<1, 3, 8>::LDS_BYTES : WaferBatchKCfg<1, 3, 4>::LDS_BYTES;
    if (R == 1 && K == 2) return wide ? WaferBatchKCfg<1, 2, 8>::LDS_BYTES : WaferBatchKCfg<1, 2, 4>::LDS_BYTES;
    if (R == 2 && K == 2) return wide ? WaferBatchKCfg<2, 2, 8>::LDS_BYTES : WaferBatchKCfg<2, 2, 4>::LDS_BYTES;
    return 0;
}

template <typename T, typename C>
static hipError_t launch_stepk(int R, int K, const WaferGeom &g, const WaferBatchMember *mem, const WaferBatchBlock *blocks, int nblocks,
                               int flip, hipStream_t s)
{
    const dim3 grid((unsigned)nblocks), block(256);
    if (R == 1 && K == 3) hipLaunchKernelGGL((wafer_k_batch_stepk<1, 3, T, C>), grid, block, 0, s, g, mem, blocks, flip);
    else if (R == 1 && K == 2) hipLaunchKernelGGL((wafer_k_batch_stepk<1, 2, T, C>), grid, block, 0, s, g, mem, blocks, flip);
    else if (R == 2 && K == 2) hipLaunchKernelGGL((wafer_k_batch_stepk<2, 2, T, C>), grid, block, 0, s, g, mem, blocks, flip);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t wafer_entry_batch_stepk(int dtype, int R, int K, const WaferGeom &g, const WaferBatchMember *mem, const WaferBatchBlock *blocks,
                                   int nblocks, int flip, hipStream_t s)
{
    if (dtype == 0) return launch_stepk<double, double>(R, K, g, mem, blocks, nblocks, flip, s);
    if (dtype == 1) return launch_stepk<float, double>(R, K, g, mem, blocks, nblocks, flip, s);
    if (dtype == 2) return launch_stepk<float, float>(R, K, g, mem, blocks, nblocks, flip, s);
    return hipErrorInvalidValue;
}

template <typename T>
static hipError_t launch_observables(int R, const WaferGeom &g, const WaferBatchMember *mem, const int *act, dim3 grid, int ntx, int nty,
                                     int zchunk, int swz, double *partials, hipStream_t s)
{
    // the waves per workgroup of wafer_launch_observables_lds: 8 (ThreePoint / FivePoint), 4 (SevenPoint)
    switch (R) {
    case 1: hipLaunchKernelGGL((wafer_k_batch_observables<1, 8, T>), grid, dim3(512), 0, s, g, mem, act, ntx, nty, zchunk, swz, partials); break;
    case 2: hipLaunchKernelGGL((wafer_k_batch_observables<2, 8, T>), grid, dim3(512), 0, s, g, mem, act, ntx, nty, zchunk, swz, partials); break;
    case 3: hipLaunchKernelGGL((wafer_k_batch_observables<3, 4, T>), grid, dim3(256), 0, s, g, mem, act, ntx, nty, zchunk, swz, partials); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t wafer_entry_batch_observables(bool f32, int R, const WaferGeom &g, const WaferBatchMember *mem, const int *act, int nact,
                                         int ntx, int nty, int nblocks, int zchunk, int swz, double *partials, double *out, hipStream_t s)
{
    const dim3 grid((unsigned)nblocks, (unsigned)nact);
    const hipError_t e = f32 ? launch_observables<float>(R, g, mem, act, grid, ntx, nty, zchunk, swz, partials, s)
                             : launch_observables<double>(R, g, mem, act, grid, ntx, nty, zchunk, swz, partials, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wafer_k_batch_reduce, dim3(4, (unsigned)nact), dim3(256), 0, s, partials, act, (long long)nblocks, out);
    return hipGetLastError();
}

hipError_t wafer_entry_batch_normalise(bool f32, const WaferGeom &g, const WaferBatchMember *mem, const int *act, int nact,
                                       const double *norm2, int n2_stride, hipStream_t s)
{
    const int ntx = (g.nx + WAFER_BATCH_TX - 1) / WAFER_BATCH_TX, nty = (g.ny + WAFER_BATCH_TY - 1) / WAFER_BATCH_TY;
    const dim3 grid((unsigned)(ntx * nty), (unsigned)g.nzl, (unsigned)nact), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    if (f32) hipLaunchKernelGGL(wafer_k_batch_normalise<float>, grid, block, 0, s, g, mem, act, ntx, norm2, n2_stride);
    else hipLaunchKernelGGL(wafer_k_batch_normalise<double>, grid, block, 0, s, g, mem, act, ntx, norm2, n2_stride);
    return hipGetLastError();
}
