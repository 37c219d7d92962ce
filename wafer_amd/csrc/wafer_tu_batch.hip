// translation unit: the batched ensemble kernels (wafer_stencil_batch.hip.h)
#include "wafer_stencil_batch.hip.h"

hipError_t wafer_entry_batch_step(int R, const WaferGeom &g, const WaferBatchMember *mem, const WaferBatchBlock *blocks, int nblocks,
                                  int flip, hipStream_t s)
{
    const dim3 grid((unsigned)nblocks), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    switch (R) {
    case 1: hipLaunchKernelGGL((wafer_k_batch_step<1>), grid, block, 0, s, g, mem, blocks, flip); break;
    case 2: hipLaunchKernelGGL((wafer_k_batch_step<2>), grid, block, 0, s, g, mem, blocks, flip); break;
    case 3: hipLaunchKernelGGL((wafer_k_batch_step<3>), grid, block, 0, s, g, mem, blocks, flip); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// the instantiations of the fused pass: ThreePoint 3 steps (and 2, for the remainder of a call), FivePoint 2 steps
int wafer_batch_stepk_lds_bytes(int R, int K)
{
    if (R == 1 && K == 3) return WaferBatchKCfg<1, 3>::LDS_BYTES;
    if (R == 1 && K == 2) return WaferBatchKCfg<1, 2>::LDS_BYTES;
    if (R == 2 && K == 2) return WaferBatchKCfg<2, 2>::LDS_BYTES;
    return 0;
}

hipError_t wafer_entry_batch_stepk(int R, int K, const WaferGeom &g, const WaferBatchMember *mem, const WaferBatchBlock *blocks,
                                   int nblocks, int flip, hipStream_t s)
{
    const dim3 grid((unsigned)nblocks), block(256);
    if (R == 1 && K == 3) hipLaunchKernelGGL((wafer_k_batch_stepk<1, 3>), grid, block, 0, s, g, mem, blocks, flip);
    else if (R == 1 && K == 2) hipLaunchKernelGGL((wafer_k_batch_stepk<1, 2>), grid, block, 0, s, g, mem, blocks, flip);
    else if (R == 2 && K == 2) hipLaunchKernelGGL((wafer_k_batch_stepk<2, 2>), grid, block, 0, s, g, mem, blocks, flip);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t wafer_entry_batch_observables(int R, const WaferGeom &g, const WaferBatchMember *mem, const int *act, int nact, int ntx,
                                         int nty, int nblocks, int zchunk, int swz, double *partials, double *out, hipStream_t s)
{
    const dim3 grid((unsigned)nblocks, (unsigned)nact);
    // the waves per workgroup of wafer_launch_observables_lds: 8 (ThreePoint / FivePoint), 4 (SevenPoint)
    switch (R) {
    case 1: hipLaunchKernelGGL((wafer_k_batch_observables<1, 8>), grid, dim3(512), 0, s, g, mem, act, ntx, nty, zchunk, swz, partials); break;
    case 2: hipLaunchKernelGGL((wafer_k_batch_observables<2, 8>), grid, dim3(512), 0, s, g, mem, act, ntx, nty, zchunk, swz, partials); break;
    case 3: hipLaunchKernelGGL((wafer_k_batch_observables<3, 4>), grid, dim3(256), 0, s, g, mem, act, ntx, nty, zchunk, swz, partials); break;
    default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wafer_k_batch_reduce, dim3(4, (unsigned)nact), dim3(256), 0, s, partials, act, (long long)nblocks, out);
    return hipGetLastError();
}

hipError_t wafer_entry_batch_normalise(const WaferGeom &g, const WaferBatchMember *mem, const int *act, int nact, const double *norm2,
                                       int n2_stride, hipStream_t s)
{
    const int ntx = (g.nx + WAFER_BATCH_TX - 1) / WAFER_BATCH_TX, nty = (g.ny + WAFER_BATCH_TY - 1) / WAFER_BATCH_TY;
    hipLaunchKernelGGL(wafer_k_batch_normalise, dim3((unsigned)(ntx * nty), (unsigned)g.nzl, (unsigned)nact),
                       dim3(WAFER_BATCH_TX, WAFER_BATCH_TY), 0, s, g, mem, act, ntx, norm2, n2_stride);
    return hipGetLastError();
}
