// translation unit: the batched excited-state kernels (wafer_gs_batch.hip.h)
#include "wafer_gs_batch.hip.h"

template <typename T>
static hipError_t launch_gs(int mode, const WaferBatchGsArgs &a, const WaferBatchMember *mem, const int *act, dim3 grid, dim3 block,
                            const double *scal, double *partials, hipStream_t s)
{
    switch (mode) {
    case WAFER_GS_NORM2: hipLaunchKernelGGL((wafer_k_batch_gs<WAFER_GS_NORM2, T>), grid, block, 0, s, a, mem, act, scal, partials); break;
    case WAFER_GS_DOT: hipLaunchKernelGGL((wafer_k_batch_gs<WAFER_GS_DOT, T>), grid, block, 0, s, a, mem, act, scal, partials); break;
    case WAFER_GS_SCALE: hipLaunchKernelGGL((wafer_k_batch_gs<WAFER_GS_SCALE, T>), grid, block, 0, s, a, mem, act, scal, partials); break;
    case WAFER_GS_AXPY: hipLaunchKernelGGL((wafer_k_batch_gs<WAFER_GS_AXPY, T>), grid, block, 0, s, a, mem, act, scal, partials); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t wafer_entry_batch_gs(bool f32, int mode, const WaferBatchGsArgs &a, const WaferBatchMember *mem, const int *act, int nact,
                                double *scal, int out_slot, double *partials, hipStream_t s)
{
    const int nb = wafer_gs_blocks(a.g);
    const dim3 grid((unsigned)nb, (unsigned)nact), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    const hipError_t e = f32 ? launch_gs<float>(mode, a, mem, act, grid, block, scal, partials, s)
                             : launch_gs<double>(mode, a, mem, act, grid, block, scal, partials, s);
    if (e != hipSuccess || !(mode == WAFER_GS_NORM2 || a.dotwith)) return e;
    hipLaunchKernelGGL(wafer_k_batch_gs_reduce, dim3((unsigned)nact), dim3(256), 0, s, partials, act, nb, scal, a.scal_stride, out_slot);
    return hipGetLastError();
}

hipError_t wafer_entry_batch_rownorm2(const WaferGeom &g, const WaferBatchMember *mem, const int *act, int nact, int nb, double *scal,
                                      int scal_stride, int out_slot, double *partials, hipStream_t s)
{
    WaferRowArgs ra;
    ra.g = g;
    ra.lz_lo = g.G;
    ra.lz_hi = g.G + g.nzl;
    hipLaunchKernelGGL((wafer_k_batch_rownorm2<float>), dim3((unsigned)nb, (unsigned)nact), dim3(256), 0, s, ra, mem, act, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wafer_k_batch_gs_reduce, dim3((unsigned)nact), dim3(256), 0, s, partials, act, nb, scal, scal_stride, out_slot);
    return hipGetLastError();
}
