// translation unit: the batched excited-state kernels (wafer_gs_batch.hip.h)
#include "wafer_gs_batch.hip.h"

hipError_t wafer_entry_batch_gs(int mode, const WaferBatchGsArgs &a, const WaferBatchMember *mem, const int *act, int nact,
                                double *scal, int out_slot, double *partials, hipStream_t s)
{
    const int nb = wafer_gs_blocks(a.g);
    const dim3 grid((unsigned)nb, (unsigned)nact), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    switch (mode) {
    case WAFER_GS_NORM2: hipLaunchKernelGGL((wafer_k_batch_gs<WAFER_GS_NORM2>), grid, block, 0, s, a, mem, act, scal, partials); break;
    case WAFER_GS_DOT: hipLaunchKernelGGL((wafer_k_batch_gs<WAFER_GS_DOT>), grid, block, 0, s, a, mem, act, scal, partials); break;
    case WAFER_GS_SCALE: hipLaunchKernelGGL((wafer_k_batch_gs<WAFER_GS_SCALE>), grid, block, 0, s, a, mem, act, scal, partials); break;
    case WAFER_GS_AXPY: hipLaunchKernelGGL((wafer_k_batch_gs<WAFER_GS_AXPY>), grid, block, 0, s, a, mem, act, scal, partials); break;
    default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !(mode == WAFER_GS_NORM2 || a.dotwith)) return e;
    hipLaunchKernelGGL(wafer_k_batch_gs_reduce, dim3((unsigned)nact), dim3(256), 0, s, partials, act, nb, scal, a.scal_stride, out_slot);
    return hipGetLastError();
}
