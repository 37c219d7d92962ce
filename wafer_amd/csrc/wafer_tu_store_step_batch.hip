// translation unit: the store step of a batch of ONE shape (the geometry is a kernel argument: wafer_tu_store_step_batch.inc), and the
// batched copy that brings the stepped states back into the slots after an odd number of steps
#define WAFER_TU_BATCH_GS WaferGeom
#include "wafer_tu_store_step_batch.inc"

hipError_t wafer_entry_batch_store_copy(const WaferBatchRitzRec *act, int nact, int blocks, const WaferRitzPtrs &src, const WaferRitzPtrs &dst,
                                        hipStream_t s)
{
    if (nact < 1 || nact > 65535 || blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wafer_k_batch_store_copy, dim3((unsigned)blocks, (unsigned)nact), dim3(256), 0, s, act, src, dst);
    return hipGetLastError();
}
