// The launch layer of the store step (wafer_store_step_batch.hip.h), written once for both geometry sources: the including unit names
// its own as WAFER_TU_BATCH_GS (WaferGeom: wafer_tu_store_step_batch.hip; WaferBatchGeomTable: wafer_tu_store_step_batch_mixed.hip) and
// gets the wafer_entry_batch_store_step overload that takes that type.
#include "wafer_store_step_batch.hip.h"

namespace {

using GS = WAFER_TU_BATCH_GS;

template <typename T, typename C>
hipError_t launch_store_step(int R, const GS &gs, const WaferBatchMember *mem, const WaferBatchBlock *blocks, int nblocks, int groups, const int *kk,
                             const WaferRitzPtrs &src, const WaferRitzPtrs &dst, hipStream_t s)
{
    const dim3 grid((unsigned)nblocks, (unsigned)groups), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    switch (R) {
    case 1: hipLaunchKernelGGL((wafer_k_batch_store_step<1, T, C, GS>), grid, block, 0, s, gs, mem, blocks, kk, src, dst); break;
    case 2: hipLaunchKernelGGL((wafer_k_batch_store_step<2, T, C, GS>), grid, block, 0, s, gs, mem, blocks, kk, src, dst); break;
    case 3: hipLaunchKernelGGL((wafer_k_batch_store_step<3, T, C, GS>), grid, block, 0, s, gs, mem, blocks, kk, src, dst); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace

hipError_t wafer_entry_batch_store_step(int dtype, int R, const GS &gs, const WaferBatchMember *mem, const WaferBatchBlock *blocks, int nblocks,
                                        int groups, const int *kk, const WaferRitzPtrs &src, const WaferRitzPtrs &dst, hipStream_t s)
{
    if (nblocks < 1 || groups < 1 || groups > WAFER_RITZ_MAX / WAFER_STORE_SG) return hipErrorInvalidValue;
    if (dtype == 0) return launch_store_step<double, double>(R, gs, mem, blocks, nblocks, groups, kk, src, dst, s);
    if (dtype == 1) return launch_store_step<float, double>(R, gs, mem, blocks, nblocks, groups, kk, src, dst, s);
    if (dtype == 2) return launch_store_step<float, float>(R, gs, mem, blocks, nblocks, groups, kk, src, dst, s);
    return hipErrorInvalidValue;
}
