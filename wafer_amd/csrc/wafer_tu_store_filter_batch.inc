// The launch layer of the store filter (wafer_store_filter_batch.hip.h), written once for both geometry sources: the including unit
// names its own as WAFER_TU_BATCH_GS (WaferGeom: wafer_tu_store_filter_batch.hip; WaferBatchGeomTable:
// wafer_tu_store_filter_batch_mixed.hip) and gets the wafer_entry_batch_store_filter and wafer_entry_batch_v_max overloads that take
// that type.
#include "wafer_store_filter_batch.hip.h"

namespace {

using GS = WAFER_TU_BATCH_GS;

template <typename T>
hipError_t launch_store_filter(int R, const GS &gs, const WaferBatchMember *mem, const WaferBatchBlock *blocks, int nblocks, int groups, const int *kk,
                               const WaferFilterCoef *coef, int first, const WaferRitzPtrs &cur, const WaferRitzPtrs &out, hipStream_t s)
{
    const dim3 grid((unsigned)nblocks, (unsigned)groups), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    switch (R) {
    case 1: hipLaunchKernelGGL((wafer_k_batch_store_filter<1, T, GS>), grid, block, 0, s, gs, mem, blocks, kk, coef, first, cur, out); break;
    case 2: hipLaunchKernelGGL((wafer_k_batch_store_filter<2, T, GS>), grid, block, 0, s, gs, mem, blocks, kk, coef, first, cur, out); break;
    case 3: hipLaunchKernelGGL((wafer_k_batch_store_filter<3, T, GS>), grid, block, 0, s, gs, mem, blocks, kk, coef, first, cur, out); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace

hipError_t wafer_entry_batch_store_filter(bool f32, int R, const GS &gs, const WaferBatchMember *mem, const WaferBatchBlock *blocks, int nblocks,
                                          int groups, const int *kk, const WaferFilterCoef *coef, int first, const WaferRitzPtrs &cur,
                                          const WaferRitzPtrs &out, hipStream_t s)
{
    if (nblocks < 1 || groups < 1 || groups > WAFER_RITZ_MAX / WAFER_STORE_SG) return hipErrorInvalidValue;
    if (f32) return launch_store_filter<float>(R, gs, mem, blocks, nblocks, groups, kk, coef, first, cur, out, s);
    return launch_store_filter<double>(R, gs, mem, blocks, nblocks, groups, kk, coef, first, cur, out, s);
}

hipError_t wafer_entry_batch_v_max(bool f32, const GS &gs, const WaferBatchMember *mem, const int *act, int nact, int max_tiles, int max_planes,
                                   unsigned long long *words, hipStream_t s)
{
    if (nact < 1 || max_tiles < 1 || max_planes < 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)max_tiles, (unsigned)max_planes, (unsigned)nact), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    if (f32) hipLaunchKernelGGL((wafer_k_batch_v_max<float, GS>), grid, block, 0, s, gs, mem, act, words);
    else hipLaunchKernelGGL((wafer_k_batch_v_max<double, GS>), grid, block, 0, s, gs, mem, act, words);
    return hipGetLastError();
}
