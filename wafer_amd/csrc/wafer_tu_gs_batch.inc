// The launch layer of the batched excited-state kernels (wafer_gs_batch.hip.h), written once for both geometry sources.  The
// including unit names its own as WAFER_TU_BATCH_GS, as for wafer_tu_batch.inc: WaferGeom (wafer_tu_gs_batch.hip, a batch of one
// shape) or WaferBatchGeomTable (wafer_tu_gs_batch_mixed.hip, several shapes with state stores), and gets the
// wafer_entry_batch_gs* overloads that take that type.
#include "wafer_gs_batch.hip.h"

namespace {

using GS = WAFER_TU_BATCH_GS;

template <typename T>
hipError_t launch_gs(int mode, const GS &gs, const WaferBatchGsArgs &a, const WaferBatchMember *mem, const int *act, dim3 grid, dim3 block,
                     const double *scal, double *partials, hipStream_t s)
{
    switch (mode) {
    case WAFER_GS_NORM2: hipLaunchKernelGGL((wafer_k_batch_gs<WAFER_GS_NORM2, T, GS>), grid, block, 0, s, gs, a, mem, act, scal, partials); break;
    case WAFER_GS_DOT: hipLaunchKernelGGL((wafer_k_batch_gs<WAFER_GS_DOT, T, GS>), grid, block, 0, s, gs, a, mem, act, scal, partials); break;
    case WAFER_GS_SCALE: hipLaunchKernelGGL((wafer_k_batch_gs<WAFER_GS_SCALE, T, GS>), grid, block, 0, s, gs, a, mem, act, scal, partials); break;
    case WAFER_GS_AXPY: hipLaunchKernelGGL((wafer_k_batch_gs<WAFER_GS_AXPY, T, GS>), grid, block, 0, s, gs, a, mem, act, scal, partials); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int NLOW, typename T>
hipError_t launch_onepass(bool normalise, const GS &gs, const WaferBatchGsOneArgs &a, const WaferBatchMember *mem, const int *act, int nact, int nb,
                          double *scal, const double *gram, double *partials, hipStream_t s)
{
    const dim3 grid((unsigned)nb, (unsigned)nact), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    hipLaunchKernelGGL((wafer_k_batch_gs_sums<NLOW, T, GS>), grid, block, 0, s, gs, a, mem, act, partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((wafer_k_batch_gs_reduce_sums<false>), dim3((unsigned)nact, 1 + NLOW), dim3(256), 0, s, (const double *)partials, act,
                       WAFER_GS_ONE_ROWS, scal, a.scal_stride, mem);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (normalise) hipLaunchKernelGGL((wafer_k_batch_gs_apply<NLOW, T, true, GS>), grid, block, 0, s, gs, a, mem, act, (const double *)scal, gram);
    else hipLaunchKernelGGL((wafer_k_batch_gs_apply<NLOW, T, false, GS>), grid, block, 0, s, gs, a, mem, act, (const double *)scal, gram);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_onepass_n(int nlow, bool normalise, const GS &gs, const WaferBatchGsOneArgs &a, const WaferBatchMember *mem, const int *act,
                            int nact, int nb, double *scal, const double *gram, double *partials, hipStream_t s)
{
    switch (nlow) {
    case 1: return launch_onepass<1, T>(normalise, gs, a, mem, act, nact, nb, scal, gram, partials, s);
    case 2: return launch_onepass<2, T>(normalise, gs, a, mem, act, nact, nb, scal, gram, partials, s);
    case 3: return launch_onepass<3, T>(normalise, gs, a, mem, act, nact, nb, scal, gram, partials, s);
    case 4: return launch_onepass<4, T>(normalise, gs, a, mem, act, nact, nb, scal, gram, partials, s);
    default: return hipErrorInvalidValue;
    }
}

template <typename T>
hipError_t launch_gram(int nl, const GS &gs, const WaferBatchGsOneArgs &a, const WaferBatchMember *mem, const int *list, const int *cnt, dim3 grid,
                       dim3 block, double *partials, hipStream_t s)
{
    switch (nl) {
    case 2: hipLaunchKernelGGL((wafer_k_batch_gram<2, T, GS>), grid, block, 0, s, gs, a, mem, list, cnt, partials); break;
    case 3: hipLaunchKernelGGL((wafer_k_batch_gram<3, T, GS>), grid, block, 0, s, gs, a, mem, list, cnt, partials); break;
    case 4: hipLaunchKernelGGL((wafer_k_batch_gram<4, T, GS>), grid, block, 0, s, gs, a, mem, list, cnt, partials); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace

hipError_t wafer_entry_batch_gs(bool f32, int mode, const GS &gs, const WaferBatchGsArgs &a, const WaferBatchMember *mem, const int *act, int nact,
                                int max_nb, double *scal, int out_slot, double *partials, hipStream_t s)
{
    const dim3 grid((unsigned)max_nb, (unsigned)nact), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    const hipError_t e = f32 ? launch_gs<float>(mode, gs, a, mem, act, grid, block, scal, partials, s)
                             : launch_gs<double>(mode, gs, a, mem, act, grid, block, scal, partials, s);
    if (e != hipSuccess || !(mode == WAFER_GS_NORM2 || a.dotwith)) return e;
    hipLaunchKernelGGL(wafer_k_batch_gs_reduce<false>, dim3((unsigned)nact), dim3(256), 0, s, (const double *)partials, act, mem, scal, a.scal_stride,
                       out_slot);
    return hipGetLastError();
}

hipError_t wafer_entry_batch_gs_onepass(bool f32, int nlow, bool normalise, const GS &gs, const WaferBatchGsOneArgs &a, const WaferBatchMember *mem,
                                        const int *act, int nact, int max_nb, double *scal, const double *gram, double *partials, hipStream_t s)
{
    return f32 ? launch_onepass_n<float>(nlow, normalise, gs, a, mem, act, nact, max_nb, scal, gram, partials, s)
               : launch_onepass_n<double>(nlow, normalise, gs, a, mem, act, nact, max_nb, scal, gram, partials, s);
}

hipError_t wafer_entry_batch_gram(bool f32, int nl, const GS &gs, const WaferBatchGsOneArgs &a, const WaferBatchMember *mem, const int *list,
                                  const int *cnt, int nlist, int max_nb, double *gram, double *partials, hipStream_t s)
{
    const dim3 grid((unsigned)max_nb, (unsigned)nlist), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    const hipError_t e = f32 ? launch_gram<float>(nl, gs, a, mem, list, cnt, grid, block, partials, s)
                             : launch_gram<double>(nl, gs, a, mem, list, cnt, grid, block, partials, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((wafer_k_batch_gs_reduce_sums<true>), dim3((unsigned)nlist, (unsigned)(nl * (nl - 1) / 2)), dim3(256), 0, s,
                       (const double *)partials, list, WAFER_GRAM_PAIRS, gram, WAFER_MAX_LOW * WAFER_MAX_LOW, mem);
    return hipGetLastError();
}
