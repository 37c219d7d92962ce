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

template <int NLOW, typename T>
static hipError_t launch_onepass(bool normalise, const WaferBatchGsOneArgs &a, const WaferBatchMember *mem, const int *act, int nact, int nb,
                                 double *scal, const double *gram, double *partials, hipStream_t s)
{
    const dim3 grid((unsigned)nb, (unsigned)nact), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    hipLaunchKernelGGL((wafer_k_batch_gs_sums<NLOW, T>), grid, block, 0, s, a, mem, act, partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((wafer_k_batch_gs_reduce_sums<false>), dim3((unsigned)nact, 1 + NLOW), dim3(256), 0, s, partials, act, nb, WAFER_GS_ONE_ROWS,
                       scal, a.scal_stride);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (normalise) hipLaunchKernelGGL((wafer_k_batch_gs_apply<NLOW, T, true>), grid, block, 0, s, a, mem, act, scal, gram);
    else hipLaunchKernelGGL((wafer_k_batch_gs_apply<NLOW, T, false>), grid, block, 0, s, a, mem, act, scal, gram);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_onepass_n(int nlow, bool normalise, const WaferBatchGsOneArgs &a, const WaferBatchMember *mem, const int *act, int nact,
                                   int nb, double *scal, const double *gram, double *partials, hipStream_t s)
{
    switch (nlow) {
    case 1: return launch_onepass<1, T>(normalise, a, mem, act, nact, nb, scal, gram, partials, s);
    case 2: return launch_onepass<2, T>(normalise, a, mem, act, nact, nb, scal, gram, partials, s);
    case 3: return launch_onepass<3, T>(normalise, a, mem, act, nact, nb, scal, gram, partials, s);
    case 4: return launch_onepass<4, T>(normalise, a, mem, act, nact, nb, scal, gram, partials, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t wafer_entry_batch_gs_onepass(bool f32, int nlow, bool normalise, const WaferBatchGsOneArgs &a, const WaferBatchMember *mem,
                                        const int *act, int nact, double *scal, const double *gram, double *partials, hipStream_t s)
{
    const int nb = wafer_gs_blocks(a.g);
    return f32 ? launch_onepass_n<float>(nlow, normalise, a, mem, act, nact, nb, scal, gram, partials, s)
               : launch_onepass_n<double>(nlow, normalise, a, mem, act, nact, nb, scal, gram, partials, s);
}

template <typename T>
static hipError_t launch_gram(int nl, const WaferBatchGsOneArgs &a, const int *list, const int *cnt, dim3 grid, dim3 block, double *partials,
                              hipStream_t s)
{
    switch (nl) {
    case 2: hipLaunchKernelGGL((wafer_k_batch_gram<2, T>), grid, block, 0, s, a, list, cnt, partials); break;
    case 3: hipLaunchKernelGGL((wafer_k_batch_gram<3, T>), grid, block, 0, s, a, list, cnt, partials); break;
    case 4: hipLaunchKernelGGL((wafer_k_batch_gram<4, T>), grid, block, 0, s, a, list, cnt, partials); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t wafer_entry_batch_gram(bool f32, int nl, const WaferBatchGsOneArgs &a, const int *list, const int *cnt, int nlist, double *gram,
                                  double *partials, hipStream_t s)
{
    const int nb = wafer_gs_blocks(a.g);
    const dim3 grid((unsigned)nb, (unsigned)nlist), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    const hipError_t e = f32 ? launch_gram<float>(nl, a, list, cnt, grid, block, partials, s) : launch_gram<double>(nl, a, list, cnt, grid, block, partials, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((wafer_k_batch_gs_reduce_sums<true>), dim3((unsigned)nlist, (unsigned)(nl * (nl - 1) / 2)), dim3(256), 0, s, partials, list, nb,
                       WAFER_GRAM_PAIRS, gram, WAFER_MAX_LOW * WAFER_MAX_LOW);
    return hipGetLastError();
}
