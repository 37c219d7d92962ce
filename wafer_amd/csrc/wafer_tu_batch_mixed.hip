// translation unit: the batched ensemble kernels for a batch of SEVERAL shapes -- the templates of wafer_stencil_batch.hip.h and
// wafer_gs_batch.hip.h instantiated with the geometry taken from the batch's device table (WaferBatchGeomTable) instead of a
// kernel argument, for the three dtypes (0 f64 <double, double>, 1 f32 <float, double>, 2 f32fast <float, float>).  The per-cell
// text is the single-shape instantiations' (wafer_tu_batch.hip, wafer_tu_gs_batch.hip); only where the geometry and a member's
// partition come from differs.
#include <string.h>
#include "wafer_gs_batch.hip.h"

template <typename T, typename C>
static hipError_t launch_step(int R, WaferBatchGeomTable gt, const WaferBatchMember *mem, const WaferBatchBlock *blocks, int nblocks, int flip,
                              hipStream_t s)
{
    const dim3 grid((unsigned)nblocks), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    switch (R) {
    case 1: hipLaunchKernelGGL((wafer_k_batch_step<1, T, C, WaferBatchGeomTable>), grid, block, 0, s, gt, mem, blocks, flip); break;
    case 2: hipLaunchKernelGGL((wafer_k_batch_step<2, T, C, WaferBatchGeomTable>), grid, block, 0, s, gt, mem, blocks, flip); break;
    case 3: hipLaunchKernelGGL((wafer_k_batch_step<3, T, C, WaferBatchGeomTable>), grid, block, 0, s, gt, mem, blocks, flip); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t wafer_entry_batchm_step(int dtype, int R, const WaferGeom *geoms, const WaferBatchMember *mem, const WaferBatchBlock *blocks,
                                   int nblocks, int flip, hipStream_t s)
{
    const WaferBatchGeomTable gt{geoms};
    if (dtype == 0) return launch_step<double, double>(R, gt, mem, blocks, nblocks, flip, s);
    if (dtype == 1) return launch_step<float, double>(R, gt, mem, blocks, nblocks, flip, s);
    if (dtype == 2) return launch_step<float, float>(R, gt, mem, blocks, nblocks, flip, s);
    return hipErrorInvalidValue;
}

// the list of wafer_tu_batch.hip (wafer_batch_stepk_lds_bytes): ThreePoint 3 and 2 steps, FivePoint 2
template <typename T, typename C>
static hipError_t launch_stepk(int R, int K, WaferBatchGeomTable gt, const WaferBatchMember *mem, const WaferBatchBlock *blocks, int nblocks,
                               int flip, hipStream_t s)
{
    const dim3 grid((unsigned)nblocks), block(256);
    if (R == 1 && K == 3) hipLaunchKernelGGL((wafer_k_batch_stepk<1, 3, T, C, WaferBatchGeomTable>), grid, block, 0, s, gt, mem, blocks, flip);
    else if (R == 1 && K == 2) hipLaunchKernelGGL((wafer_k_batch_stepk<1, 2, T, C, WaferBatchGeomTable>), grid, block, 0, s, gt, mem, blocks, flip);
    else if (R == 2 && K == 2) hipLaunchKernelGGL((wafer_k_batch_stepk<2, 2, T, C, WaferBatchGeomTable>), grid, block, 0, s, gt, mem, blocks, flip);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t wafer_entry_batchm_stepk(int dtype, int R, int K, const WaferGeom *geoms, const WaferBatchMember *mem, const WaferBatchBlock *blocks,
                                    int nblocks, int flip, hipStream_t s)
{
    const WaferBatchGeomTable gt{geoms};
    if (dtype == 0) return launch_stepk<double, double>(R, K, gt, mem, blocks, nblocks, flip, s);
    if (dtype == 1) return launch_stepk<float, double>(R, K, gt, mem, blocks, nblocks, flip, s);
    if (dtype == 2) return launch_stepk<float, float>(R, K, gt, mem, blocks, nblocks, flip, s);
    return hipErrorInvalidValue;
}

template <typename T>
static hipError_t launch_observables(int R, WaferBatchGeomTable gt, const WaferBatchMember *mem, const int *act, dim3 grid, int swz,
                                     double *partials, hipStream_t s)
{
    // (ntx, nty, zchunk: the kernel takes them from the member's record)
    switch (R) {
    case 1: hipLaunchKernelGGL((wafer_k_batch_observables<1, 8, T, WaferBatchGeomTable>), grid, dim3(512), 0, s, gt, mem, act, 0, 0, 0, swz, partials); break;
    case 2: hipLaunchKernelGGL((wafer_k_batch_observables<2, 8, T, WaferBatchGeomTable>), grid, dim3(512), 0, s, gt, mem, act, 0, 0, 0, swz, partials); break;
    case 3: hipLaunchKernelGGL((wafer_k_batch_observables<3, 4, T, WaferBatchGeomTable>), grid, dim3(256), 0, s, gt, mem, act, 0, 0, 0, swz, partials); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t wafer_entry_batchm_observables(bool f32, int R, const WaferGeom *geoms, const WaferBatchMember *mem, const int *act, int nact,
                                          int max_nb, int swz, double *partials, double *out, hipStream_t s)
{
    const WaferBatchGeomTable gt{geoms};
    const dim3 grid((unsigned)max_nb, (unsigned)nact);
    const hipError_t e = f32 ? launch_observables<float>(R, gt, mem, act, grid, swz, partials, s)
                             : launch_observables<double>(R, gt, mem, act, grid, swz, partials, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wafer_k_batch_reduce_mixed, dim3(4, (unsigned)nact), dim3(256), 0, s, partials, act, mem, out);
    return hipGetLastError();
}

hipError_t wafer_entry_batchm_normalise(bool f32, const WaferGeom *geoms, const WaferBatchMember *mem, const int *act, int nact,
                                        int max_tiles, int max_planes, const double *norm2, int n2_stride, hipStream_t s)
{
    const WaferBatchGeomTable gt{geoms};
    const dim3 grid((unsigned)max_tiles, (unsigned)max_planes, (unsigned)nact), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    if (f32) hipLaunchKernelGGL((wafer_k_batch_normalise<float, WaferBatchGeomTable>), grid, block, 0, s, gt, mem, act, 0, norm2, n2_stride);
    else hipLaunchKernelGGL((wafer_k_batch_normalise<double, WaferBatchGeomTable>), grid, block, 0, s, gt, mem, act, 0, norm2, n2_stride);
    return hipGetLastError();
}

hipError_t wafer_entry_batchm_norm2(bool f32, const WaferGeom *geoms, const WaferBatchMember *mem, const int *act, int nact, int max_nb,
                                    double *scal, int scal_stride, int out_slot, double *partials, hipStream_t s)
{
    const dim3 grid((unsigned)max_nb, (unsigned)nact);
    if (f32) {
        const WaferBatchGeomTable gt{geoms};
        hipLaunchKernelGGL((wafer_k_batch_rownorm2<float, WaferBatchGeomTable>), grid, dim3(256), 0, s, gt, mem, act, partials);
    } else {
        WaferBatchGsArgsMixed a;
        memset(&a, 0, sizeof a);
        a.geoms = geoms;
        a.scal_stride = scal_stride;
        hipLaunchKernelGGL((wafer_k_batch_gs<WAFER_GS_NORM2, double, WaferBatchGsArgsMixed>), grid, dim3(WAFER_BATCH_TX, WAFER_BATCH_TY), 0, s, a, mem,
                           act, (const double *)scal, partials);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wafer_k_batch_gs_reduce_mixed, dim3((unsigned)nact), dim3(256), 0, s, (const double *)partials, act, mem, scal, scal_stride, out_slot);
    return hipGetLastError();
}
