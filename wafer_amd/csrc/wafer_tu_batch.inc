// The launch layer of the batched ensemble kernels (wafer_stencil_batch.hip.h, wafer_gs_batch.hip.h, wafer_setup_batch.hip.h), written once for both
// geometry sources.  The including unit names its own as WAFER_TU_BATCH_GS: WaferGeom (wafer_tu_batch.hip: the one geometry of
// a batch of one shape, a kernel argument) or WaferBatchGeomTable (wafer_tu_batch_mixed.hip: the device table of a batch of
// several shapes), and gets the wafer_entry_batch_* overloads that take that type.  For each dtype -- 0 f64 <double, double>,
// 1 f32 <float, double> (float storage, fp64 arithmetic), 2 f32fast <float, float> (float arithmetic in the ground-state step).
#include "wafer_gs_batch.hip.h"
#include "wafer_resample_batch.hip.h"
#include "wafer_setup_batch.hip.h"

namespace {

using GS = WAFER_TU_BATCH_GS;

template <typename T, typename C>
hipError_t launch_step(int R, const GS &gs, const WaferBatchMember *mem, const WaferBatchBlock *blocks, int nblocks, int flip, hipStream_t s)
{
    const dim3 grid((unsigned)nblocks), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    switch (R) {
    case 1: hipLaunchKernelGGL((wafer_k_batch_step<1, T, C, GS>), grid, block, 0, s, gs, mem, blocks, flip); break;
    case 2: hipLaunchKernelGGL((wafer_k_batch_step<2, T, C, GS>), grid, block, 0, s, gs, mem, blocks, flip); break;
    case 3: hipLaunchKernelGGL((wafer_k_batch_step<3, T, C, GS>), grid, block, 0, s, gs, mem, blocks, flip); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// the instantiations of the fused pass (wafer_batch_stepk_lds_bytes), the same list for every dtype and geometry source:
// ThreePoint 3 steps (and 2, for the remainder of a call), FivePoint 2 steps
template <typename T, typename C>
hipError_t launch_stepk(int R, int K, const GS &gs, const WaferBatchMember *mem, const WaferBatchBlock *blocks, int nblocks, int flip,
                        hipStream_t s)
{
    const dim3 grid((unsigned)nblocks), block(256);
    if (R == 1 && K == 3) hipLaunchKernelGGL((wafer_k_batch_stepk<1, 3, T, C, GS>), grid, block, 0, s, gs, mem, blocks, flip);
    else if (R == 1 && K == 2) hipLaunchKernelGGL((wafer_k_batch_stepk<1, 2, T, C, GS>), grid, block, 0, s, gs, mem, blocks, flip);
    else if (R == 2 && K == 2) hipLaunchKernelGGL((wafer_k_batch_stepk<2, 2, T, C, GS>), grid, block, 0, s, gs, mem, blocks, flip);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

template <typename T>
hipError_t launch_observables(int R, const GS &gs, const WaferBatchMember *mem, const int *act, dim3 grid, int swz, double *partials,
                              hipStream_t s)
{
    // the waves per workgroup of wafer_launch_observables_lds: 8 (ThreePoint / FivePoint), 4 (SevenPoint)
    switch (R) {
    case 1: hipLaunchKernelGGL((wafer_k_batch_observables<1, 8, T, GS>), grid, dim3(512), 0, s, gs, mem, act, swz, partials); break;
    case 2: hipLaunchKernelGGL((wafer_k_batch_observables<2, 8, T, GS>), grid, dim3(512), 0, s, gs, mem, act, swz, partials); break;
    case 3: hipLaunchKernelGGL((wafer_k_batch_observables<3, 4, T, GS>), grid, dim3(256), 0, s, gs, mem, act, swz, partials); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace

hipError_t wafer_entry_batch_step(int dtype, int R, const GS &gs, const WaferBatchMember *mem, const WaferBatchBlock *blocks, int nblocks, int flip,
                                  hipStream_t s)
{
    if (dtype == 0) return launch_step<double, double>(R, gs, mem, blocks, nblocks, flip, s);
    if (dtype == 1) return launch_step<float, double>(R, gs, mem, blocks, nblocks, flip, s);
    if (dtype == 2) return launch_step<float, float>(R, gs, mem, blocks, nblocks, flip, s);
    return hipErrorInvalidValue;
}

hipError_t wafer_entry_batch_stepk(int dtype, int R, int K, const GS &gs, const WaferBatchMember *mem, const WaferBatchBlock *blocks, int nblocks,
                                   int flip, hipStream_t s)
{
    if (dtype == 0) return launch_stepk<double, double>(R, K, gs, mem, blocks, nblocks, flip, s);
    if (dtype == 1) return launch_stepk<float, double>(R, K, gs, mem, blocks, nblocks, flip, s);
    if (dtype == 2) return launch_stepk<float, float>(R, K, gs, mem, blocks, nblocks, flip, s);
    return hipErrorInvalidValue;
}

hipError_t wafer_entry_batch_observables(bool f32, int R, const GS &gs, const WaferBatchMember *mem, const int *act, int nact, int max_nb, int swz,
                                         double *partials, double *out, hipStream_t s)
{
    const dim3 grid((unsigned)max_nb, (unsigned)nact);
    const hipError_t e = f32 ? launch_observables<float>(R, gs, mem, act, grid, swz, partials, s)
                             : launch_observables<double>(R, gs, mem, act, grid, swz, partials, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wafer_k_batch_reduce, dim3(4, (unsigned)nact), dim3(256), 0, s, partials, act, mem, out);
    return hipGetLastError();
}

hipError_t wafer_entry_batch_normalise(bool f32, const GS &gs, const WaferBatchMember *mem, const int *act, int nact, int max_tiles,
                                       int max_planes, const double *norm2, int n2_stride, hipStream_t s)
{
    const dim3 grid((unsigned)max_tiles, (unsigned)max_planes, (unsigned)nact), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    if (f32) hipLaunchKernelGGL((wafer_k_batch_normalise<float, GS>), grid, block, 0, s, gs, mem, act, norm2, n2_stride);
    else hipLaunchKernelGGL((wafer_k_batch_normalise<double, GS>), grid, block, 0, s, gs, mem, act, norm2, n2_stride);
    return hipGetLastError();
}

hipError_t wafer_entry_batch_symmetrise(bool f32, const GS &gs, const WaferBatchMember *mem, const int *act, int nact, const int *sym,
                                        int max_tiles, int max_planes, hipStream_t s)
{
    const dim3 grid((unsigned)max_tiles, (unsigned)max_planes, (unsigned)nact), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    if (f32) hipLaunchKernelGGL((wafer_k_batch_symmetrise<float, GS>), grid, block, 0, s, gs, mem, act, sym);
    else hipLaunchKernelGGL((wafer_k_batch_symmetrise<double, GS>), grid, block, 0, s, gs, mem, act, sym);
    return hipGetLastError();
}

hipError_t wafer_entry_batch_trilerp(bool f32, bool src_f32, const GS &gs, const WaferBatchMember *mem, const int *act, int nact,
                                     int max_tiles, int max_planes, const WaferResampleSource &src, void *dst0, void *dst1, int by_cur, int basis,
                                     hipStream_t s)
{
    if (src_f32 && !f32) return hipErrorInvalidValue;   // (a member source has the batch's storage type)
    const dim3 grid((unsigned)max_tiles, (unsigned)max_planes, (unsigned)nact), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    if (!f32) hipLaunchKernelGGL((wafer_k_batch_trilerp<double, double, GS>), grid, block, 0, s, gs, mem, act, src, dst0, dst1, by_cur, basis);
    else if (src_f32) hipLaunchKernelGGL((wafer_k_batch_trilerp<float, float, GS>), grid, block, 0, s, gs, mem, act, src, dst0, dst1, by_cur, basis);
    else hipLaunchKernelGGL((wafer_k_batch_trilerp<float, double, GS>), grid, block, 0, s, gs, mem, act, src, dst0, dst1, by_cur, basis);
    return hipGetLastError();
}

hipError_t wafer_entry_batch_norm2(bool f32, const GS &gs, const WaferBatchMember *mem, const int *act, int nact, int max_nb, double *scal,
                                   int scal_stride, int out_slot, double *partials, hipStream_t s)
{
    const dim3 grid((unsigned)max_nb, (unsigned)nact);
    if (f32) {
        hipLaunchKernelGGL((wafer_k_batch_rownorm2<float, GS>), grid, dim3(256), 0, s, gs, mem, act, partials);
    } else {   // the chain's NORM2 mode reads no store slot
        const WaferBatchGsArgs a{0, scal_stride, 0, nullptr, nullptr};
        hipLaunchKernelGGL((wafer_k_batch_gs<WAFER_GS_NORM2, double, GS>), grid, dim3(WAFER_BATCH_TX, WAFER_BATCH_TY), 0, s, gs, a, mem, act,
                           (const double *)scal, partials);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (f32) hipLaunchKernelGGL(wafer_k_batch_gs_reduce<true>, dim3((unsigned)nact), dim3(256), 0, s, (const double *)partials, act, mem, scal, scal_stride, out_slot);
    else hipLaunchKernelGGL(wafer_k_batch_gs_reduce<false>, dim3((unsigned)nact), dim3(256), 0, s, (const double *)partials, act, mem, scal, scal_stride, out_slot);
    return hipGetLastError();
}

// ---- set-up (wafer_setup_batch.hip.h) ----------------------------------------------------------------------------------------
hipError_t wafer_entry_batch_potential(bool f32, const GS &gs, const WaferBatchMember *mem, const WaferBatchSetupRec *rec, int nlisted,
                                       int max_tiles, int max_planes, hipStream_t s)
{
    const dim3 grid((unsigned)max_tiles, (unsigned)max_planes, (unsigned)nlisted), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    if (f32) hipLaunchKernelGGL((wafer_k_batch_potential<float, GS>), grid, block, 0, s, gs, mem, rec);
    else hipLaunchKernelGGL((wafer_k_batch_potential<double, GS>), grid, block, 0, s, gs, mem, rec);
    return hipGetLastError();
}

hipError_t wafer_entry_batch_potsub_fullcornell(bool f32, const GS &gs, const WaferBatchMember *mem, const WaferBatchSetupRec *rec, int nlisted,
                                                int max_tiles, int max_planes, hipStream_t s)
{
    const dim3 grid((unsigned)max_tiles, (unsigned)max_planes, (unsigned)nlisted), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    if (f32) hipLaunchKernelGGL((wafer_k_batch_potsub_fullcornell<float, GS>), grid, block, 0, s, gs, mem, rec);
    else hipLaunchKernelGGL((wafer_k_batch_potsub_fullcornell<double, GS>), grid, block, 0, s, gs, mem, rec);
    return hipGetLastError();
}

hipError_t wafer_entry_batch_initial_condition(bool f32, const GS &gs, const WaferBatchMember *mem, const WaferBatchSetupRec *rec, int nlisted,
                                               int max_tiles, int max_planes, hipStream_t s)
{
    const dim3 grid((unsigned)max_tiles, (unsigned)max_planes, (unsigned)nlisted), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    if (f32) hipLaunchKernelGGL((wafer_k_batch_initial_condition<float, GS>), grid, block, 0, s, gs, mem, rec);
    else hipLaunchKernelGGL((wafer_k_batch_initial_condition<double, GS>), grid, block, 0, s, gs, mem, rec);
    return hipGetLastError();
}

hipError_t wafer_entry_batch_v_check(bool f32, const GS &gs, const WaferBatchMember *mem, const int *act, int nact, int max_tiles, int max_planes,
                                     unsigned long long *words, hipStream_t s)
{
    const dim3 grid((unsigned)max_tiles, (unsigned)max_planes, (unsigned)nact), block(WAFER_BATCH_TX, WAFER_BATCH_TY);
    if (f32) hipLaunchKernelGGL((wafer_k_batch_v_check<float, GS>), grid, block, 0, s, gs, mem, act, words);
    else hipLaunchKernelGGL((wafer_k_batch_v_check<double, GS>), grid, block, 0, s, gs, mem, act, words);
    return hipGetLastError();
}
