// translation unit: moment matrices of the stored states of a batch (wafer_moments_batch.hip.h) -- the sums kernel for both geometry
// sources (WaferGeom: a batch of one shape; WaferBatchGeomTable: several shapes with state stores) and its reduce
#include "wafer_moments_batch.hip.h"

namespace {

template <int R, typename T, typename GS>
hipError_t launch_sums(const GS &gs, const WaferBatchMember *mem, const WaferBatchMomentRec *act, int nact, int max_nb, int max_k, int swz,
                       const WaferRitzPtrs &st, double *partials, double *sums, hipStream_t s)
{
    constexpr int NW = WaferRitzCfg<R>::NW;
    hipLaunchKernelGGL((wafer_k_batch_moment_sums<R, NW, T, GS>), dim3((unsigned)max_nb, (unsigned)max_k, (unsigned)nact), dim3(NW * 64), 0, s, gs,
                       mem, act, swz, st, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wafer_k_batch_moment_reduce, dim3((unsigned)wafer_moment_rows(WAFER_RITZ_MAX), (unsigned)nact), dim3(256), 0, s,
                       (const double *)partials, act, mem, sums);
    return hipGetLastError();
}

template <typename GS>
hipError_t sums_by_type_and_reach(bool f32, int R, const GS &gs, const WaferBatchMember *mem, const WaferBatchMomentRec *act, int nact, int max_nb,
                                  int max_k, int swz, const WaferRitzPtrs &st, double *partials, double *sums, hipStream_t s)
{
    if (nact < 1 || nact > 65535 || max_k < 1 || max_k > WAFER_RITZ_MAX || max_nb < 1) return hipErrorInvalidValue;
    if (f32) {
        if (R == 1) return launch_sums<1, float, GS>(gs, mem, act, nact, max_nb, max_k, swz, st, partials, sums, s);
        if (R == 2) return launch_sums<2, float, GS>(gs, mem, act, nact, max_nb, max_k, swz, st, partials, sums, s);
        if (R == 3) return launch_sums<3, float, GS>(gs, mem, act, nact, max_nb, max_k, swz, st, partials, sums, s);
        return hipErrorInvalidValue;
    }
    if (R == 1) return launch_sums<1, double, GS>(gs, mem, act, nact, max_nb, max_k, swz, st, partials, sums, s);
    if (R == 2) return launch_sums<2, double, GS>(gs, mem, act, nact, max_nb, max_k, swz, st, partials, sums, s);
    if (R == 3) return launch_sums<3, double, GS>(gs, mem, act, nact, max_nb, max_k, swz, st, partials, sums, s);
    return hipErrorInvalidValue;
}

} // namespace

hipError_t wafer_entry_batch_moment_sums(bool f32, int R, const WaferGeom &gs, const WaferBatchMember *mem, const WaferBatchMomentRec *act, int nact,
                                         int max_nb, int max_k, int swz, const WaferRitzPtrs &st, double *partials, double *sums, hipStream_t s)
{
    return sums_by_type_and_reach(f32, R, gs, mem, act, nact, max_nb, max_k, swz, st, partials, sums, s);
}

hipError_t wafer_entry_batch_moment_sums(bool f32, int R, const WaferBatchGeomTable &gs, const WaferBatchMember *mem, const WaferBatchMomentRec *act,
                                         int nact, int max_nb, int max_k, int swz, const WaferRitzPtrs &st, double *partials, double *sums,
                                         hipStream_t s)
{
    return sums_by_type_and_reach(f32, R, gs, mem, act, nact, max_nb, max_k, swz, st, partials, sums, s);
}
