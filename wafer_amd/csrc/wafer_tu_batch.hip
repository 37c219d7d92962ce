// translation unit: the batched ensemble kernels for a batch of ONE shape -- the geometry is a kernel argument (wafer_tu_batch.inc)
#define WAFER_TU_BATCH_GS WaferGeom
#include "wafer_tu_batch.inc"

// the instantiations of the fused pass, the same list for every dtype: ThreePoint 3 steps (and 2, for the remainder of a call),
// FivePoint 2 steps.  f64 and f32 keep double queues and LDS, f32fast float ones (half the bytes).
int wafer_batch_stepk_lds_bytes(int dtype, int R, int K)
{
    if (dtype < 0 || dtype > 2) return 0;
    const bool wide = dtype != 2;
    if (R == 1 && K == 3) return wide ? WaferBatchKCfg<1, 3, 8>::LDS_BYTES : WaferBatchKCfg<1, 3, 4>::LDS_BYTES;
    if (R == 1 && K == 2) return wide ? WaferBatchKCfg<1, 2, 8>::LDS_BYTES : WaferBatchKCfg<1, 2, 4>::LDS_BYTES;
    if (R == 2 && K == 2) return wide ? WaferBatchKCfg<2, 2, 8>::LDS_BYTES : WaferBatchKCfg<2, 2, 4>::LDS_BYTES;
    return 0;
}
