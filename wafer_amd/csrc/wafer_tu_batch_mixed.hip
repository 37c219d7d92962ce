// translation unit: the batched ensemble kernels for a batch of SEVERAL shapes -- the same templates instantiated with the geometry
// taken from the batch's device table, indexed by the workgroup's shape (wafer_tu_batch.inc)
#define WAFER_TU_BATCH_GS WaferBatchGeomTable
#include "wafer_tu_batch.inc"
