// translation unit: the store filter of a batch of SEVERAL shapes with state stores -- the same template instantiated with the
// geometry taken from the batch's device table, indexed by the workgroup's shape (wafer_tu_store_filter_batch.inc)
#define WAFER_TU_BATCH_GS WaferBatchGeomTable
#include "wafer_tu_store_filter_batch.inc"
