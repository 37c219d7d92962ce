// translation unit: the store filter of a batch of ONE shape (the geometry is a kernel argument: wafer_tu_store_filter_batch.inc)
#define WAFER_TU_BATCH_GS WaferGeom
#include "wafer_tu_store_filter_batch.inc"
