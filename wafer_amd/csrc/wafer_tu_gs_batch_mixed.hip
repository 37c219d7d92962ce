// translation unit: the batched excited-state kernels (wafer_gs_batch.hip.h) reading each member's geometry from the device table
// -- a batch of several shapes with state stores (wafer_batch_create_mixed_states)
#define WAFER_TU_BATCH_GS WaferBatchGeomTable
#include "wafer_tu_gs_batch.inc"
