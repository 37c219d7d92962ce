// translation unit: the batched excited-state kernels (wafer_gs_batch.hip.h) of a batch of one shape
#define WAFER_TU_BATCH_GS WaferGeom
#include "wafer_tu_gs_batch.inc"
