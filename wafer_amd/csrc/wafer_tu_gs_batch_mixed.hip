// translation unit: the batched excited-state kernels (wafer_gs_batch.hip.h) reading each member's geometry and partition from
// the device tables -- a batch of several shapes with state stores (wafer_batch_create_mixed_states)
#define WAFER_TU_GS_MIXED 1
#include "wafer_tu_gs_batch.inc"
