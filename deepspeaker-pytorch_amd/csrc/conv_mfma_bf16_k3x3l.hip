// conv_mfma_bf16_k3x3l.hip -- instantiations of conv_mfma_bf16_kernel for 3x3 taps, split-operand bf16x3
// arithmetic, the latency rows kCfgBLat (one translation unit per combination so that they compile in parallel).
#define DS_BF16_KERNEL_TU
#include "conv_mfma_bf16_kernel.h"

void ds_bf16_launch_k3x3l(const PlanB &pl, void *stream) { launch_lat_b<3>(pl, stream); }
