// row_distance.h -- the squared distance of two embedding rows as PairwiseDistance computes it, shared by every
// kernel whose reported distances must carry PairwiseDistance's bits (tail_loss.hip, identify.hip).
// One 64-lane wavefront owns the pair: lane l sums dimensions l, l + 64, ... in order, then a butterfly over the lanes.
#pragma once
#include <ds_device.h>

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += ds_shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ float row_sqdist(const float *a, const float *b, int D, int lane) {
    float s = 0.f;
    for (int k = lane; k < D; k += 64) {
        const float d = fabsf(a[k] - b[k]);
        s += d * d;
    }
    return wave_sum(s);
}

}  // namespace
