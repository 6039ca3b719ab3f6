// row_distance.h -- the squared distance of two embedding rows as PairwiseDistance computes it, shared by every
// kernel whose reported distances must carry PairwiseDistance's bits (tail_loss.hip, identify.hip, score_norm.hip).
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

// Four pairs (a, b0) .. (a, b3) at once, each with row_sqdist's arithmetic bit for bit, for kernels that walk many
// rows against one: the 4 x 8 loads of a 512-dimension step are in flight together (one pair at a time, every step
// waits a trip to L2), and the four butterflies share their exchanges.  Per pair the sum is the same tree: at the
// 32- and 16-lane steps a lane keeps the pair its half / quarter ends up owning and hands the other over (lane l still
// adds its own value and lane l ^ m's), the steps below run inside 16-lane groups.  Dimensions past D contribute
// fma(0, 0, s) = s.  Returns pair 0 on lanes 0..15, pair 2 on 16..31, pair 1 on 32..47, pair 3 on 48..63.
__device__ __forceinline__ float row_sqdist_x4(const float *a, const float *b0, const float *b1, const float *b2,
                                               const float *b3, int D, int lane) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int k0 = 0; k0 < D; k0 += 512) {
        float av[8], v0[8], v1[8], v2[8], v3[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = k0 + 64 * u + lane;
            const bool in = k < D;
            av[u] = in ? a[k] : 0.f;
            v0[u] = in ? b0[k] : 0.f;
            v1[u] = in ? b1[k] : 0.f;
            v2[u] = in ? b2[k] : 0.f;
            v3[u] = in ? b3[k] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float d0 = fabsf(av[u] - v0[u]), d1 = fabsf(av[u] - v1[u]);
            const float d2 = fabsf(av[u] - v2[u]), d3 = fabsf(av[u] - v3[u]);
            s0 += d0 * d0;
            s1 += d1 * d1;
            s2 += d2 * d2;
            s3 += d3 * d3;
        }
    }
    const bool h32 = (lane & 32) != 0, h16 = (lane & 16) != 0;
    const float x = (h32 ? s1 : s0) + ds_shfl_xor(h32 ? s0 : s1, 32);
    const float y = (h32 ? s3 : s2) + ds_shfl_xor(h32 ? s2 : s3, 32);
    float z = (h16 ? y : x) + ds_shfl_xor(h16 ? x : y, 16);
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) z += ds_shfl_xor(z, m);
    return z;
}

}  // namespace
