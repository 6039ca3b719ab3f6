// bn_fold.h -- what the two BatchNorm translation units (bn_pack.hip: forward, bn_bwd.hip: backward and the float64
// split forms) share: the double-precision fold of partial rows and the grid of the element-wise passes.
#pragma once
#include <ds_device.h>

// Fold of [n_partial][C][2] partial sums in double precision, fixed order: one workgroup per FOLD_C channels,
// FOLD_R row-lanes stride over the partial rows (stage-1 layers have thousands of rows and only 64 channels --
// a channel-per-thread layout left the chip idle; 8 channels x 32 lanes still meant 8 workgroups walking 64 rows
// each: 27 us, now 8), then lane 0 folds the lane sums.
// Round 6: the lane sums are folded by an xor tree of shuffles inside each wave (lane = 2 * row lane + channel: offsets
// 2 .. 32) and the four waves' results by one thread -- the last step used to be ONE thread adding 128 LDS values per
// channel in sequence (14 - 18 us per launch, 48 launches per training step).
constexpr int FOLD_C = 2, FOLD_R = 128;
__device__ __forceinline__ bool fold_partials(const float *partial, int n_partial, int C, double *red, int &c,
                                              double &t1, double &t2, int cgroup = -1) {
    const int cl = threadIdx.x % FOLD_C, rl = threadIdx.x / FOLD_C;
    c = (cgroup < 0 ? (int)blockIdx.x : cgroup) * FOLD_C + cl;
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        for (int r = rl; r < n_partial; r += FOLD_R) {
            const float *src = partial + ((size_t)r * C + c) * 2;
            s1 += (double)src[0];
            s2 += (double)src[1];
        }
    }
#pragma unroll
    for (int m = 2; m <= 32; m <<= 1) {
        s1 += ds_shfl_xor_f64(s1, m);
        s2 += ds_shfl_xor_f64(s2, m);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane < FOLD_C) {
        red[(wave * FOLD_C + cl) * 2 + 0] = s1;
        red[(wave * FOLD_C + cl) * 2 + 1] = s2;
    }
    __syncthreads();
    if (rl != 0 || c >= C) return false;
    t1 = 0.0;
    t2 = 0.0;
    for (int k = 0; k < 4; ++k) {
        t1 += red[(k * FOLD_C + cl) * 2 + 0];
        t2 += red[(k * FOLD_C + cl) * 2 + 1];
    }
    return true;
}

// workgroups of a grid-stride element-wise pass over n elements (256 threads each)
static inline int grid_for(long long n) {
    long long g = (n + 255) / 256;
    return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}
