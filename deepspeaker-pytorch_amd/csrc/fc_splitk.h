// fc_splitk.h -- the f32-MFMA split-K GEMM behind the projection, the softmax head and the margin head
// (fc_mfma_f32.hip, margin_head.hip): the partial-tile kernel, its split rule, the fixed-order wave sum and the mean of the
// per-row losses.  Include inside the translation unit's unnamed namespace.
#pragma once

constexpr int CK = DS_CONV_CK;

__device__ __forceinline__ float fc_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += ds_shfl_xor(v, m);
    return v;
}

// grid = m_tiles * n_tiles * S;  block = 256 (4 waves, one 32x32 output tile each)
__global__ void __launch_bounds__(256) fc_splitk_kernel(const float *x, const float *w, float *partial, int B, int K,
                                                        int N, int S, int n_tiles) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, lhi = lane >> 5;
    int bid = blockIdx.x;
    const int sp = bid % S;
    bid /= S;
    const int nt = bid % n_tiles, mt = bid / n_tiles;
    const int m0 = mt * 32, n0 = nt * 128 + wave * 32;
    const int chunks = K / CK, per = chunks / S;
    const int c0 = sp * per;
    const int row = (m0 + l31 < B) ? m0 + l31 : B - 1;
    const float *xa = x + (size_t)row * K + 4 * lhi;
    const float *wb = w + ((size_t)n0 + l31) * CK + 4 * lhi;
    const size_t wstride = (size_t)N * CK;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int c = c0; c < c0 + per; c += 4) {          // per is a multiple of 4
        f32x4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = *(const f32x4 *)(xa + (size_t)(c + u) * CK);
            b[u] = *(const f32x4 *)(wb + (size_t)(c + u) * wstride);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = ds_mfma_32x32x2_f32(a[u][j], b[u][j], acc);
    }
    float *dst = partial + (size_t)sp * B * N;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        if (m < B) dst[(size_t)m * N + n0 + l31] = acc[r];
    }
}

__global__ void __launch_bounds__(256) fc_mean_kernel(const float *x, float *out, int n) {
    float *scratch = ds_dynamic_lds();
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) acc += x[i];
    acc = fc_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (scratch[0] + scratch[1] + scratch[2] + scratch[3]) / (float)n;
}

static int fc_splits(int K) {
    const int chunks = K / CK;
    for (int s = 8; s > 1; s >>= 1)
        if (chunks % (4 * s) == 0) return s;
    return 1;
}
