// bn_fold.h -- what the BatchNorm translation units share (bn_pack.hip: forward statistics and normalise, bn_bwd.hip:
// the f32-class backward and the float64 split forms, train_f16.hip: the fp16 family): the block-level tail of the
// reductions, the double-precision fold of partial rows, the statistics formula, the backward coefficient stores, the
// grid of the element-wise passes and the one host launcher that crosses objects.
#pragma once
#include <ds_device.h>

// Tail of a reduction workgroup (256 threads, V channels per thread, cvec = C / V channel groups x `slots` pixel slots):
// per-block partial sums of two per-channel quantities -> partial[blockIdx.x][c][2]; red: [slots][C][2] floats, folded
// in slot order.  V = 8: the fp16 reductions of train_f16.hip; V = 4: bn_bwd_reduce_kernel of bn_bwd.hip, which keeps
// this text written out (see there).
template <int V>
struct bn_fvec { typedef float type __attribute__((ext_vector_type(V))); };
template <int V>
__device__ __forceinline__ void block_fold(float *red, const typename bn_fvec<V>::type &s1,
                                           const typename bn_fvec<V>::type &s2, int slot, int slots, int cg, int C,
                                           float *partial) {
    if (slot < slots) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            red[((slot * C) + cg * V + j) * 2 + 0] = s1[j];
            red[((slot * C) + cg * V + j) * 2 + 1] = s2[j];
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float a1 = 0.f, a2 = 0.f;
        for (int s = 0; s < slots; ++s) {
            a1 += red[(s * C + c) * 2 + 0];
            a2 += red[(s * C + c) * 2 + 1];
        }
        partial[((size_t)blockIdx.x * C + c) * 2 + 0] = a1;
        partial[((size_t)blockIdx.x * C + c) * 2 + 1] = a2;
    }
}

// Fold of [n_partial][C][2] partial sums in double precision, fixed order: one workgroup per FOLD_C channels,
// FOLD_R row-lanes stride over the partial rows (stage-1 layers have thousands of rows and only 64 channels --
// a channel-per-thread layout left the chip idle; 8 channels x 32 lanes still meant 8 workgroups walking 64 rows
// each: 27 us, now 8), then lane 0 folds the lane sums.
// Round 6: the lane sums are folded by an xor tree of shuffles inside each wave (lane = 2 * row lane + channel: offsets
// 2 .. 32) and the four waves' results by one thread -- the last step used to be ONE thread adding 128 LDS values per
// channel in sequence (14 - 18 us per launch, 48 launches per training step; 16 - 35 us per member in the fp16 step).
// red: [4 waves][FOLD_C][2] doubles.  A kernel that folds member after member puts a __syncthreads() between two
// calls (the previous member's `red` has been read); the single-use kernels have the one barrier in here.
constexpr int FOLD_C = 2, FOLD_R = 128;
__device__ __forceinline__ bool fold_partials(const float *partial, int n_partial, int C, double *red, int &c,
                                              double &t1, double &t2, int cgroup = -1) {
    static_assert(FOLD_C == 2 && FOLD_R == 128, "lane = 2 * row lane + channel; four waves");
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

// Train-mode statistics of one channel from t1 = sum z, t2 = sum z^2 over `count` pixels, in double precision: mean,
// clamped biased variance, invstd, the momentum update of the running statistics with the unbiased variance, scale =
// gamma * invstd, shift = beta - mean * scale.  The rows form and the sums form of the finalisation must agree bit for
// bit (data-parallel ranks rely on it): this is the only text of the formula.  Pointers are the channel's own
// elements; running_mean / running_var (both or neither) and mean / invstd may be null.
__device__ __forceinline__ void bn_stats_of_channel(double t1, double t2, double count, float gamma_c, float beta_c,
                                                    float eps, float momentum, float *running_mean, float *running_var,
                                                    float *mean_out, float *invstd_out, float *scale, float *shift) {
    const double mean = t1 / count;
    double var = t2 / count - mean * mean;                 // biased (normalisation) variance
    if (var < 0.0) var = 0.0;
    const double invstd = 1.0 / sqrt(var + (double)eps);
    const double unbiased = count > 1.0 ? var * (count / (count - 1.0)) : var;
    if (running_mean) {
        *running_mean = (float)((1.0 - (double)momentum) * (double)*running_mean + (double)momentum * mean);
        *running_var = (float)((1.0 - (double)momentum) * (double)*running_var + (double)momentum * unbiased);
    }
    if (mean_out) *mean_out = (float)mean;
    if (invstd_out) *invstd_out = (float)invstd;
    const double s = (double)gamma_c * invstd;
    *scale = (float)s;
    *shift = (float)((double)beta_c - mean * s);
}

// The backward's coefficients of channel c of one member from t1 = sum gy, t2 = sum gy * xhat over `count` pixels:
// coef_m [3][C] = { gamma * invstd, t1 / count, t2 / count }
__device__ __forceinline__ void bn_bwd_store_coef(float *coef_m, int C, int c, float gamma_c, float invstd_c, double t1,
                                                  double t2, double count) {
    coef_m[c] = gamma_c * invstd_c;
    coef_m[C + c] = (float)(t1 / count);
    coef_m[2 * C + c] = (float)(t2 / count);
}

// workgroups of a grid-stride element-wise pass over n elements (256 threads each)
static inline int grid_for(long long n) {
    long long g = (n + 255) / 256;
    return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

// Forward statistics of G members from their partial rows (n_partial rows of [C][2] each, consecutive) in one launch,
// the running statistics updated member after member in call order; mean_t / invstd_t may be null.  No argument
// checks: the entry points keep their own.  Defined in bn_pack.hip (kernels are not shared across objects, host
// functions are); ds_bn_stats_group_f16 calls it after its fp16 partial pass.
int ds_bn_launch_stats_finalize(const float *partial, int n_partial, double count, const float *gamma, const float *beta,
                                float eps, float momentum, float *running_mean, float *running_var, float *mean_t,
                                float *invstd_t, float *scale_t, float *shift_t, int C, int G, void *stream);
