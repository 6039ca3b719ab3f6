// bn_pack.hip -- forward BatchNorm bookkeeping kernels and one-off layout/weight packing.
//   * eval-mode fold and train-mode statistics finalisation of nn.BatchNorm2d, for one member or G, from partial rows
//     or from float64 sums (reference model.py:59,62,94,99,103,107; semantics SURVEY 8(a) a2): every forward
//     statistics kernel of the library, the fp16 step's included
//   * elementwise normalise (+residual, +clipped ReLU) for the train-mode path
//   * OIHW -> packed filter layouts, NCHW <-> channels-last conversion
// (BatchNorm's backward, the float64 folds, the scheduler pool and the ABI version are in files of their own.)
#include <ds_device.h>
#include "ds_common.h"
#include "bn_fold.h"

namespace {

__global__ void __launch_bounds__(256) bn_fold_kernel(const float *gamma, const float *beta, const float *mean,
                                                      const float *var, float eps, float *scale, float *shift,
                                                      int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) {
        const float inv = 1.0f / sqrtf(var[c] + eps);
        const float s = gamma[c] * inv;
        scale[c] = s;
        shift[c] = beta[c] - mean[c] * s;
    }
}

__device__ __forceinline__ float *at_or_null(float *p, size_t i) { return p ? p + i : nullptr; }

// Train-mode statistics of G members of one BatchNorm layer in one launch (one member: G = 1), from partial rows or
// from float64 sums: batch mean / invstd / (scale, shift) per member into [G][C] tables (mean_t / invstd_t may be
// null), and the running statistics updated member after member IN CALL ORDER (the reference's model(data_a),
// model(data_p), model(data_n) are three nn.BatchNorm2d.train() calls: three momentum updates, model.py:188).
__global__ void __launch_bounds__(256) bn_stats_finalize_group_kernel(const float *partial, int n_partial, double count,
                                                                      const float *gamma, const float *beta, float eps,
                                                                      float momentum, float *running_mean,
                                                                      float *running_var, float *mean_t, float *invstd_t,
                                                                      float *scale_t, float *shift_t, int C, int G) {
    double *red = (double *)ds_dynamic_lds();              // [4 waves][FOLD_C][2] (128 of the bytes the launch asks for)
    for (int m = 0; m < G; ++m) {
        if (m) __syncthreads();                             // (the previous member's fold has been read)
        int c;
        double t1, t2;
        if (fold_partials(partial + (size_t)m * n_partial * C * 2, n_partial, C, red, c, t1, t2)) {
            const size_t o = (size_t)m * C + c;
            bn_stats_of_channel(t1, t2, count, gamma[c], beta[c], eps, momentum, at_or_null(running_mean, c),
                                at_or_null(running_var, c), at_or_null(mean_t, o), at_or_null(invstd_t, o), scale_t + o,
                                shift_t + o);
        }
    }
}

// ... from sums [G][2C+1] float64 (per member C pairs { sum z, sum z^2 } and the pixel count, which travels with the
// all-reduce of data-parallel training); count > 0 overrides the count slot, which is then not read (G = 1: the
// sums may be [C][2] alone)
__global__ void __launch_bounds__(256) bn_stats_from_sums_group_kernel(const double *sums, double count,
                                                                       const float *gamma, const float *beta, float eps,
                                                                       float momentum, float *running_mean,
                                                                       float *running_var, float *mean_t, float *invstd_t,
                                                                       float *scale_t, float *shift_t, int C, int G) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    for (int m = 0; m < G; ++m) {
        const double *sm = sums + (size_t)m * (2 * C + 1);
        const size_t o = (size_t)m * C + c;
        bn_stats_of_channel(sm[c * 2], sm[c * 2 + 1], count > 0.0 ? count : sm[2 * C], gamma[c], beta[c], eps, momentum,
                            at_or_null(running_mean, c), at_or_null(running_var, c), at_or_null(mean_t, o),
                            at_or_null(invstd_t, o), scale_t + o, shift_t + o);
    }
}

__global__ void __launch_bounds__(256) bn_apply_kernel(const float *x, const float *scale, const float *shift,
                                                       const float *res, float *y, long long n_vec, int C,
                                                       int flags) {
    const int cvec = C >> 2;
    // 256 threads, grid stride a multiple of 256: when C / 4 is a power of two dividing 256 (every layer of the network) a
    // thread keeps ONE channel group for the whole pass -- table rows loaded once, no 64-bit modulo per vector (round 4:
    // the per-vector `i % cvec` in 64-bit arithmetic was a third of the pass's instructions)
    const bool fixed = (256 % cvec) == 0 && (cvec & (cvec - 1)) == 0;
    const int c4f = threadIdx.x & (cvec - 1);
    f32x4 sc = {0.f, 0.f, 0.f, 0.f}, sh = sc;
    if (fixed) {
        sc = ((const f32x4 *)scale)[c4f];
        sh = ((const f32x4 *)shift)[c4f];
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_vec; i += (long long)gridDim.x * 256) {
        if (!fixed) {
            const int c4 = (int)(i % cvec);
            sc = ((const f32x4 *)scale)[c4];
            sh = ((const f32x4 *)shift)[c4];
        }
        f32x4 v = ((const f32x4 *)x)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ds_bn_affine(v[j], sc[j], sh[j]);
        if (flags & DS_EPI_RESIDUAL) v += ((const f32x4 *)res)[i];
        if (flags & DS_EPI_CLIP) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = fminf(fmaxf(v[j], 0.0f), 20.0f);
        }
        ((f32x4 *)y)[i] = v;
    }
}

// OIHW -> [Cin/8][KS*KS][Cout][8]; dgrad: roles of Cout/Cin swapped, taps flipped
__global__ void __launch_bounds__(256) pack_conv_weight_kernel(const float *w, float *out, int Cout, int Cin, int KS,
                                                               int dgrad) {
    const int T = KS * KS;
    const long long n = (long long)Cout * Cin * T;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        // i indexes the packed tensor [K/8][T][N][8] where (N,K) = (Cout,Cin) or (Cin,Cout) for dgrad
        const int N = dgrad ? Cin : Cout, K = dgrad ? Cout : Cin;
        const int kk = (int)(i & 7);
        long long r = i >> 3;
        const int nn = (int)(r % N);
        r /= N;
        const int t = (int)(r % T);
        const int kc = (int)(r / T);
        const int k = kc * 8 + kk;
        const int tt = dgrad ? (T - 1 - t) : t;
        const int kh = tt / KS, kw = tt - kh * KS;
        const int co = dgrad ? k : nn, ci = dgrad ? nn : k;
        (void)K;
        out[i] = w[(((size_t)co * Cin + ci) * KS + kh) * KS + kw];
    }
}

// 5x5 stride-2 data-gradient packing: four parity classes (ph,pw) in order (0,0),(0,1),(1,0),(1,1),
// class taps = {kh = ph mod 2} x {kw = pw mod 2} in ascending kernel index; each class block is
// [Cout/8][taps][Cin][8] (K = Cout, N = Cin) -- see ds_conv_dgrad_f32.
__global__ void __launch_bounds__(256) pack_conv_dgrad_s2_kernel(const float *w, float *out, int Cout, int Cin) {
    const long long n = (long long)Cout * Cin * 25;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        long long r = i;
        int ph = 0, pw = 0, nh = 3, nw = 3;
        for (int c = 0; c < 4; ++c) {
            ph = c >> 1; pw = c & 1;
            nh = ph ? 2 : 3; nw = pw ? 2 : 3;
            const long long sz = (long long)nh * nw * Cout * Cin;
            if (r < sz) break;
            r -= sz;
        }
        const int kk = (int)(r & 7);
        r >>= 3;
        const int ci = (int)(r % Cin);
        r /= Cin;
        const int t = (int)(r % (nh * nw));
        const int kc = (int)(r / (nh * nw));
        const int co = kc * 8 + kk;
        const int kh = ph + 2 * (t / nw), kw = pw + 2 * (t % nw);
        out[i] = w[(((size_t)co * Cin + ci) * 5 + kh) * 5 + kw];
    }
}

__global__ void __launch_bounds__(256) pack_conv1_weight_kernel(const float *w, float *out, int Cout) {
    const int i = blockIdx.x * 256 + threadIdx.x;          // out[t][co] = w[co][0][t]
    if (i < 25 * Cout) {
        const int t = i / Cout, co = i - t * Cout;
        out[i] = w[co * 25 + t];
    }
}

// fc weight [N][C*F] (c*F+f) -> [K'/8][1][N][8] with k' = f*C + c
__global__ void __launch_bounds__(256) pack_fc_weight_kernel(const float *w, float *out, int N, int C, int F) {
    const long long n = (long long)N * C * F;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int kk = (int)(i & 7);
        long long r = i >> 3;
        const int nn = (int)(r % N);
        const int kc = (int)(r / N);
        const int kp = kc * 8 + kk;
        const int f = kp / C, c = kp - f * C;
        out[i] = w[(size_t)nn * C * F + (size_t)c * F + f];
    }
}

// fc data-gradient packing: gpooled[b][k'] = sum_n gf[b][n] * W[n][c*F+f]  ->  [N/8][1][K'][8]
__global__ void __launch_bounds__(256) pack_fc_weight_dgrad_kernel(const float *w, float *out, int N, int C, int F) {
    const long long n = (long long)N * C * F;
    const int K = C * F;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int kk = (int)(i & 7);
        long long r = i >> 3;
        const int kp = (int)(r % K);
        const int nc = (int)(r / K);
        const int nn = nc * 8 + kk;
        const int f = kp / C, c = kp - f * C;
        out[i] = w[(size_t)nn * K + (size_t)c * F + f];
    }
}

__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const float *x, float *y, int B, int C, int HW,
                                                           int to_nhwc) {
    const long long n = (long long)B * C * HW;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        // i indexes the DESTINATION so writes are coalesced
        if (to_nhwc) {
            const int c = (int)(i % C);
            const long long r = i / C;
            const int s = (int)(r % HW);
            const int b = (int)(r / HW);
            y[i] = x[((size_t)b * C + c) * HW + s];
        } else {
            const int s = (int)(i % HW);
            const long long r = i / HW;
            const int c = (int)(r % C);
            const int b = (int)(r / C);
            y[i] = x[((size_t)b * HW + s) * C + c];
        }
    }
}

// the one launch of the sums form (no argument checks: the two entry points keep their own)
int stats_from_sums(const double *sums, double count, const float *gamma, const float *beta, float eps, float momentum,
                    float *running_mean, float *running_var, float *mean_t, float *invstd_t, float *scale_t,
                    float *shift_t, int C, int G, void *stream) {
    DS_LAUNCH(bn_stats_from_sums_group_kernel, ds_ceil_div(C, 256), 256, 0, stream, sums, count, gamma, beta, eps, momentum,
              running_mean, running_var, mean_t, invstd_t, scale_t, shift_t, C, G);
    return ds_last_launch_error();
}

}  // namespace

// ... and of the rows form (bn_fold.h).  The fold uses 4 waves x FOLD_C x 2 doubles of the LDS it asks for; the
// request is what these launches have always made.
int ds_bn_launch_stats_finalize(const float *partial, int n_partial, double count, const float *gamma, const float *beta,
                                float eps, float momentum, float *running_mean, float *running_var, float *mean_t,
                                float *invstd_t, float *scale_t, float *shift_t, int C, int G, void *stream) {
    DS_LAUNCH(bn_stats_finalize_group_kernel, ds_ceil_div(C, FOLD_C), 256, FOLD_R * FOLD_C * 2 * sizeof(double), stream,
              partial, n_partial, count, gamma, beta, eps, momentum, running_mean, running_var, mean_t, invstd_t, scale_t,
              shift_t, C, G);
    return ds_last_launch_error();
}

extern "C" int ds_bn_fold_f32(const float *gamma, const float *beta, const float *running_mean,
                              const float *running_var, float eps, float *scale, float *shift, int C, void *stream) {
    DS_REQUIRE(gamma && beta && running_mean && running_var && scale && shift, DS_ERR_NULL);
    DS_REQUIRE(C > 0, DS_ERR_BAD_SHAPE);
    DS_LAUNCH(bn_fold_kernel, ds_ceil_div(C, 256), 256, 0, stream, gamma, beta, running_mean, running_var, eps, scale,
              shift, C);
    return ds_last_launch_error();
}

extern "C" int ds_bn_stats_finalize_f32(const float *partial, int n_partial, long long count, const float *gamma,
                                        const float *beta, float eps, float momentum, float *running_mean,
                                        float *running_var, float *batch_mean, float *batch_invstd, float *scale,
                                        float *shift, int C, void *stream) {
    DS_REQUIRE(partial && gamma && beta && scale && shift, DS_ERR_NULL);
    DS_REQUIRE((running_mean == nullptr) == (running_var == nullptr), DS_ERR_NULL);
    DS_REQUIRE(C > 0 && n_partial > 0 && count > 0, DS_ERR_BAD_SHAPE);
    return ds_bn_launch_stats_finalize(partial, n_partial, (double)count, gamma, beta, eps, momentum, running_mean,
                                       running_var, batch_mean, batch_invstd, scale, shift, C, 1, stream);
}

// ---- forward statistics of data-parallel training: local sums -> (all-reduce by the caller) -> finalize ----
// one member from sums [C][2] and its count, or (count == 0) from sums [2C+1] with the count in the last slot
extern "C" int ds_bn_stats_from_sums_f32(const double *sums, long long count, const float *gamma, const float *beta,
                                         float eps, float momentum, float *running_mean, float *running_var,
                                         float *batch_mean, float *batch_invstd, float *scale, float *shift, int C,
                                         void *stream) {
    DS_REQUIRE(sums && gamma && beta && scale && shift, DS_ERR_NULL);
    DS_REQUIRE((running_mean == nullptr) == (running_var == nullptr), DS_ERR_NULL);
    DS_REQUIRE(C > 0 && count >= 0, DS_ERR_BAD_SHAPE);
    return stats_from_sums(sums, (double)count, gamma, beta, eps, momentum, running_mean, running_var, batch_mean,
                           batch_invstd, scale, shift, C, 1, stream);
}

// [G][C] tables (and the running statistics, members in call order) from the all-reduced sums [G][2C+1] of G members:
// the second half of ds_bn_stats_partial_f16 + ds_partial_sum_f64_group
extern "C" int ds_bn_stats_from_sums_group_f32(const double *sums, const float *gamma, const float *beta, float eps,
                                               float momentum, float *running_mean, float *running_var, float *mean_t,
                                               float *invstd_t, float *scale_t, float *shift_t, int C, int G, void *stream) {
    DS_REQUIRE(sums && gamma && beta && mean_t && invstd_t && scale_t && shift_t, DS_ERR_NULL);
    DS_REQUIRE(C > 0 && G > 0 && G <= 64, DS_ERR_BAD_SHAPE);
    DS_REQUIRE((running_mean == nullptr) == (running_var == nullptr), DS_ERR_NULL);
    return stats_from_sums(sums, 0.0, gamma, beta, eps, momentum, running_mean, running_var, mean_t, invstd_t, scale_t,
                           shift_t, C, G, stream);
}

extern "C" int ds_bn_apply_f32(const float *x, const float *scale, const float *shift, const float *residual,
                               float *y, long long n_pix, int C, int flags, void *stream) {
    DS_REQUIRE(x && scale && shift && y, DS_ERR_NULL);
    DS_REQUIRE(!(flags & DS_EPI_RESIDUAL) || residual, DS_ERR_NULL);
    DS_REQUIRE(n_pix > 0 && C > 0 && (C % 4) == 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(DS_ALIGNED16(x) && DS_ALIGNED16(y) && DS_ALIGNED16(scale) && DS_ALIGNED16(shift), DS_ERR_ALIGNMENT);
    const long long n_vec = n_pix * (C / 4);
    int grid = grid_for(n_vec);
    DS_LAUNCH(bn_apply_kernel, grid, 256, 0, stream, x, scale, shift, residual, y, n_vec, C, flags);
    return ds_last_launch_error();
}

extern "C" int ds_pack_conv_weight_f32(const float *w_oihw, float *w_packed, int Cout, int Cin, int KS, int dgrad,
                                       void *stream) {
    DS_REQUIRE(w_oihw && w_packed, DS_ERR_NULL);
    DS_REQUIRE(Cout > 0 && Cin > 0 && (KS == 1 || KS == 3 || KS == 5), DS_ERR_BAD_SHAPE);
    DS_REQUIRE(((dgrad ? Cout : Cin) % 8) == 0, DS_ERR_BAD_SHAPE);
    const long long n = (long long)Cout * Cin * KS * KS;
    DS_LAUNCH(pack_conv_weight_kernel, grid_for(n), 256, 0, stream, w_oihw, w_packed, Cout, Cin, KS, dgrad);
    return ds_last_launch_error();
}

extern "C" int ds_pack_conv_dgrad_s2_f32(const float *w_oihw, float *w_packed, int Cout, int Cin, void *stream) {
    DS_REQUIRE(w_oihw && w_packed, DS_ERR_NULL);
    DS_REQUIRE(Cout > 0 && Cin > 0 && (Cout % 8) == 0, DS_ERR_BAD_SHAPE);
    DS_LAUNCH(pack_conv_dgrad_s2_kernel, grid_for((long long)Cout * Cin * 25), 256, 0, stream, w_oihw, w_packed, Cout,
              Cin);
    return ds_last_launch_error();
}

extern "C" int ds_pack_conv1_weight_f32(const float *w_oihw, float *w_packed, int Cout, void *stream) {
    DS_REQUIRE(w_oihw && w_packed, DS_ERR_NULL);
    DS_REQUIRE(Cout > 0, DS_ERR_BAD_SHAPE);
    DS_LAUNCH(pack_conv1_weight_kernel, ds_ceil_div(25 * Cout, 256), 256, 0, stream, w_oihw, w_packed, Cout);
    return ds_last_launch_error();
}

extern "C" int ds_pack_fc_weight_f32(const float *w, float *w_packed, int N, int C, int F, void *stream) {
    DS_REQUIRE(w && w_packed, DS_ERR_NULL);
    DS_REQUIRE(N > 0 && C > 0 && F > 0 && ((C * F) % 8) == 0, DS_ERR_BAD_SHAPE);
    DS_LAUNCH(pack_fc_weight_kernel, grid_for((long long)N * C * F), 256, 0, stream, w, w_packed, N, C, F);
    return ds_last_launch_error();
}

extern "C" int ds_pack_fc_weight_dgrad_f32(const float *w, float *w_packed, int N, int C, int F, void *stream) {
    DS_REQUIRE(w && w_packed, DS_ERR_NULL);
    DS_REQUIRE(N > 0 && C > 0 && F > 0 && (N % 8) == 0, DS_ERR_BAD_SHAPE);
    DS_LAUNCH(pack_fc_weight_dgrad_kernel, grid_for((long long)N * C * F), 256, 0, stream, w, w_packed, N, C, F);
    return ds_last_launch_error();
}

extern "C" int ds_nchw_to_nhwc_f32(const float *x, float *y, int B, int C, int H, int W, void *stream) {
    DS_REQUIRE(x && y, DS_ERR_NULL);
    DS_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, DS_ERR_BAD_SHAPE);
    DS_LAUNCH(nchw_to_nhwc_kernel, grid_for((long long)B * C * H * W), 256, 0, stream, x, y, B, C, H * W, 1);
    return ds_last_launch_error();
}

extern "C" int ds_nhwc_to_nchw_f32(const float *x, float *y, int B, int C, int H, int W, void *stream) {
    DS_REQUIRE(x && y, DS_ERR_NULL);
    DS_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, DS_ERR_BAD_SHAPE);
    DS_LAUNCH(nchw_to_nhwc_kernel, grid_for((long long)B * C * H * W), 256, 0, stream, x, y, B, C, H * W, 0);
    return ds_last_launch_error();
}
