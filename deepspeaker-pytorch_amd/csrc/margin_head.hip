// margin_head.hip -- the angular-margin softmax head of the pre-training regime (AAM-softmax / ArcFace and AM-softmax /
// CosFace) on the classifier's own weight: cosines of L2-normalised embeddings and class rows, a margin at the label
// column, scaled cross-entropy.
//
//   c[i,j] = clamp(x^_i . w^_j, -1, 1)        z[i,j] = s c[i,j],  z[i,y_i] = s phi(c[i,y_i])
//   am:   phi = c - m
//   aam:  phi = c cos m - sqrt(max(1 - c^2, DS_MARGIN_SIN2_FLOOR)) sin m   where c > -cos m, else c - m sin m
//   loss = mean_i (logsumexp_{j < n_cls} z[i,j] - z[i,y_i])
//
// The cosines are the split-K GEMM of fc_splitk.h on the normalised rows; as in the plain head (fc_reduce_ce_kernel) the
// reduction epilogue folds the K-slices, and here also clamps, stores c (the backward pass needs c, not z), applies the
// margin and takes row maximum, log-sum-exp and row loss in the same pass.  The backward pass writes
// gc = dL/dc (label column times dphi/dc), the row sums r_i = sum_j gc c and the column sums q_j = sum_i gc c; the two
// GEMMs gc W^ and gc^T x^ are the plain head's, and a row kernel projects their results onto the tangent spaces of the
// normalisations:  gx_i = inv_x[i] (A_i - r_i x^_i),  gW_j = inv_w[j] (Bm_j - q_j w^_j).
// Every sum has one fixed order that depends on the row (or column) alone: results are deterministic and a row's c,
// loss and gradient do not depend on the other rows of the batch.
#include <ds_device.h>
#include "ds_common.h"

namespace {

#include "fc_splitk.h"      // fc_splitk_kernel, fc_splits, fc_wave_sum, fc_mean_kernel

struct MarginRule {
    float s, m, cos_m, sin_m, m_sin_m;
    int kind;
};

__device__ __forceinline__ float margin_sn(float c) {
    return sqrtf(fmaxf((1.0f - c) * (1.0f + c), DS_MARGIN_SIN2_FLOOR));
}
__device__ __forceinline__ float margin_phi(const MarginRule &mr, float c) {
    if (mr.kind == DS_MARGIN_AM) return c - mr.m;
    if (c > -mr.cos_m) return c * mr.cos_m - margin_sn(c) * mr.sin_m;
    return c - mr.m_sin_m;
}
__device__ __forceinline__ float margin_dphi(const MarginRule &mr, float c) {
    if (mr.kind == DS_MARGIN_AM || !(c > -mr.cos_m)) return 1.0f;
    return mr.cos_m + c * mr.sin_m / margin_sn(c);
}

__device__ __forceinline__ float margin_wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, ds_shfl_xor(v, m));
    return v;
}

// one wave per row: out = x / ||x|| (0 for an all-zero row), inv = 1 / ||x|| (0); rows R .. R_out-1 of out and inv are zero
// (the class rows padded to the GEMM's 128-column tile)
__global__ void __launch_bounds__(256) row_normalize_kernel(const float *x, float *out, float *inv, int R, int R_out,
                                                            int K) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R_out) return;
    const int kv = K >> 2;
    f32x4 *o = (f32x4 *)(out + (size_t)row * K);
    if (row >= R) {
        const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
        for (int v = lane; v < kv; v += 64) o[v] = z4;
        if (lane == 0) inv[row] = 0.f;
        return;
    }
    const f32x4 *src = (const f32x4 *)(x + (size_t)row * K);
    float ss = 0.f;
    for (int v = lane; v < kv; v += 64) {
        const f32x4 t = src[v];
#pragma unroll
        for (int j = 0; j < 4; ++j) ss = __builtin_fmaf(t[j], t[j], ss);
    }
    ss = fc_wave_sum(ss);
    const float nrm = sqrtf(ss);
    const float iv = nrm > 0.f ? 1.0f / nrm : 0.f;
    for (int v = lane; v < kv; v += 64) o[v] = src[v] * iv;
    if (lane == 0) inv[row] = iv;
}

// The GEMM's reduction epilogue, one wave per row, a lane on 4 adjacent columns per step: folds the K-slices in the order
// s = 0 .. S-1, clamps and stores c [B, N].  CE: margin at the label column, row maximum and log-sum-exp over the n_cls
// real columns (a pad column holds c = 0, which would win the maximum of a row of negative cosines: it never enters),
// row loss.  !CE: cos_out [B, n_cls] = s c, nothing else.
template <bool CE>
__global__ void __launch_bounds__(256) margin_reduce_kernel(const float *partial, float *c, const long long *labels,
                                                            float *row_loss, float *lse, float *cos_out, int B, int N,
                                                            int n_cls, int S, MarginRule mr) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int r = row < B ? row : B - 1;
    const long long y = CE ? labels[r] : -1;
    float mx = -3.0e38f, zy = 0.f;
    for (int k = 4 * lane; k < N; k += 256) {
        f32x4 pv[8];                            // S <= 8 (fc_splits)
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
            pv[s] = s < S ? *(const f32x4 *)(partial + ((size_t)s * B + r) * N + k) : z4;
        }
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 8; ++s) v += pv[s];             // fixed order: s = 0 .. S-1 (+ zeros)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fminf(fmaxf(v[j], -1.0f), 1.0f);
        if (row < B) *(f32x4 *)(c + (size_t)r * N + k) = v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int kk = k + j;
            if (CE) {
                const float z = mr.s * (kk == y ? margin_phi(mr, v[j]) : v[j]);
                if (kk == y) zy = z;
                if (kk < n_cls) mx = fmaxf(mx, z);
            } else if (row < B && kk < n_cls) {
                cos_out[(size_t)r * n_cls + kk] = mr.s * v[j];
            }
        }
    }
    if (!CE) return;
    mx = margin_wave_max(mx);
    float se = 0.f;
    if (row < B)                                            // a lane re-reads only the columns it wrote itself
        for (int k = 4 * lane; k < N; k += 256) {
            const f32x4 v = *(const f32x4 *)(c + (size_t)r * N + k);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kk = k + j;
                if (kk < n_cls) se += expf(mr.s * (kk == y ? margin_phi(mr, v[j]) : v[j]) - mx);
            }
        }
    se = fc_wave_sum(se);
    zy = fc_wave_sum(zy);                                   // one lane holds the label column, the others 0
    const float l = mx + logf(se);
    if (row < B && lane == 0) {
        lse[row] = l;
        row_loss[row] = l - zy;
    }
}

// one wave per row: gc [M, N] (pad columns 0) and r[row] = sum_j gc c.
// CE:  gc = s (gloss / M) (exp(z - lse) - [j == y]), the label column times dphi/dc.   !CE: gc = s gout [M, n_cls].
template <bool CE>
__global__ void __launch_bounds__(256) margin_bwd_rows_kernel(const float *c, const long long *labels, const float *lse,
                                                              const float *gloss, const float *gout, float *gc,
                                                              float *r_out, int M, int N, int n_cls, MarginRule mr) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float coef = CE ? mr.s * (gloss[0] / (float)M) : mr.s;
    const float l = CE ? lse[row] : 0.f;
    const long long y = CE ? labels[row] : -1;
    float racc = 0.f;
    for (int k = 4 * lane; k < N; k += 256) {
        const f32x4 cv = *(const f32x4 *)(c + (size_t)row * N + k);
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int kk = k + j;
            if (kk < n_cls) {
                if (CE) {
                    const bool at = kk == y;
                    const float z = mr.s * (at ? margin_phi(mr, cv[j]) : cv[j]);
                    g[j] = coef * (expf(z - l) - (at ? 1.0f : 0.0f));
                    if (at) g[j] *= margin_dphi(mr, cv[j]);
                } else {
                    g[j] = coef * gout[(size_t)row * n_cls + kk];
                }
            }
            racc = __builtin_fmaf(g[j], cv[j], racc);
        }
        *(f32x4 *)(gc + (size_t)row * N + k) = g;
    }
    racc = fc_wave_sum(racc);
    if (lane == 0) r_out[row] = racc;
}

// q[j] = sum_i gc[i,j] c[i,j]: a workgroup of 16 waves on 64 columns, wave w sums rows w, w + 16, ... in ascending order,
// the 16 sums are added in wave order -- no atomics, one order for a given M
constexpr int COL_WAVES = 16;
__global__ void __launch_bounds__(1024) margin_colsum_kernel(const float *gc, const float *c, float *q, int M, int N) {
    float *part = ds_dynamic_lds();                         // [COL_WAVES][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    float acc = 0.f;
    for (int i = wave; i < M; i += COL_WAVES) acc = __builtin_fmaf(gc[(size_t)i * N + col], c[(size_t)i * N + col], acc);
    part[wave * 64 + lane] = acc;
    __syncthreads();
    if (wave == 0) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < COL_WAVES; ++w) t += part[w * 64 + lane];
        q[col] = t;
    }
}

// one wave per row: out = inv[row] (g - coef[row] u)
__global__ void __launch_bounds__(256) margin_fixup_kernel(const float *g, const float *u, const float *coef,
                                                           const float *inv, float *out, int R, int K) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const float cf = coef[row], iv = inv[row];
    const f32x4 *gp = (const f32x4 *)(g + (size_t)row * K), *up = (const f32x4 *)(u + (size_t)row * K);
    f32x4 *o = (f32x4 *)(out + (size_t)row * K);
    for (int v = lane; v < (K >> 2); v += 64) {
        const f32x4 gv = gp[v], uv = up[v];
        f32x4 t;
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = iv * __builtin_fmaf(-cf, uv[j], gv[j]);
        o[v] = t;
    }
}

static int margin_rule(MarginRule &mr, float scale, float margin, int kind) {
    DS_REQUIRE(kind == DS_MARGIN_AAM || kind == DS_MARGIN_AM, DS_ERR_UNSUPPORTED);
    // (the float nearest pi/2 lies above it: compare in double)
    DS_REQUIRE(scale > 0.f && scale <= 3.4028234e38f && margin >= 0.f && (double)margin < 1.5707963267948966,
               DS_ERR_BAD_SHAPE);
    mr.s = scale;
    mr.m = margin;
    mr.cos_m = (float)cos((double)margin);
    mr.sin_m = (float)sin((double)margin);
    mr.m_sin_m = (float)((double)margin * sin((double)margin));
    mr.kind = kind;
    return DS_OK;
}

static bool gemm_shape_ok(int M, int K, int N, int n_cls) {
    return M > 0 && K > 0 && N > 0 && K % (4 * CK) == 0 && N % 128 == 0 && n_cls > 0 && n_cls <= N;
}

template <bool CE>
static int margin_forward(const float *xhat, const float *w_packed, float *workspace, float *c, const long long *labels,
                          float *row_loss, float *lse, float *loss, float *cos_out, int M, int K, int N, int n_cls,
                          const MarginRule &mr, void *stream) {
    const int S = fc_splits(K), n_tiles = N / 128, m_tiles = ds_ceil_div(M, 32);
    DS_LAUNCH(fc_splitk_kernel, m_tiles * n_tiles * S, 256, 0, stream, xhat, w_packed, workspace, M, K, N, S, n_tiles);
    int rc = ds_last_launch_error();
    if (rc) return rc;
    DS_LAUNCH(margin_reduce_kernel<CE>, ds_ceil_div(M, 4), 256, 0, stream, (const float *)workspace, c, labels, row_loss,
              lse, cos_out, M, N, n_cls, S, mr);
    rc = ds_last_launch_error();
    if (rc || !CE) return rc;
    DS_LAUNCH(fc_mean_kernel, 1, 256, 64, stream, (const float *)row_loss, loss, M);
    return ds_last_launch_error();
}

static int margin_colsum(const float *gc, const float *c, float *q, int M, int N, void *stream) {
    DS_LAUNCH(margin_colsum_kernel, N / 64, 64 * COL_WAVES, COL_WAVES * 64 * sizeof(float), stream, gc, c, q, M, N);
    return ds_last_launch_error();
}

}  // namespace

extern "C" int ds_row_normalize_f32(const float *x, float *xhat, float *inv, int R, int R_out, int K, void *stream) {
    DS_REQUIRE(x && xhat && inv, DS_ERR_NULL);
    DS_REQUIRE(R > 0 && R_out >= R && K > 0 && K % 4 == 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(DS_ALIGNED16(x) && DS_ALIGNED16(xhat), DS_ERR_ALIGNMENT);
    DS_LAUNCH(row_normalize_kernel, ds_ceil_div(R_out, 4), 256, 0, stream, x, xhat, inv, R, R_out, K);
    return ds_last_launch_error();
}

extern "C" long long ds_fc_margin_workspace_floats(int M, int K, int N) {
    if (!gemm_shape_ok(M, K, N, 1)) return DS_ERR_BAD_SHAPE;
    return (long long)fc_splits(K) * M * N;
}

extern "C" int ds_fc_margin_ce_fwd_f32(const float *xhat, const float *w_packed, float *workspace, float *c,
                                       const long long *labels, float *row_loss, float *lse, float *loss, int M, int K,
                                       int N, int n_cls, float scale, float margin, int kind, void *stream) {
    DS_REQUIRE(xhat && w_packed && workspace && c && labels && row_loss && lse && loss, DS_ERR_NULL);
    DS_REQUIRE(gemm_shape_ok(M, K, N, n_cls), DS_ERR_BAD_SHAPE);
    DS_REQUIRE(DS_ALIGNED16(xhat) && DS_ALIGNED16(w_packed) && DS_ALIGNED16(workspace) && DS_ALIGNED16(c), DS_ERR_ALIGNMENT);
    MarginRule mr;
    int rc = margin_rule(mr, scale, margin, kind);
    if (rc) return rc;
    return margin_forward<true>(xhat, w_packed, workspace, c, labels, row_loss, lse, loss, nullptr, M, K, N, n_cls, mr,
                                stream);
}

extern "C" int ds_fc_cosine_fwd_f32(const float *xhat, const float *w_packed, float *workspace, float *c, float *cos_out,
                                    int M, int K, int N, int n_cls, float scale, void *stream) {
    DS_REQUIRE(xhat && w_packed && workspace && c && cos_out, DS_ERR_NULL);
    DS_REQUIRE(gemm_shape_ok(M, K, N, n_cls), DS_ERR_BAD_SHAPE);
    DS_REQUIRE(DS_ALIGNED16(xhat) && DS_ALIGNED16(w_packed) && DS_ALIGNED16(workspace) && DS_ALIGNED16(c), DS_ERR_ALIGNMENT);
    MarginRule mr;
    int rc = margin_rule(mr, scale, 0.f, DS_MARGIN_AM);
    if (rc) return rc;
    return margin_forward<false>(xhat, w_packed, workspace, c, nullptr, nullptr, nullptr, nullptr, cos_out, M, K, N, n_cls,
                                 mr, stream);
}

extern "C" int ds_margin_ce_bwd_f32(const float *c, const long long *labels, const float *lse, const float *grad_loss,
                                    float *gc, float *r, float *q, int M, int N, int n_cls, float scale, float margin,
                                    int kind, void *stream) {
    DS_REQUIRE(c && labels && lse && grad_loss && gc && r && q, DS_ERR_NULL);
    DS_REQUIRE(M > 0 && N > 0 && N % 128 == 0 && n_cls > 0 && n_cls <= N, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(DS_ALIGNED16(c) && DS_ALIGNED16(gc), DS_ERR_ALIGNMENT);
    MarginRule mr;
    int rc = margin_rule(mr, scale, margin, kind);
    if (rc) return rc;
    DS_LAUNCH(margin_bwd_rows_kernel<true>, ds_ceil_div(M, 4), 256, 0, stream, c, labels, lse, grad_loss,
              (const float *)nullptr, gc, r, M, N, n_cls, mr);
    rc = ds_last_launch_error();
    if (rc) return rc;
    return margin_colsum((const float *)gc, c, q, M, N, stream);
}

extern "C" int ds_cosine_bwd_f32(const float *c, const float *grad_out, float *gc, float *r, float *q, int M, int N,
                                 int n_cls, float scale, void *stream) {
    DS_REQUIRE(c && grad_out && gc && r && q, DS_ERR_NULL);
    DS_REQUIRE(M > 0 && N > 0 && N % 128 == 0 && n_cls > 0 && n_cls <= N, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(DS_ALIGNED16(c) && DS_ALIGNED16(gc), DS_ERR_ALIGNMENT);
    MarginRule mr;
    int rc = margin_rule(mr, scale, 0.f, DS_MARGIN_AM);
    if (rc) return rc;
    DS_LAUNCH(margin_bwd_rows_kernel<false>, ds_ceil_div(M, 4), 256, 0, stream, c, (const long long *)nullptr,
              (const float *)nullptr, (const float *)nullptr, grad_out, gc, r, M, N, n_cls, mr);
    rc = ds_last_launch_error();
    if (rc) return rc;
    return margin_colsum((const float *)gc, c, q, M, N, stream);
}

extern "C" int ds_margin_grad_fixup_f32(const float *g, const float *u, const float *coef, const float *inv, float *out,
                                        int R, int K, void *stream) {
    DS_REQUIRE(g && u && coef && inv && out, DS_ERR_NULL);
    DS_REQUIRE(R > 0 && K > 0 && K % 4 == 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(DS_ALIGNED16(g) && DS_ALIGNED16(u) && DS_ALIGNED16(out), DS_ERR_ALIGNMENT);
    DS_LAUNCH(margin_fixup_kernel, ds_ceil_div(R, 4), 256, 0, stream, g, u, coef, inv, out, R, K);
    return ds_last_launch_error();
}
