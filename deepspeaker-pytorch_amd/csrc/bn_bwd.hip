// bn_bwd.hip -- backward of train-mode BatchNorm (f32 class: the f32 and bf16x3 training steps) for a batch of G members
// with their own statistics (one member: G = 1), its split forms for data parallelism (float64 sums between the
// reduction and the application), the float64 fold of partial rows (forward and backward) and the column sum of the
// fc bias gradient.
#include <ds_device.h>
#include "ds_common.h"
#include "bn_fold.h"

// =================================================================================================
// backward kernels of BatchNorm (train mode) -- autograd of reference model.py:70,74,188,... as
// executed by loss.backward() (train_triplet.py:223,290); formulas: SURVEY 8(a) a13
// =================================================================================================
namespace {

// gy = (g1 [+ g2]) * [0 < act < 20]   (the clipped-ReLU mask; act == nullptr: no mask)
// partial[blk][c] = { sum gy, sum gy * xhat },  xhat = (z - mean) * invstd.   gy is also written out.
__global__ void __launch_bounds__(256) bn_bwd_reduce_kernel(const float *g1, const float *g2, const float *act,
                                                            const float *z, const float *mean, const float *invstd,
                                                            float *gy, float *partial, long long n_pix, int C,
                                                            int pix_per_block, int blocks_per_member) {
    // a batch of G members with their own statistics (the three forwards of a triplet step run as one batch): member
    // m = blockIdx.x / blocks_per_member owns pixels [m * n_pix, (m + 1) * n_pix), row m of mean / invstd and
    // blocks_per_member partial rows
    const int member = blockIdx.x / blocks_per_member, mblock = blockIdx.x - member * blocks_per_member;
    {
        const size_t off = (size_t)member * n_pix * C;
        g1 += off;
        if (g2) g2 += off;
        if (act) act += off;
        z += off;
        gy += off;
        mean += (size_t)member * C;
        invstd += (size_t)member * C;
    }
    float *red = ds_dynamic_lds();                         // [slots][C][2]
    const int cvec = C >> 2;
    const int slots = 256 / cvec;
    const int cg = threadIdx.x % cvec, slot = threadIdx.x / cvec;
    const long long p0 = (long long)mblock * pix_per_block;
    long long p1 = p0 + pix_per_block;
    if (p1 > n_pix) p1 = n_pix;
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    if (slot < slots) {
        const f32x4 mu = ((const f32x4 *)mean)[cg], is = ((const f32x4 *)invstd)[cg];
        for (long long p = p0 + slot; p < p1; p += slots) {
            const size_t i = (size_t)p * cvec + cg;
            f32x4 g = ((const f32x4 *)g1)[i];
            if (g2) g += ((const f32x4 *)g2)[i];
            if (act) {
                const f32x4 a = ((const f32x4 *)act)[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) g[j] = (a[j] > 0.0f && a[j] < 20.0f) ? g[j] : 0.0f;
            }
            ((f32x4 *)gy)[i] = g;
            const f32x4 xh = (((const f32x4 *)z)[i] - mu) * is;
            s1 += g;
            s2 += g * xh;
        }
        // From here on this restates block_fold<4> of bn_fold.h (red, s1, s2, slot, slots, cg, C, partial), written out:
        // calling it gives the same 335 instructions with other registers and another schedule around the loop, and
        // this is the one hot kernel of the file -- its text stays what was measured.  Change the two together.
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            red[((slot * C) + cg * 4 + j) * 2 + 0] = s1[j];
            red[((slot * C) + cg * 4 + j) * 2 + 1] = s2[j];
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

// fold the partials (double precision, fixed order): dgamma = sum gy*xhat, dbeta = sum gy,
// coef = { gamma*invstd, sum gy / N, sum gy*xhat / N } -- for a batch of G members in one launch: workgroup (member,
// channel group); per member its own partial rows, invstd row, coefficient block and dgamma / dbeta rows (summed over
// the members by bn_member_sum_kernel; one member: the rows ARE the layer's dgamma / dbeta)
__global__ void __launch_bounds__(256) bn_bwd_finalize_group_kernel(const float *partial, int n_partial, double count,
                                                                    const float *gamma, const float *invstd,
                                                                    float *ggamma_m, float *gbeta_m, float *coef, int C,
                                                                    int n_cgroups) {
    double *red = (double *)ds_dynamic_lds();              // [4 waves][FOLD_C][2] (128 of the bytes the launch asks for)
    const int member = blockIdx.x / n_cgroups, cgroup = blockIdx.x - member * n_cgroups;
    partial += (size_t)member * n_partial * C * 2;
    invstd += (size_t)member * C;
    coef += (size_t)member * 3 * C;
    int c;
    double t1, t2;
    if (fold_partials(partial, n_partial, C, red, c, t1, t2, cgroup)) {
        gbeta_m[(size_t)member * C + c] = (float)t1;
        ggamma_m[(size_t)member * C + c] = (float)t2;
        bn_bwd_store_coef(coef, C, c, gamma[c], invstd[c], t1, t2, count);
    }
}

// dgamma / dbeta of the layer = the members' contributions added in member order (what accumulating the reference's
// three backward passes into .grad does)
__global__ void __launch_bounds__(256) bn_member_sum_kernel(const float *ggamma_m, const float *gbeta_m, float *ggamma,
                                                            float *gbeta, int G, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) {
        float a = 0.f, b = 0.f;
        for (int m = 0; m < G; ++m) {
            a += ggamma_m[(size_t)m * C + c];
            b += gbeta_m[(size_t)m * C + c];
        }
        ggamma[c] = a;
        gbeta[c] = b;
    }
}

// gz = gamma*invstd * (gy - mean(gy) - xhat * mean(gy*xhat)), every member with its own rows of the tables
__global__ void __launch_bounds__(256) bn_bwd_apply_group_kernel(const float *gy, const float *z, const float *mean,
                                                                 const float *invstd, const float *coef, float *gz,
                                                                 long long n_vec_member, int G, int C) {
    const int cvec = C >> 2;                    // a power of two dividing 256 (checked by the host): fixed channel group
    const int c4 = threadIdx.x & (cvec - 1);
    for (int member = 0; member < G; ++member) {            // (no per-vector division: members are walked one by one)
        const float *mu_p = mean + (size_t)member * C, *is_p = invstd + (size_t)member * C, *cf = coef + (size_t)member * 3 * C;
        const f32x4 mu = ((const f32x4 *)mu_p)[c4], is = ((const f32x4 *)is_p)[c4];
        const f32x4 k1 = ((const f32x4 *)cf)[c4], k2 = ((const f32x4 *)(cf + C))[c4], k3 = ((const f32x4 *)(cf + 2 * C))[c4];
        const size_t mbase = (size_t)member * (size_t)n_vec_member;
        for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < n_vec_member; v += (long long)gridDim.x * 256) {
            const size_t i = mbase + (size_t)v;
            const f32x4 xh = (((const f32x4 *)z)[i] - mu) * is;
            ((f32x4 *)gz)[i] = k1 * (((const f32x4 *)gy)[i] - k2 - xh * k3);
        }
    }
}

// out[c] = sum_r x[r][c]   (bias gradient of the fc layer).  A workgroup owns 32 columns; its 8 row lanes stride over
// the rows and are folded in lane order (fixed order => deterministic).  (One thread per column walking all rows left
// two workgroups busy for 170 us at the head of every backward pass.)
__global__ void __launch_bounds__(256) colsum_kernel(const float *x, float *out, int R, int C) {
    float *red = ds_dynamic_lds();                         // [8][32]
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    float s = 0.f;
    if (c < C)
        for (int r = rl; r < R; r += 8) s += x[(size_t)r * C + c];
    red[rl * 32 + cl] = s;
    __syncthreads();
    if (rl == 0 && c < C) {
        float t = 0.f;
        for (int k = 0; k < 8; ++k) t += red[k * 32 + cl];
        out[c] = t;
    }
}

}  // namespace

// ---- split forms for data-parallel training: local sums -> (all-reduce by the caller) -> finish ----
namespace {

// Partial rows -> float64 sums, folded like the single-process finalize kernels fold them (fold_partials: FOLD_C
// channels x FOLD_R row lanes per workgroup; one workgroup per 32 channels with 8 row lanes left 6..48 workgroups
// walking up to 2048 rows each: 66 us per BatchNorm layer of the data-parallel step).  A batch of G members with their
// own statistics: workgroup = (member, channel group).  sums is [G][2C+1] doubles: per member C pairs, then the
// member's pixel count (which travels with the all-reduce); count <= 0: the pairs alone, the count slot is not
// written (ds_partial_sum_f64 promises [C][2]).
__global__ void __launch_bounds__(256) partial_sum_f64_group_kernel(const float *partial, int n_partial, double *sums,
                                                                    double count, int C, int n_cgroups) {
    double *red = (double *)ds_dynamic_lds();              // [4 waves][FOLD_C][2] (128 of the bytes the launch asks for)
    const int member = blockIdx.x / n_cgroups, cgroup = blockIdx.x - member * n_cgroups;
    partial += (size_t)member * n_partial * C * 2;
    sums += (size_t)member * (2 * C + 1);
    if (count > 0.0 && cgroup == 0 && threadIdx.x == 0) sums[2 * C] = count;
    int c;
    double t1, t2;
    if (fold_partials(partial, n_partial, C, red, c, t1, t2, cgroup)) {
        sums[c * 2 + 0] = t1;
        sums[c * 2 + 1] = t2;
    }
}

// the coefficients of bn_bwd_finalize_group_kernel from (all-reduced) sums; count <= 0: the member's count slot
__global__ void __launch_bounds__(256) bn_bwd_from_sums_group_kernel(const double *sums, double count,
                                                                     const float *gamma, const float *invstd,
                                                                     float *ggamma_m, float *gbeta_m, float *coef,
                                                                     int C, int n_cgroups) {
    const int member = blockIdx.x / n_cgroups, cgroup = blockIdx.x - member * n_cgroups;
    const int c = cgroup * 256 + threadIdx.x;
    if (c >= C) return;
    sums += (size_t)member * (2 * C + 1);
    invstd += (size_t)member * C;
    coef += (size_t)member * 3 * C;
    if (count <= 0.0) count = sums[2 * C];
    gbeta_m[(size_t)member * C + c] = (float)sums[c * 2];
    ggamma_m[(size_t)member * C + c] = (float)sums[c * 2 + 1];
    bn_bwd_store_coef(coef, C, c, gamma[c], invstd[c], sums[c * 2], sums[c * 2 + 1], count);
}

// ---- the stages on the host side, every launch written once ----
// No argument checks in here: each entry point below keeps the DS_REQUIRE conditions and return codes it has always
// had, and they differ (only the grouped forms ask for aligned g2 / act; ds_bn_bwd_apply_f32 asks for neither
// C <= 1024 nor any alignment; the split halves check only what they read).  Making them one set would change what
// callers are refused for, so they are deliberately NOT unified here.

// gy and the partial rows of G members: G * ds_bn_bwd_partial_rows(n_pix, C) rows of [C][2]
int bwd_reduce(const float *g1, const float *g2, const float *act, const float *z, const float *mean,
               const float *invstd, float *gy, float *partial, long long n_pix, int C, int G, void *stream) {
    const int blocks = ds_bn_bwd_partial_rows(n_pix, C);
    const int ppb = (int)((n_pix + blocks - 1) / blocks);
    const int slots = 256 / (C / 4);
    DS_LAUNCH(bn_bwd_reduce_kernel, blocks * G, 256, (size_t)slots * C * 2 * 4, stream, g1, g2, act, z, mean, invstd, gy,
              partial, n_pix, C, ppb, blocks);
    return ds_last_launch_error();
}

// n_partial rows per member -> sums [G][2C+1] float64 (count <= 0: [C][2] without the count slot, G = 1)
int fold_to_sums(const float *partial, int n_partial, double *sums, double count, int C, int G, void *stream) {
    const int n_cgroups = ds_ceil_div(C, FOLD_C);
    DS_LAUNCH(partial_sum_f64_group_kernel, n_cgroups * G, 256, FOLD_R * FOLD_C * 2 * sizeof(double), stream, partial,
              n_partial, sums, count, C, n_cgroups);
    return ds_last_launch_error();
}

// Coefficients and dgamma / dbeta from the members' partial rows (`partial`, n_partial rows each, over `count` pixels)
// or, partial == nullptr, from their float64 `sums` (count 0: each member's own count slot), then gz of all members.
// G = 1: the coefficient kernel's one dgamma / dbeta row IS ggamma / gbeta -- no member sum, member_sums is not
// touched: the three launches of the single-member forms, and a dgamma of -0.f stays -0.f (0.f + -0.f is +0.f).
int bwd_finish(const float *partial, int n_partial, const double *sums, double count, const float *gy, const float *z,
               const float *mean, const float *invstd, const float *gamma, float *coef, float *member_sums,
               float *ggamma, float *gbeta, float *gz, long long n_pix, int C, int G, void *stream) {
    float *gg_m = G == 1 ? ggamma : member_sums, *gb_m = G == 1 ? gbeta : member_sums + (size_t)G * C;
    if (partial) {
        const int n_cgroups = ds_ceil_div(C, FOLD_C);
        DS_LAUNCH(bn_bwd_finalize_group_kernel, n_cgroups * G, 256, FOLD_R * FOLD_C * 2 * sizeof(double), stream, partial,
                  n_partial, count, gamma, invstd, gg_m, gb_m, coef, C, n_cgroups);
    } else {
        DS_LAUNCH(bn_bwd_from_sums_group_kernel, ds_ceil_div(C, 256) * G, 256, 0, stream, sums, count, gamma, invstd, gg_m,
                  gb_m, coef, C, ds_ceil_div(C, 256));
    }
    int rc = ds_last_launch_error();
    if (rc) return rc;
    if (G > 1) {
        DS_LAUNCH(bn_member_sum_kernel, ds_ceil_div(C, 256), 256, 0, stream, (const float *)gg_m, (const float *)gb_m,
                  ggamma, gbeta, G, C);
        rc = ds_last_launch_error();
        if (rc) return rc;
    }
    const long long n_vec_member = n_pix * (C / 4);
    DS_LAUNCH(bn_bwd_apply_group_kernel, grid_for(n_vec_member * G), 256, 0, stream, gy, z, mean, invstd,
              (const float *)coef, gz, n_vec_member, G, C);
    return ds_last_launch_error();
}

}  // namespace

// Workgroups (= partial rows) of the reduction: a workgroup walks its pixels 1024 / C at a time, so the pixels per
// workgroup shrink with the channel count (about 8 steps per thread) -- the 10x4 stage of a 256-utterance member
// has only 10 k pixels, and 256 of them per workgroup left 40 workgroups on 256 CUs -- bounded by 2048 rows.
extern "C" int ds_bn_bwd_partial_rows(long long n_pix, int C) {
    if (n_pix <= 0 || C <= 0) return DS_ERR_BAD_SHAPE;
    long long ppb = 8192 / C;
    if (ppb < 8) ppb = 8;
    long long blocks = (n_pix + ppb - 1) / ppb;
    if (blocks > 2048) blocks = 2048;
    return (int)blocks;
}

// ---- the float64 folds of data-parallel training, forward and backward (the forward's second half,
// ds_bn_stats_from_sums_f32, is with the other forward statistics in bn_pack.hip) ----
// sums [C][2] float64 of one member's partial rows: ds_partial_sum_f64_group with G = 1, minus the count slot
extern "C" int ds_partial_sum_f64(const float *partial, int n_partial, double *sums, int C, void *stream) {
    DS_REQUIRE(partial && sums, DS_ERR_NULL);
    DS_REQUIRE(n_partial > 0 && C > 0, DS_ERR_BAD_SHAPE);
    return fold_to_sums(partial, n_partial, sums, 0.0, C, 1, stream);
}

// per-tile partial statistics of G members (each n_partial rows of [C][2]) -> sums [G][2C+1] float64 in ONE launch
// (what the per-BatchNorm-layer all-reduce of data-parallel training carries)
extern "C" int ds_partial_sum_f64_group(const float *partial, int n_partial, double *sums, long long count, int C, int G,
                                        void *stream) {
    DS_REQUIRE(partial && sums, DS_ERR_NULL);
    DS_REQUIRE(n_partial > 0 && C > 0 && G > 0 && G <= 64 && count > 0, DS_ERR_BAD_SHAPE);
    return fold_to_sums(partial, n_partial, sums, (double)count, C, G, stream);
}

// ---- the backward of one member: the G = 1 case of the grouped forms below (three launches) ----
extern "C" int ds_bn_bwd_f32(const float *g1, const float *g2, const float *act, const float *z, const float *mean,
                             const float *invstd, const float *gamma, float *gy, float *partial, float *coef,
                             float *ggamma, float *gbeta, float *gz, long long n_pix, int C, void *stream) {
    DS_REQUIRE(g1 && z && mean && invstd && gamma && gy && partial && coef && ggamma && gbeta && gz, DS_ERR_NULL);
    DS_REQUIRE(n_pix > 0 && C >= 4 && (C % 4) == 0 && C <= 1024 && 256 % (C / 4) == 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(DS_ALIGNED16(g1) && DS_ALIGNED16(z) && DS_ALIGNED16(gy) && DS_ALIGNED16(gz) && DS_ALIGNED16(mean) &&
                   DS_ALIGNED16(invstd) && DS_ALIGNED16(coef), DS_ERR_ALIGNMENT);
    const int rc = bwd_reduce(g1, g2, act, z, mean, invstd, gy, partial, n_pix, C, 1, stream);
    if (rc) return rc;
    return bwd_finish(partial, ds_bn_bwd_partial_rows(n_pix, C), nullptr, (double)n_pix, gy, z, mean, invstd, gamma, coef,
                      nullptr, ggamma, gbeta, gz, n_pix, C, 1, stream);
}

// ds_bn_bwd_f32 split for data parallelism: the reduction alone (the caller folds the rows with ds_partial_sum_f64
// and all-reduces the sums), then coefficients, dgamma / dbeta and gz from the sums (count 0: read sums[2C])
extern "C" int ds_bn_bwd_reduce_f32(const float *g1, const float *g2, const float *act, const float *z,
                                    const float *mean, const float *invstd, float *gy, float *partial,
                                    long long n_pix, int C, void *stream) {
    DS_REQUIRE(g1 && z && mean && invstd && gy && partial, DS_ERR_NULL);
    DS_REQUIRE(n_pix > 0 && C >= 4 && (C % 4) == 0 && C <= 1024 && 256 % (C / 4) == 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(DS_ALIGNED16(g1) && DS_ALIGNED16(z) && DS_ALIGNED16(gy) && DS_ALIGNED16(mean) && DS_ALIGNED16(invstd),
               DS_ERR_ALIGNMENT);
    return bwd_reduce(g1, g2, act, z, mean, invstd, gy, partial, n_pix, C, 1, stream);
}

extern "C" int ds_bn_bwd_apply_f32(const double *sums, long long count, const float *gy, const float *z,
                                   const float *mean, const float *invstd, const float *gamma, float *coef,
                                   float *ggamma, float *gbeta, float *gz, long long n_pix, int C, void *stream) {
    DS_REQUIRE(sums && gy && z && mean && invstd && gamma && coef && ggamma && gbeta && gz, DS_ERR_NULL);
    DS_REQUIRE(n_pix > 0 && count >= 0 && C >= 4 && (C % 4) == 0, DS_ERR_BAD_SHAPE);
    return bwd_finish(nullptr, 0, sums, (double)count, gy, z, mean, invstd, gamma, coef, nullptr, ggamma, gbeta, gz, n_pix,
                      C, 1, stream);
}

// ---- the backward of a batch made of G members with their own batch statistics (Engine.forward_train_group: the
// three forwards of a triplet step as one batch), in four launches instead of 3 G + 2 (G = 1: three): g1 / g2 / act /
// z / gy / gz are [G * n_pix, C]; mean, invstd [G][C]; partial G * ds_bn_bwd_partial_rows(n_pix, C) * C * 2 floats;
// coef [G][3C]; member_sums [2][G][C] scratch (G = 1: not touched); ggamma / gbeta [C] = the members' dgamma / dbeta
// added in member order. ----
extern "C" int ds_bn_bwd_group_f32(const float *g1, const float *g2, const float *act, const float *z, const float *mean,
                                   const float *invstd, const float *gamma, float *gy, float *partial, float *coef,
                                   float *member_sums, float *ggamma, float *gbeta, float *gz, long long n_pix, int C,
                                   int G, void *stream) {
    DS_REQUIRE(g1 && z && mean && invstd && gamma && gy && partial && coef && member_sums && ggamma && gbeta && gz,
               DS_ERR_NULL);
    DS_REQUIRE(n_pix > 0 && G > 0 && G <= 64 && C >= 4 && (C % 4) == 0 && C <= 1024 && 256 % (C / 4) == 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(DS_ALIGNED16(g1) && DS_ALIGNED16(z) && DS_ALIGNED16(gy) && DS_ALIGNED16(gz) && DS_ALIGNED16(mean) &&
                   DS_ALIGNED16(invstd) && DS_ALIGNED16(coef) && (!g2 || DS_ALIGNED16(g2)) && (!act || DS_ALIGNED16(act)),
               DS_ERR_ALIGNMENT);
    const int rc = bwd_reduce(g1, g2, act, z, mean, invstd, gy, partial, n_pix, C, G, stream);
    if (rc) return rc;
    return bwd_finish(partial, ds_bn_bwd_partial_rows(n_pix, C), nullptr, (double)n_pix, gy, z, mean, invstd, gamma, coef,
                      member_sums, ggamma, gbeta, gz, n_pix, C, G, stream);
}

// ds_bn_bwd_group_f32 split at the point where data-parallel training exchanges the sums: the local
// reductions of all G members -> sums [G][2C+1] float64 (C pairs {sum gy, sum gy*xhat} and the member's pixel count)
// ... all-reduce by the caller ... -> coefficients, dgamma / dbeta and gz of all members.  Two + three launches.
extern "C" int ds_bn_bwd_group_reduce_f32(const float *g1, const float *g2, const float *act, const float *z,
                                          const float *mean, const float *invstd, float *gy, float *partial,
                                          double *sums, long long n_pix, int C, int G, void *stream) {
    DS_REQUIRE(g1 && z && mean && invstd && gy && partial && sums, DS_ERR_NULL);
    DS_REQUIRE(n_pix > 0 && G > 0 && G <= 64 && C >= 4 && (C % 4) == 0 && C <= 1024 && 256 % (C / 4) == 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(DS_ALIGNED16(g1) && DS_ALIGNED16(z) && DS_ALIGNED16(gy) && DS_ALIGNED16(mean) && DS_ALIGNED16(invstd) &&
                   (!g2 || DS_ALIGNED16(g2)) && (!act || DS_ALIGNED16(act)), DS_ERR_ALIGNMENT);
    const int rc = bwd_reduce(g1, g2, act, z, mean, invstd, gy, partial, n_pix, C, G, stream);
    if (rc) return rc;
    return fold_to_sums(partial, ds_bn_bwd_partial_rows(n_pix, C), sums, (double)n_pix, C, G, stream);
}

extern "C" int ds_bn_bwd_group_apply_f32(const double *sums, const float *gy, const float *z, const float *mean,
                                         const float *invstd, const float *gamma, float *coef, float *member_sums,
                                         float *ggamma, float *gbeta, float *gz, long long n_pix, int C, int G,
                                         void *stream) {
    DS_REQUIRE(sums && gy && z && mean && invstd && gamma && coef && member_sums && ggamma && gbeta && gz, DS_ERR_NULL);
    DS_REQUIRE(n_pix > 0 && G > 0 && G <= 64 && C >= 4 && (C % 4) == 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(DS_ALIGNED16(gy) && DS_ALIGNED16(z) && DS_ALIGNED16(gz) && DS_ALIGNED16(mean) && DS_ALIGNED16(invstd) &&
                   DS_ALIGNED16(coef), DS_ERR_ALIGNMENT);
    return bwd_finish(nullptr, 0, sums, 0.0, gy, z, mean, invstd, gamma, coef, member_sums, ggamma, gbeta, gz, n_pix, C, G,
                      stream);
}

// The second half of ds_bn_bwd_group_f32 alone, for partial sums that were produced elsewhere (the data-gradient kernel
// whose epilogue is the reduction: ds_conv_dgrad_bnbwd_bf16): n_partial rows of [C][2] per member, consecutive.
extern "C" int ds_bn_bwd_group_finish_f32(const float *partial, int n_partial, const float *gy, const float *z,
                                          const float *mean, const float *invstd, const float *gamma, float *coef,
                                          float *member_sums, float *ggamma, float *gbeta, float *gz, long long n_pix,
                                          int C, int G, void *stream) {
    DS_REQUIRE(partial && gy && z && mean && invstd && gamma && coef && member_sums && ggamma && gbeta && gz, DS_ERR_NULL);
    DS_REQUIRE(n_partial > 0 && n_pix > 0 && G > 0 && G <= 64 && C >= 4 && (C % 4) == 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(DS_ALIGNED16(gy) && DS_ALIGNED16(z) && DS_ALIGNED16(gz) && DS_ALIGNED16(mean) && DS_ALIGNED16(invstd) &&
                   DS_ALIGNED16(coef), DS_ERR_ALIGNMENT);
    return bwd_finish(partial, n_partial, nullptr, (double)n_pix, gy, z, mean, invstd, gamma, coef, member_sums, ggamma,
                      gbeta, gz, n_pix, C, G, stream);
}

extern "C" int ds_colsum_f32(const float *x, float *out, int R, int C, void *stream) {
    DS_REQUIRE(x && out, DS_ERR_NULL);
    DS_REQUIRE(R > 0 && C > 0, DS_ERR_BAD_SHAPE);
    DS_LAUNCH(colsum_kernel, ds_ceil_div(C, 32), 256, 8 * 32 * sizeof(float), stream, x, out, R, C);
    return ds_last_launch_error();
}
