// identify.hip -- speaker identification: "which of the M enrolled rows are nearest to this query?"
//   * ds_nearest_topk_f32: for every query row its k smallest gallery rows by the screening distance
//       s(q, g) = (|q|^2 + |g|^2) - 2 q.g,    q.g from v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulation),
//     with the top-k kept inside the kernel: the N x M matrix is never written anywhere.
//   * ds_nearest_rescore_f32: the winners' distances again by direct differences, in the arithmetic of
//     PairwiseDistance (row_distance.h), and the final order by that distance (the GEMM form cancels badly for
//     near-duplicate rows).
//   * ds_segment_mean_rows_f32: speaker models = mean of a speaker's enrolment rows, optionally back on the sphere.
//   * ds_rank_hits_i32: cumulative match counts (rank-1 ... rank-k accuracy).
// Everything is ordered lexicographically by (distance, gallery index), which makes the result a property of the SET of
// rows: it does not depend on the order candidates are met in, on the tiling or on the number of gallery splits.
#include <ds_device.h>
#include "ds_common.h"
#include "row_distance.h"
#include "screen_tile.h"

namespace {

// NQ, NG, the staging constants, row_sqnorm_kernel and the tile GEMM with its screening epilogue: screen_tile.h
constexpr int MAX_SPLITS = 64;

__device__ __forceinline__ bool pair_less(float d, int i, float d2, int i2) { return d < d2 || (d == d2 && i < i2); }

// A workgroup owns NQ queries and walks the NG-row tiles [tile0, tile1) of one gallery split.
//   GEMM and screening epilogue: screen_tile (screen_tile.h), shared with the cohort statistics of score_norm.hip.
//   Top-k: the tile's screening values go to LDS (over the dead staging buffer); four threads per query test 32
//   candidates each against the query's current k-th best, and the query's owner thread inserts the few that pass
//   into the sorted list it keeps in LDS.
__global__ void __launch_bounds__(256) nearest_screen_kernel(const float *q, const float *g, const float *qn,
                                                             const float *gn, const long long *qlab,
                                                             const long long *glab, int mode, float *ws_d, int *ws_i,
                                                             int N, int M, int D, int k, int tiles_per_split,
                                                             int n_qblocks) {
    float *lds = ds_dynamic_lds();
    float *stage = lds;                                    // [NQ + NG][KP], later [NQ][SP]
    float *gn_s = lds + TILE_FLOATS;                       // [NG]
    float *qn_s = gn_s + NG;                               // [NQ]
    long long *glab_s = (long long *)(qn_s + NQ);          // [NG]
    unsigned *mask_s = (unsigned *)(glab_s + NG);          // [NQ][4]
    float *thr_d = (float *)(mask_s + NQ * 4);             // [NQ] the k-th best so far (+inf, INT_MAX while the list is short)
    int *thr_i = (int *)(thr_d + NQ);                      // [NQ]
    const int kp = k | 1;                                  // odd list pitch: the owners' lists start in different banks
    float *list_d = (float *)(thr_i + NQ);                 // [NQ][kp]
    int *list_i = (int *)(list_d + NQ * kp);               // [NQ][kp]

    const int tid = threadIdx.x;
    const int qb = blockIdx.x % n_qblocks, split = blockIdx.x / n_qblocks;
    const int q0 = qb * NQ;
    const int n_tiles = (M + NG - 1) / NG;
    const int tile0 = split * tiles_per_split;
    const int tile1 = tile0 + tiles_per_split < n_tiles ? tile0 + tiles_per_split : n_tiles;

    if (tid < NQ) {
        qn_s[tid] = q0 + tid < N ? qn[q0 + tid] : 0.f;
        thr_d[tid] = __builtin_inff();
        thr_i[tid] = 0x7FFFFFFF;
    }
    // the owner of query `oq` is thread 4 * oq; its list length lives in a register
    const int oq = tid >> 2, seg = tid & 3;
    int cnt = 0;
    const long long my_qlab = (mode != 0 && q0 + oq < N) ? qlab[q0 + oq] : 0;

    f32x4 pre[SLOTS];
    if (tile0 < tile1) screen_fetch(pre, q, g, q0, tile0, 0, N, M, D, tid);
    for (int tile = tile0; tile < tile1; ++tile) {
        const int j0 = tile * NG;
        screen_tile(stage, pre, q, g, qn_s, gn_s, q0, tile, tile + 1 < tile1 ? tile + 1 : -1, N, M, D, [&]() {
            if (tid < NG) {                                // this tile's norms and labels (their last readers are behind us)
                gn_s[tid] = j0 + tid < M ? gn[j0 + tid] : 0.f;
                if (mode != 0) glab_s[tid] = j0 + tid < M ? glab[j0 + tid] : 0;
            }
        });
        {   // 32 candidates per thread against the query's current k-th best
            const float td = thr_d[oq];
            const int ti = thr_i[oq];
            unsigned m = 0;
            if (q0 + oq < N) {
#pragma unroll
                for (int v = 0; v < 8; ++v) {
                    const f32x4 s4 = *(const f32x4 *)(stage + oq * SP + seg * 32 + v * 4);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int c = seg * 32 + v * 4 + u, j = j0 + c;
                        bool ok = j < M && pair_less(s4[u], j, td, ti);
                        if (mode != 0) ok = ok && ((glab_s[c] == my_qlab) == (mode == 2));
                        m |= ok ? 1u << (v * 4 + u) : 0u;
                    }
                }
            }
            mask_s[oq * 4 + seg] = m;
        }
        __syncthreads();
        if (seg == 0) {
            float *ld = list_d + oq * kp;
            int *li = list_i + oq * kp;
            for (int sg = 0; sg < 4; ++sg) {
                unsigned m = mask_s[oq * 4 + sg];
                while (m) {
                    const int bit = __builtin_ctz(m);
                    m &= m - 1;
                    const int c = sg * 32 + bit, j = j0 + c;
                    const float s = stage[oq * SP + c];
                    int pos;
                    if (cnt == k) {
                        if (!pair_less(s, j, ld[k - 1], li[k - 1])) continue;
                        pos = k - 1;
                    } else {
                        pos = cnt++;
                    }
                    while (pos > 0 && pair_less(s, j, ld[pos - 1], li[pos - 1])) {
                        ld[pos] = ld[pos - 1];
                        li[pos] = li[pos - 1];
                        --pos;
                    }
                    ld[pos] = s;
                    li[pos] = j;
                }
            }
            if (cnt == k) {
                thr_d[oq] = ld[k - 1];
                thr_i[oq] = li[k - 1];
            }
            mask_s[oq * 4] = (unsigned)cnt;                // the list length, for the write-out below
        }
    }
    if (tile0 >= tile1 && seg == 0) mask_s[oq * 4] = 0u;
    __syncthreads();
    // this split's lists: [split][N][k], unfilled ranks as (+inf, -1)
    for (int e = tid; e < NQ * k; e += 256) {
        const int qi = e / k, r = e - qi * k;
        if (q0 + qi < N) {
            const bool have = r < (int)mask_s[qi * 4];
            const size_t o = ((size_t)split * N + q0 + qi) * k + r;
            ws_d[o] = have ? list_d[qi * kp + r] : __builtin_inff();
            ws_i[o] = have ? list_i[qi * kp + r] : -1;
        }
    }
}

// One wavefront per query folds the splits' sorted lists: the rank of an entry is its position in its own list plus,
// for every other split, the number of that split's entries that are smaller (binary search; the pairs are distinct
// because a gallery row belongs to one split).
__global__ void __launch_bounds__(256) nearest_merge_kernel(const float *ws_d, const int *ws_i, float *out_d,
                                                            long long *out_i, int N, int k, int n_splits) {
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int qq = qi < N ? qi : N - 1;                    // a dead wave repeats the last query and writes nothing
    const int total = n_splits * k;
    int valid = 0;
    for (int e = lane; e < total; e += 64) {
        const int s = e / k, p = e - s * k;
        const size_t o = ((size_t)s * N + qq) * k;
        const int idx = ws_i[o + p];
        if (idx < 0) continue;
        ++valid;
        const float d = ws_d[o + p];
        int rank = p;
        for (int s2 = 0; s2 < n_splits && rank < k; ++s2) {
            if (s2 == s) continue;
            const size_t o2 = ((size_t)s2 * N + qq) * k;
            int lo = 0, hi = k;                            // first entry of s2 that is not smaller than (d, idx)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const int i2 = ws_i[o2 + mid];
                if (i2 >= 0 && pair_less(ws_d[o2 + mid], i2, d, idx)) lo = mid + 1;
                else hi = mid;
            }
            rank += lo;
        }
        if (rank < k && qi < N) {
            out_d[(size_t)qi * k + rank] = d;
            out_i[(size_t)qi * k + rank] = idx;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) valid += ds_shfl_xor_i(valid, m);
    if (qi < N && lane < k && lane >= valid) {
        out_d[(size_t)qi * k + lane] = __builtin_inff();
        out_i[(size_t)qi * k + lane] = -1;
    }
}

// One wavefront per query: the exact distance of each winner (PairwiseDistance's arithmetic, one pair at a time over
// the whole wave), then the winners in ascending (distance, index) order; missing ranks stay last as (+inf, -1).
__global__ void __launch_bounds__(256) nearest_rescore_kernel(const float *q, const float *g, const long long *idx_in,
                                                              float *out_d, long long *out_i, int N, int D, int k,
                                                              float eps) {
    float *sd = ds_dynamic_lds();                          // [4][64] distances
    int *si = (int *)(sd + 256);                           // [4][64] indices
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qi = blockIdx.x * 4 + wave;
    const int qq = qi < N ? qi : N - 1;
    float my_d = __builtin_inff();
    int my_i = -1;
    for (int r = 0; r < k; ++r) {
        const long long j = idx_in[(size_t)qq * k + r];
        const float s = row_sqdist(q + (size_t)qq * D, g + (size_t)(j >= 0 ? j : 0) * D, D, lane);
        if (lane == r && j >= 0) {
            my_d = sqrtf(s + eps);
            my_i = (int)j;
        }
    }
    sd[wave * 64 + lane] = my_d;
    si[wave * 64 + lane] = my_i;
    ds_wave_sync();
    if (lane < k && qi < N) {
        int rank = 0;
        for (int r = 0; r < k; ++r) {
            const float d2 = sd[wave * 64 + r];
            const int i2 = si[wave * 64 + r];
            // a missing entry sorts after every present one, and among themselves by slot
            const bool less = my_i >= 0 ? (i2 >= 0 && pair_less(d2, i2, my_d, my_i)) : (i2 >= 0 || r < lane);
            rank += less ? 1 : 0;
        }
        out_d[(size_t)qi * k + rank] = my_d;
        out_i[(size_t)qi * k + rank] = my_i;
    }
}

// models[s,:] = mean of emb[offsets[s] .. offsets[s+1]), rows added in order; renorm: scaled to L2 norm alpha as
// l2norm_scale_kernel does ((m / sqrt(sum m^2 + eps)) * alpha).  One wavefront per speaker.
__global__ void __launch_bounds__(256) segment_mean_rows_kernel(const float *emb, const long long *off, float *models,
                                                                int S, int D, int renorm, float alpha, float eps) {
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = s < S;
    const long long a = live ? off[s] : 0, b = live ? off[s + 1] : 0;
    const float cnt = (float)(b - a);
    float *dst = models + (size_t)(live ? s : 0) * D;
    float ss = 0.f;
    for (int k = lane; k < D; k += 64) {
        float sum = 0.f;
        for (long long r = a; r < b; ++r) sum += emb[(size_t)r * D + k];
        const float m = b > a ? sum / cnt : 0.f;
        if (live) dst[k] = m;
        ss += m * m;
    }
    ss = wave_sum(ss);
    if (renorm && live) {
        const float nrm = sqrtf(ss + eps);
        for (int k = lane; k < D; k += 64) dst[k] = (dst[k] / nrm) * alpha;        // this lane's own stores above
    }
}

// hits[r] = number of queries whose own label appears among their first r + 1 results.  One workgroup: every wave
// counts the first-match ranks of 64 queries at a time by ballot, the waves' counts are added in wave order.
__global__ void __launch_bounds__(1024) rank_hits_kernel(const long long *idx, const long long *glab,
                                                         const long long *qlab, int *hits, int N, int k) {
    int *cnt = (int *)ds_dynamic_lds();                    // [16][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    cnt[wave * 64 + lane] = 0;
    ds_wave_sync();
    for (int base = wave * 64; base < N; base += 1024) {
        const int qi = base + lane;
        int first = -1;
        if (qi < N) {
            const long long want = qlab[qi];
            for (int r = 0; r < k; ++r) {
                const long long j = idx[(size_t)qi * k + r];
                if (j >= 0 && glab[j] == want) { first = r; break; }
            }
        }
        for (int r = 0; r < k; ++r) {
            const int n = __popcll(ds_ballot(first == r));
            if (lane == 0) cnt[wave * 64 + r] += n;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int r = 0; r < k; ++r) {
            for (int w = 0; w < 16; ++w) run += cnt[w * 64 + r];
            hits[r] = run;
        }
    }
}

struct nearest_plan { int n_qblocks, n_tiles, tiles_per_split, n_splits; };

// splits == 0: enough gallery ranges that the workgroups fill the chip twice over, as far as there are tiles
nearest_plan plan_nearest(int N, int M, int splits) {
    nearest_plan p;
    p.n_qblocks = ds_ceil_div(N, NQ);
    p.n_tiles = ds_ceil_div(M, NG);
    int want = splits > 0 ? splits : ds_ceil_div(2 * ds_cu_count(), p.n_qblocks);
    if (want > MAX_SPLITS) want = MAX_SPLITS;
    if (want > p.n_tiles) want = p.n_tiles;
    p.tiles_per_split = ds_ceil_div(p.n_tiles, want);
    p.n_splits = ds_ceil_div(p.n_tiles, p.tiles_per_split);
    return p;
}

bool nearest_shape_ok(int N, int M, int D, int k, int splits) {
    // (N, M <= 2^30: row and workgroup indices stay inside an int)
    return N > 0 && M > 0 && N <= (1 << 30) && M <= (1 << 30) && D > 0 && D % 4 == 0 && D <= DS_NEAREST_MAX_D && k >= 1 &&
           k <= DS_NEAREST_MAX_K && splits >= 0;
}

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

extern "C" long long ds_nearest_workspace_bytes(int N, int M, int D, int k, int splits) {
    if (!nearest_shape_ok(N, M, D, k, splits)) return DS_ERR_BAD_SHAPE;
    const nearest_plan p = plan_nearest(N, M, splits);
    return (long long)(align16((size_t)N * 4) + align16((size_t)M * 4) + 2 * align16((size_t)p.n_splits * N * k * 4));
}

extern "C" int ds_nearest_topk_f32(const float *queries, const float *gallery, const long long *query_label,
                                   const long long *gallery_label, int mode, void *workspace, float *out_dist,
                                   long long *out_index, int N, int M, int D, int k, int splits, void *stream) {
    DS_REQUIRE(queries && gallery && workspace && out_dist && out_index, DS_ERR_NULL);
    DS_REQUIRE(mode >= 0 && mode <= 2, DS_ERR_UNSUPPORTED);
    DS_REQUIRE(mode == 0 || (query_label && gallery_label), DS_ERR_NULL);
    DS_REQUIRE(nearest_shape_ok(N, M, D, k, splits), DS_ERR_BAD_SHAPE);
    DS_REQUIRE(DS_ALIGNED16(queries) && DS_ALIGNED16(gallery) && DS_ALIGNED16(workspace), DS_ERR_ALIGNMENT);
    const nearest_plan p = plan_nearest(N, M, splits);
    char *ws = (char *)workspace;
    float *qn = (float *)ws;
    float *gn = (float *)(ws + align16((size_t)N * 4));
    float *ws_d = (float *)((char *)gn + align16((size_t)M * 4));
    int *ws_i = (int *)((char *)ws_d + align16((size_t)p.n_splits * N * k * 4));
    DS_LAUNCH(row_sqnorm_kernel, (int)ds_ceil_div_ll((long long)N + M, 4), 256, 0, stream, queries, gallery, qn, gn, N, M, D);
    int rc = ds_last_launch_error();
    if (rc) return rc;
    const size_t lds = ((size_t)TILE_FLOATS + NG + NQ + 2 * NG + 4 * NQ + 2 * NQ + 2 * (size_t)NQ * (k | 1)) * 4;
    DS_LAUNCH_BIG_LDS(nearest_screen_kernel, p.n_qblocks * p.n_splits, 256, lds, stream, queries, gallery, (const float *)qn,
                      (const float *)gn, query_label, gallery_label, mode, ws_d, ws_i, N, M, D, k, p.tiles_per_split,
                      p.n_qblocks);
    rc = ds_last_launch_error();
    if (rc) return rc;
    DS_LAUNCH(nearest_merge_kernel, ds_ceil_div(N, 4), 256, 0, stream, (const float *)ws_d, (const int *)ws_i, out_dist,
              out_index, N, k, p.n_splits);
    return ds_last_launch_error();
}

extern "C" int ds_nearest_rescore_f32(const float *queries, const float *gallery, const long long *index,
                                      float *out_dist, long long *out_index, int N, int M, int D, int k, void *stream) {
    DS_REQUIRE(queries && gallery && index && out_dist && out_index, DS_ERR_NULL);
    DS_REQUIRE(index != out_index, DS_ERR_UNSUPPORTED);    // the order changes: not in place
    DS_REQUIRE(nearest_shape_ok(N, M, D, k, 0), DS_ERR_BAD_SHAPE);
    const float eps = (float)(1e-4 / (double)D);           // PairwiseDistance's (ds_pairwise_distance_f32)
    DS_LAUNCH(nearest_rescore_kernel, ds_ceil_div(N, 4), 256, 2 * 256 * 4, stream, queries, gallery, index, out_dist,
              out_index, N, D, k, eps);
    return ds_last_launch_error();
}

extern "C" int ds_segment_mean_rows_f32(const float *emb, const long long *offsets, float *models, int S, int D,
                                        int renorm, float alpha, float eps, void *stream) {
    DS_REQUIRE(emb && offsets && models, DS_ERR_NULL);
    DS_REQUIRE(S > 0 && D > 0, DS_ERR_BAD_SHAPE);
    DS_LAUNCH(segment_mean_rows_kernel, ds_ceil_div(S, 4), 256, 0, stream, emb, offsets, models, S, D, renorm, alpha, eps);
    return ds_last_launch_error();
}

extern "C" int ds_rank_hits_i32(const long long *index, const long long *gallery_label, const long long *query_label,
                                int *hits, int N, int k, void *stream) {
    DS_REQUIRE(index && gallery_label && query_label && hits, DS_ERR_NULL);
    DS_REQUIRE(N > 0 && k >= 1 && k <= DS_NEAREST_MAX_K, DS_ERR_BAD_SHAPE);
    DS_LAUNCH(rank_hits_kernel, 1, 1024, 16 * 64 * 4, stream, index, gallery_label, query_label, hits, N, k);
    return ds_last_launch_error();
}
