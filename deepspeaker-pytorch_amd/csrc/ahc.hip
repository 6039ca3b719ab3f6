// ahc.hip -- speaker diarisation: the within-recording distance matrices of a packed batch of recordings and their
// agglomerative hierarchical clustering (AHC), one recording per workgroup.
//   * ds_ahc_distances_f32: recording r has n_r rows of emb[N,D]; its n_r x n_r matrix of PairwiseDistance(2) -- direct
//     differences, row_distance.h, the bits of ds_pairwise_distance_f32 -- is written at offset sum n^2 of the packed
//     output.  A workgroup owns one TR x TR tile of the upper triangle of one recording: the tile's rows are staged in
//     LDS once, a wavefront owns one row against four at a time (row_sqdist_x4), the tile is collected in LDS and
//     written twice, as it is and transposed, so the matrix is symmetric bit for bit.  Diagonal: +inf.
//   * ds_ahc_linkage_f32: all n_r - 1 merges of a recording in one launch, in place over its matrix.  Per slot the LDS
//     holds the nearest active neighbour ABOVE the slot (index, distance) and the cluster's size (0: merged away).  A
//     step is an argmin over those n values, the update of row and column a, and a rescan of the rows whose neighbour
//     was a or b.  Every comparison is on (value, index), so the result is a property of the matrix alone.
//   * ds_ahc_cut: labels from the linkage: the leading steps at or below a threshold and / or down to a number of
//     clusters; a leaf follows `into` to its cluster's lowest member, whose rank among the roots is the label.
// The table (int64, host-built by ds_ahc_plan, csrc/ragged_tiles.h): row_off | mat_off | step_off | tile_off | tile_rec.
#include <ds_device.h>
#include "ds_common.h"
#include "ragged_tiles.h"
#include "row_distance.h"

namespace {

constexpr int AHC_ROWS = 0, AHC_MAT = 1, AHC_STEPS = 2;    // the table's columns
constexpr int DIST_THREADS = 1024;                        // 16 wavefronts share the two staged tiles
constexpr int LINK_THREADS = 512, LINK_WAVES = LINK_THREADS / 64;
constexpr int LINK_SLOTS = DS_AHC_MAX_N / LINK_THREADS;    // slots per thread of the linkage, at the cap
constexpr int CUT_THREADS = 256;
constexpr int AHC_LDS_MAX = 160 * 1024;
constexpr int NO_INDEX = 0x7FFFFFFF;                       // loses every comparison of indices
// per slot: neighbour, its distance, size; beside them two sets of per-wave partial results
constexpr int LINK_AUX_WORDS = 4 * LINK_WAVES;
static_assert((3 * DS_AHC_MAX_N + LINK_AUX_WORDS) * 4 <= 64 * 1024, "the per-slot state of the largest recording fits the LDS");

// rows per distance tile: two tiles of rows and the tile of results in LDS; 0 = D not supported
inline int ahc_tile_rows(int D) {
    if (D < 1 || D > DS_NEAREST_MAX_D) return 0;
    for (int tr = 32; tr >= 8; tr >>= 1)
        if ((2LL * tr * D + tr * (tr + 1)) * 4 <= AHC_LDS_MAX) return tr;
    return 0;
}

__global__ void __launch_bounds__(DIST_THREADS) ahc_distances_kernel(const float *emb, ragged_table<3> tb, int TR, int D,
                                                                     float eps, float *dist) {
    float *lds = ds_dynamic_lds();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = (int)tb.tile_utt()[blockIdx.x];
    const int n = (int)tb.count(AHC_ROWS, r);
    const int nt = (n + TR - 1) / TR;
    // tile (ti, tj), ti <= tj, of the upper triangle in row-major order
    int ti = 0, rem = (int)(blockIdx.x - tb.tile_off()[r]);
    while (ti < nt - 1 && rem >= nt - ti) {
        rem -= nt - ti;
        ++ti;
    }
    const int tj = ti + rem < nt ? ti + rem : nt - 1;
    const bool diag = ti == tj;
    const int i0 = ti * TR, j0 = tj * TR;
    const int ri = n - i0 < TR ? n - i0 : TR, rj = n - j0 < TR ? n - j0 : TR;
    const int SP = TR + 1;
    float *A = lds;                                        // [TR][D] rows i0 ..
    float *B = diag ? lds : lds + TR * D;                  // [TR][D] rows j0 ..
    float *res = lds + 2 * TR * D;                         // [TR][SP]
    const long long row0 = tb.col(AHC_ROWS)[r];
    auto stage = [&](float *dst, const float *src, int count) {        // 16 bytes per lane where the rows allow it
        if ((D & 3) == 0 && ((uintptr_t)src & 15u) == 0) {
            for (int e = tid; e < count / 4; e += DIST_THREADS) ((f32x4 *)dst)[e] = ((const f32x4 *)src)[e];
        } else {
            for (int e = tid; e < count; e += DIST_THREADS) dst[e] = src[e];
        }
    };
    stage(A, emb + (row0 + i0) * D, ri * D);
    if (!diag) stage(B, emb + (row0 + j0) * D, rj * D);
    __syncthreads();
    // wave w: rows w, w + 16, ... of the i tile against the j tile, four rows at a time (a short last group repeats
    // its last row); on the diagonal tile only the groups that reach beyond the row itself
    for (int i = wave; i < ri; i += DIST_THREADS / 64) {
        for (int j = diag ? ((i + 1) & ~3) : 0; j < rj; j += 4) {
            const int c0 = j, c1 = j + 1 < rj ? j + 1 : rj - 1, c2 = j + 2 < rj ? j + 2 : rj - 1,
                      c3 = j + 3 < rj ? j + 3 : rj - 1;
            const float s = row_sqdist_x4(A + i * D, B + c0 * D, B + c1 * D, B + c2 * D, B + c3 * D, D, lane);
            const int slot = j + ((lane >> 5) & 1) + 2 * ((lane >> 4) & 1);    // the pair this lane's quarter holds
            if ((lane & 15) == 0 && slot < rj) res[i * SP + slot] = sqrtf(s + eps);
        }
    }
    __syncthreads();
    float *out = dist + tb.col(AHC_MAT)[r];
    for (int e = tid; e < TR * TR; e += DIST_THREADS) {
        const int p = e / TR, q = e - p * TR;
        if (diag) {
            if (p < ri && q < ri)
                out[(size_t)(i0 + p) * n + i0 + q] = p == q ? __builtin_inff() : (p < q ? res[p * SP + q] : res[q * SP + p]);
        } else {
            if (p < ri && q < rj) out[(size_t)(i0 + p) * n + j0 + q] = res[p * SP + q];
            if (p < rj && q < ri) out[(size_t)(j0 + p) * n + i0 + q] = res[q * SP + p];      // the transposed tile
        }
    }
}

// (v, i) before (bv, bi): the smaller value, then the smaller index.  Written so that an index always beats NO_INDEX,
// whatever the values (a NaN never leaves a search without a result).
__device__ __forceinline__ bool ahc_before(float v, int i, float bv, int bi) { return v < bv || (!(v > bv) && i < bi); }

__device__ __forceinline__ void ahc_wave_best(float &v, int &i) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = ds_shfl_xor(v, m);
        const int oi = ds_shfl_xor_i(i, m);
        if (ahc_before(ov, oi, v, i)) {
            v = ov;
            i = oi;
        }
    }
}

// the best (v, i) of the workgroup, on every thread; wv / wi [LINK_WAVES] are scratch that the caller does not reuse
// before another barrier
__device__ __forceinline__ void ahc_block_best(float &v, int &i, float *wv, int *wi) {
    ahc_wave_best(v, i);
    if ((threadIdx.x & 63) == 0) {
        wv[threadIdx.x >> 6] = v;
        wi[threadIdx.x >> 6] = i;
    }
    __syncthreads();
    v = wv[0];
    i = wi[0];
#pragma unroll
    for (int w = 1; w < LINK_WAVES; ++w)
        if (ahc_before(wv[w], wi[w], v, i)) {
            v = wv[w];
            i = wi[w];
        }
}

// The distance of the merged cluster (n_a + n_b members) to another from the two old distances.  Average: every
// product, the sum and the division rounded to f32 on their own (no fused multiply-add): NumPy's float32 arithmetic.
__device__ __forceinline__ float ahc_merge(int method, float x, float y, float fa, float fb, float fab) {
#pragma clang fp contract(off)
    if (method == DS_AHC_SINGLE) return fminf(x, y);
    if (method == DS_AHC_COMPLETE) return fmaxf(x, y);
    const float pa = fa * x;
    const float pb = fb * y;
    const float sum = pa + pb;
    return sum / fab;
}

// one wavefront: the nearest active slot above k (not `skip`), by (distance, index), into nn / nd.  Eight loads of the
// row are in flight per lane: one at a time, every 64 entries cost a trip to L2 or HBM.
__device__ __forceinline__ void ahc_rescan(const float *M, int n, int k, int skip, const int *sz, int *nn, float *nd,
                                           int lane) {
    const float *row = M + (size_t)k * n;
    float bv = __builtin_inff();
    int bi = NO_INDEX;
    for (int j0 = k + 1 + lane; j0 < n; j0 += 8 * 64) {
        float v[8];
        unsigned live = 0u;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = j0 + 64 * u;
            const bool ok = j < n && j != skip && sz[j] != 0;
            v[u] = ok ? row[j] : 0.f;
            live |= ok ? 1u << u : 0u;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (((live >> u) & 1u) && ahc_before(v[u], j0 + 64 * u, bv, bi)) {
                bv = v[u];
                bi = j0 + 64 * u;
            }
    }
    ahc_wave_best(bv, bi);
    if (lane == 0) {
        nn[k] = bi == NO_INDEX ? -1 : bi;
        nd[k] = bv;
    }
}

__global__ void __launch_bounds__(LINK_THREADS) ahc_linkage_kernel(float *dist, ragged_table<3> tb, int n_max, int method,
                                                                   int *pair, float *height, int *size_out, int *into,
                                                                   int *step_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x;
    const int n = (int)tb.count(AHC_ROWS, r);
    if (n > n_max) return;                                 // (the entry sized the LDS for n_max)
    int *nn = (int *)ds_dynamic_lds();                     // [n_max] nearest active slot above, -1: none
    float *nd = (float *)(nn + n_max);                     // [n_max] its distance
    int *sz = (int *)(nd + n_max);                         // [n_max] members, 0: merged away
    float *wv = (float *)(sz + n_max);                     // [2][LINK_WAVES]
    int *wi = (int *)(wv + 2 * LINK_WAVES);                // [2][LINK_WAVES]
    float *M = dist + tb.col(AHC_MAT)[r];
    const long long row0 = tb.col(AHC_ROWS)[r], s0 = tb.col(AHC_STEPS)[r];

    for (int i = tid; i < n; i += LINK_THREADS) {
        into[row0 + i] = -1;
        step_out[row0 + i] = -1;
        sz[i] = 1;
    }
    __syncthreads();
    for (int k = wave; k < n; k += LINK_WAVES) ahc_rescan(M, n, k, -1, sz, nn, nd, lane);
    __syncthreads();

    for (int s = 0; s < n - 1; ++s) {
        // ---- the pair: the slot with the smallest neighbour distance, ties to the lowest slot; its neighbour is the
        // lowest of the slots above it at that distance
        float bv = __builtin_inff();
        int bi = NO_INDEX;
        for (int i = tid; i < n; i += LINK_THREADS)
            if (sz[i] > 0 && nn[i] >= 0 && ahc_before(nd[i], i, bv, bi)) {
                bv = nd[i];
                bi = i;
            }
        ahc_block_best(bv, bi, wv, wi);
        const int a = bi;
        if (a >= n) return;                                // (cannot happen: the lowest active slot has a neighbour)
        const int b = nn[a];
        const int na = sz[a], nb = sz[b];
        if (tid == 0) {
            pair[2 * (s0 + s)] = a;
            pair[2 * (s0 + s) + 1] = b;
            height[s0 + s] = bv;
            size_out[s0 + s] = na + nb;
            into[row0 + b] = a;
            step_out[row0 + b] = s;
        }
        // ---- row and column a; the neighbours that the update itself settles
        const float fa = (float)na, fb = (float)nb, fab = (float)(na + nb);
        float *Ma = M + (size_t)a * n;
        const float *Mb = M + (size_t)b * n;
        float cv = __builtin_inff();                       // slot a's new neighbour
        int ci = NO_INDEX;
        unsigned flags = 0u;                               // bit it: the row of this thread's it-th slot is searched again
        float xs[LINK_SLOTS], ys[LINK_SLOTS];               // rows a and b: every load before the first store
        unsigned live = 0u;
#pragma unroll
        for (int it = 0; it < LINK_SLOTS; ++it) {
            const int k = tid + it * LINK_THREADS;
            const bool ok = k < n && k != a && k != b && sz[k] != 0;
            xs[it] = ok ? Ma[k] : 0.f;
            ys[it] = ok ? Mb[k] : 0.f;
            live |= ok ? 1u << it : 0u;
        }
#pragma unroll
        for (int it = 0; it < LINK_SLOTS; ++it) {
            const int k = tid + it * LINK_THREADS;
            if (!((live >> it) & 1u)) continue;
            const float v = ahc_merge(method, xs[it], ys[it], fa, fb, fab);
            Ma[k] = v;
            M[(size_t)k * n + a] = v;
            if (k > a) {
                if (ahc_before(v, k, cv, ci)) {
                    cv = v;
                    ci = k;
                }
                if (k < b && nn[k] == b) flags |= 1u << it;
            } else {
                const int q = nn[k];
                if (q == a || q == b) {
                    flags |= 1u << it;
                } else if (ahc_before(v, a, nd[k], q)) {
                    nn[k] = a;
                    nd[k] = v;
                }
            }
        }
        ahc_block_best(cv, ci, wv + LINK_WAVES, wi + LINK_WAVES);      // (its barrier publishes row and column a)
        if (tid == 0) {
            nn[a] = ci == NO_INDEX ? -1 : ci;
            nd[a] = cv;
            sz[a] = na + nb;
            sz[b] = 0;                                     // (the searches below leave b out by its index)
        }
        // ---- the rows whose neighbour was a or b, each by the wavefront that owns the slot
        for (int it = 0; it * LINK_THREADS < n; ++it) {
            unsigned long long m = ds_ballot((flags >> it) & 1u);
            while (m) {
                const int k = it * LINK_THREADS + wave * 64 + __builtin_ctzll(m);
                m &= m - 1ull;
                ahc_rescan(M, n, k, b, sz, nn, nd, lane);
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int ahc_block_min_i(int v, int *wmin) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int o = ds_shfl_xor_i(v, m);
        v = o < v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = v;
    __syncthreads();
    v = wmin[0];
    for (int w = 1; w < CUT_THREADS / 64; ++w) v = wmin[w] < v ? wmin[w] : v;
    return v;
}

__global__ void __launch_bounds__(CUT_THREADS) ahc_cut_kernel(ragged_table<3> tb, int n_max, const float *height,
                                                              const int *into, const int *step, const float *thr_vec,
                                                              float thr, int thr_mode, const int *ncl_vec, int ncl,
                                                              int ncl_mode, int *labels, int *n_found) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x;
    const int n = (int)tb.count(AHC_ROWS, r);
    if (n > n_max) return;
    if (n == 0) {
        if (tid == 0) n_found[r] = 0;
        return;
    }
    int *root = (int *)ds_dynamic_lds();                   // [n_max] the leaf's root
    int *rank = root + n_max;                              // [n_max] a root's rank among the roots
    int *ctab = rank + n_max;                              // [n_max / 64 + 1] roots per 64-slot chunk, then their prefix
    int *wmin = ctab + n_max / 64 + 1;                     // [CUT_THREADS / 64]
    const long long row0 = tb.col(AHC_ROWS)[r], s0 = tb.col(AHC_STEPS)[r];

    // ---- M: the leading steps at or below the threshold (the prefix rule), at most n - n_clusters
    int first = n - 1;
    if (thr_mode != 0) {
        const float t = thr_mode == 2 ? thr_vec[r] : thr;
        for (int s = tid; s < n - 1; s += CUT_THREADS)
            if (!(height[s0 + s] <= t)) {
                first = s;
                break;
            }
    }
    int M = ahc_block_min_i(first, wmin);
    if (ncl_mode != 0) {
        const int c = ncl_mode == 2 ? ncl_vec[r] : ncl;
        const int lim = c >= n ? 0 : (c >= 1 ? n - c : n - 1);
        M = M < lim ? M : lim;
    }
    // ---- a leaf follows `into` while the step that absorbed the slot is among the first M (steps rise along the way)
    for (int i = tid; i < n; i += CUT_THREADS) {
        int q = i;
        for (int hop = 0; hop < n; ++hop) {
            const int st = step[row0 + q];
            if (st < 0 || st >= M) break;
            const int up = into[row0 + q];
            if (up < 0 || up >= n) break;
            q = up;
        }
        root[i] = q;
    }
    __syncthreads();
    // ---- the rank of every root among the roots, in index order
    const int n_chunks = (n + 63) / 64;
    for (int c = wave; c < n_chunks; c += CUT_THREADS / 64) {
        const int i = c * 64 + lane;
        const unsigned long long bal = ds_ballot(i < n && root[i] == i);
        if (lane == 0) ctab[c] = __popcll(bal);
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int c = 0; c < n_chunks; ++c) {
            const int t = ctab[c];
            ctab[c] = run;
            run += t;
        }
        n_found[r] = run;
    }
    __syncthreads();
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int c = wave; c < n_chunks; c += CUT_THREADS / 64) {
        const int i = c * 64 + lane;
        const bool is_root = i < n && root[i] == i;
        const unsigned long long bal = ds_ballot(is_root);
        if (is_root) rank[i] = ctab[c] + __popcll(bal & lt);
    }
    __syncthreads();
    for (int i = tid; i < n; i += CUT_THREADS) labels[row0 + i] = rank[root[i]];
}

}  // namespace

extern "C" int ds_ahc_plan(const long long *row_off, int n_rec, int D, long long *table, long long *counts) {
    DS_REQUIRE(row_off && counts, DS_ERR_NULL);
    const int tr = ahc_tile_rows(D);
    DS_REQUIRE(n_rec > 0 && tr > 0 && row_off[0] == 0, DS_ERR_BAD_SHAPE);
    ragged_plan<3> plan{table, n_rec};
    long long n_max = 0;
    for (int u = 0; u < n_rec; ++u) {
        const long long n = row_off[u + 1] - row_off[u];
        DS_REQUIRE(n >= 0 && n <= DS_AHC_MAX_N, DS_ERR_BAD_SHAPE);
        const long long nt = (n + tr - 1) / tr;
        plan.add(u, {n, n * n, n > 0 ? n - 1 : 0}, nt * (nt + 1) / 2);
        DS_REQUIRE(plan.tiles < (1LL << 31) && plan.total[AHC_ROWS] < (1LL << 31), DS_ERR_BAD_SHAPE);
        n_max = n > n_max ? n : n_max;
    }
    plan.finish();
    counts[0] = plan.total[AHC_ROWS];
    counts[1] = plan.tiles;
    counts[2] = tr;
    counts[3] = plan.total[AHC_MAT];
    counts[4] = plan.total[AHC_STEPS];
    counts[5] = n_max;
    return 0;
}

extern "C" long long ds_ahc_workspace_bytes(const long long *row_off, int n_rec) {
    if (!row_off || n_rec <= 0 || row_off[0] != 0) return DS_ERR_BAD_SHAPE;
    long long entries = 0;
    for (int u = 0; u < n_rec; ++u) {
        const long long n = row_off[u + 1] - row_off[u];
        if (n < 0 || n > DS_AHC_MAX_N) return DS_ERR_BAD_SHAPE;
        entries += n * n;
    }
    return (entries * 4 + 15) & ~15LL;
}

extern "C" int ds_ahc_distances_f32(const float *emb, const long long *table, int n_rec, int n_tiles, int tile_rows, int D,
                                    float *dist, void *stream) {
    DS_REQUIRE(table, DS_ERR_NULL);
    DS_REQUIRE(n_rec > 0 && n_tiles >= 0 && ahc_tile_rows(D) > 0 && tile_rows == ahc_tile_rows(D), DS_ERR_BAD_SHAPE);
    if (n_tiles == 0) return 0;                            // no recording has a row
    DS_REQUIRE(emb && dist, DS_ERR_NULL);
    const float eps = (float)(1e-4 / (double)D);           // PairwiseDistance's (ds_pairwise_distance_f32)
    const size_t lds = ((size_t)2 * tile_rows * D + (size_t)tile_rows * (tile_rows + 1)) * 4;
    DS_LAUNCH_BIG_LDS(ahc_distances_kernel, n_tiles, DIST_THREADS, lds, stream, emb, ragged_table<3>{table, n_rec}, tile_rows,
                      D, eps, dist);
    return ds_last_launch_error();
}

extern "C" int ds_ahc_linkage_f32(float *dist, const long long *table, int n_rec, int n_max, int method, int *pair,
                                  float *height, int *size, int *into, int *step, void *stream) {
    DS_REQUIRE(table, DS_ERR_NULL);
    DS_REQUIRE(method == DS_AHC_AVERAGE || method == DS_AHC_COMPLETE || method == DS_AHC_SINGLE, DS_ERR_UNSUPPORTED);
    DS_REQUIRE(n_rec > 0 && n_max >= 0 && n_max <= DS_AHC_MAX_N, DS_ERR_BAD_SHAPE);
    if (n_max == 0) return 0;
    DS_REQUIRE(into && step && (n_max < 2 || (dist && pair && height && size)), DS_ERR_NULL);
    const size_t lds = ((size_t)3 * n_max + LINK_AUX_WORDS) * 4;
    DS_LAUNCH(ahc_linkage_kernel, n_rec, LINK_THREADS, lds, stream, dist, ragged_table<3>{table, n_rec}, n_max, method, pair,
              height, size, into, step);
    return ds_last_launch_error();
}

extern "C" int ds_ahc_cut(const long long *table, int n_rec, int n_max, const float *height, const int *into,
                          const int *step, const float *threshold_vec, float threshold, int threshold_mode,
                          const int *n_clusters_vec, int n_clusters, int n_clusters_mode, int *labels, int *n_found,
                          void *stream) {
    DS_REQUIRE(table && n_found, DS_ERR_NULL);
    DS_REQUIRE(n_rec > 0 && n_max >= 0 && n_max <= DS_AHC_MAX_N, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(threshold_mode >= 0 && threshold_mode <= 2 && n_clusters_mode >= 0 && n_clusters_mode <= 2 &&
                   (threshold_mode != 0 || n_clusters_mode != 0),
               DS_ERR_UNSUPPORTED);
    DS_REQUIRE((threshold_mode != 2 || threshold_vec) && (n_clusters_mode != 2 || n_clusters_vec), DS_ERR_NULL);
    DS_REQUIRE(threshold_mode == 2 || threshold == threshold, DS_ERR_BAD_SHAPE);        // a NaN threshold
    DS_REQUIRE(n_clusters_mode != 1 || n_clusters >= 1, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(n_max == 0 || (into && step && labels && (n_max < 2 || height)), DS_ERR_NULL);
    const size_t lds = ((size_t)2 * n_max + n_max / 64 + 1 + CUT_THREADS / 64) * 4;
    DS_LAUNCH(ahc_cut_kernel, n_rec, CUT_THREADS, lds, stream, ragged_table<3>{table, n_rec}, n_max, height, into, step,
              threshold_vec, threshold, threshold_mode, n_clusters_vec, n_clusters, n_clusters_mode, labels, n_found);
    return ds_last_launch_error();
}
