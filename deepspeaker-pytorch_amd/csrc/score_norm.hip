// score_norm.hip -- score normalisation (Z / T / S / AS-norm): the statistics of every embedding's distances to a cohort
// of impostor embeddings, over all cohort rows or over the K closest, and their application to trial scores.
//   * ds_cohort_stats_f32: for every row of emb[N,D] the min(K, eligible) cohort[M,D] rows with the smallest screening
//     value s(q, g) = (|q|^2 + |g|^2) - 2 q.g -- screen_tile.h, the SAME function and therefore the same bits as the
//     k-list search of identify.hip -- and the mean and population standard deviation of the DISTANCES to those rows.
//       cohort_screen_kernel  the screening values of a block of `row_block` rows, [row_block x M] in the workspace; the
//                             N x M matrix never exists.
//       cohort_select_kernel  one workgroup per row: the row's M values as order-preserving 32-bit keys in LDS, the K-th
//                             smallest key by an exact radix select (eight 4-bit digits, most significant first; every
//                             thread counts its keys' digits in registers and the counts are added in a fixed order: no
//                             atomics), the selection (key < K-th, plus the first K - count_less rows, in index order,
//                             of those equal to it), the selected rows' distances again by direct differences in
//                             PairwiseDistance's arithmetic (row_distance.h) and their two-pass mean / deviation in a
//                             fixed order over the index-ordered list.
//     The selection is ordered lexicographically by (s, cohort index), so it is a property of the row and the cohort; the
//     statistics are a property of the row and its selected set: neither depends on N, row_block or the other rows.
//   * ds_score_norm_apply_f32: out = ((raw - mean_a) / sd_a + (raw - mean_b) / sd_b) / 2, or one side alone.
#include <ds_device.h>
#include "ds_common.h"
#include "row_distance.h"
#include "screen_tile.h"

namespace {

constexpr int MAX_CHUNKS = DS_COHORT_MAX_M / 64;           // 64-row chunks of a cohort: one ballot each
constexpr unsigned KEY_INELIGIBLE = 0xFFFFFFFFu;
// bytes of LDS beside the keys: digit counters [256][4], wave counts [2][4][16], chunk tables 2 x [MAX_CHUNKS], the
// selection bits [2 MAX_CHUNKS], scan scratch [256 + 4], wave sums [4]
constexpr int SEL_AUX_WORDS = 256 * 4 + 2 * 4 * 16 + 2 * MAX_CHUNKS + 2 * MAX_CHUNKS + 256 + 4 + 4;
static_assert((DS_COHORT_MAX_M + SEL_AUX_WORDS) * 4 <= 160 * 1024, "the keys of the largest cohort fit the LDS");

// The screening values of rows [r0, r1) against every cohort row: workgroup (qb, split) owns NQ rows from r0 + NQ qb and
// the cohort tiles of its split, and copies each finished tile from LDS to ws_s[(row - r0) * Mp + j] (Mp: M rounded up to
// 4, so that the b128 stores stay aligned and inside the row).
__global__ void __launch_bounds__(256) cohort_screen_kernel(const float *q, const float *g, const float *qn,
                                                            const float *gn, float *ws_s, int r0, int r1, int M, int Mp,
                                                            int D, int tiles_per_split, int n_qblocks) {
    float *lds = ds_dynamic_lds();
    float *stage = lds;                                    // [NQ + NG][KP], later [NQ][SP]
    float *gn_s = lds + TILE_FLOATS;                       // [NG]
    float *qn_s = gn_s + NG;                               // [NQ]
    const int tid = threadIdx.x;
    const int qb = blockIdx.x % n_qblocks, split = blockIdx.x / n_qblocks;
    const int q0 = r0 + qb * NQ;
    const int n_tiles = (M + NG - 1) / NG;
    const int tile0 = split * tiles_per_split;
    const int tile1 = tile0 + tiles_per_split < n_tiles ? tile0 + tiles_per_split : n_tiles;
    if (tid < NQ) qn_s[tid] = q0 + tid < r1 ? qn[q0 + tid] : 0.f;
    f32x4 pre[SLOTS];
    if (tile0 < tile1) screen_fetch(pre, q, g, q0, tile0, 0, r1, M, D, tid);
    for (int tile = tile0; tile < tile1; ++tile) {
        const int j0 = tile * NG;
        screen_tile(stage, pre, q, g, qn_s, gn_s, q0, tile, tile + 1 < tile1 ? tile + 1 : -1, r1, M, D, [&]() {
            if (tid < NG) gn_s[tid] = j0 + tid < M ? gn[j0 + tid] : 0.f;
        });
#pragma unroll
        for (int it = 0; it < NQ * NG / 4 / 256; ++it) {
            const int e = tid + it * 256;
            const int row = e / (NG / 4), c = (e - row * (NG / 4)) * 4;
            if (q0 + row < r1 && j0 + c < M)
                *(f32x4 *)(ws_s + (size_t)(q0 - r0 + row) * Mp + j0 + c) = *(const f32x4 *)(stage + row * SP + c);
        }
    }
}

// float -> unsigned with the same order (negative values, which cancellation produces for near-duplicate rows, below
// the positive ones; -0 and +0 one key, as they are one value for the k-list search's comparison).  The largest key
// is kept for ineligible rows: only a NaN could have taken it.
__device__ __forceinline__ unsigned order_key(float s) {
    unsigned b = __builtin_bit_cast(unsigned, s);
    if (s == 0.f) b = 0u;
    const unsigned k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return k < KEY_INELIGIBLE - 1u ? k : KEY_INELIGIBLE - 1u;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += ds_shfl_xor_i(v, m);
    return v;
}

// sum of v over the workgroup's 256 threads, the waves' sums added in wave order; wsum[4] is scratch
__device__ __forceinline__ int block_sum_i(int v, int *wsum) {
    v = wave_sum_i(v);
    __syncthreads();                                       // the previous readers of wsum are done
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    return wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
__device__ __forceinline__ float block_sum_f(float v, float *wsum) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// number of v's on the threads below this one; tmp[256 + 4] is scratch (free again on return)
__device__ __forceinline__ int block_exclusive_scan(int v, int *tmp) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    tmp[tid] = v;
    ds_wave_sync();
    int p = 0;
    for (int i = 0; i < lane; ++i) p += tmp[wave * 64 + i];
    if (lane == 63) tmp[256 + wave] = p + v;
    __syncthreads();
    for (int w = 0; w < wave; ++w) p += tmp[256 + w];
    __syncthreads();
    return p;
}

// in place: tab[c] <- tab[0] + ... + tab[c - 1] for the n <= 2 * 256 entries of a chunk table (thread t owns 2t, 2t + 1)
__device__ __forceinline__ void chunk_table_scan(int *tab, int n, int *tmp) {
    const int c = 2 * threadIdx.x;
    const int a = c < n ? tab[c] : 0, b = c + 1 < n ? tab[c + 1] : 0;
    const int p = block_exclusive_scan(a + b, tmp);        // (its barriers are behind every thread's reads above)
    if (c < n) tab[c] = p;
    if (c + 1 < n) tab[c + 1] = p + a;
    __syncthreads();
}

__global__ void __launch_bounds__(256) cohort_select_kernel(const float *emb, const float *cohort, const float *ws_s,
                                                            const long long *elab, const long long *clab, int mode,
                                                            float *mean, float *stdv, int *count, int *selected, int r0,
                                                            int M, int Mp, int D, int K, int words, float eps) {
    unsigned *keys = (unsigned *)ds_dynamic_lds();         // [M rounded up to 64]; later the selected list, then its distances
    const int n_chunks = (M + 63) / 64;
    unsigned *dcnt = keys + n_chunks * 64;                 // [256][4] sixteen 8-bit digit counters per thread
    int *wcnt = (int *)(dcnt + 256 * 4);                   // [2][4][16] digit counts per wave, double-buffered by pass
    int *eq_tab = wcnt + 2 * 4 * 16;                       // [MAX_CHUNKS] keys equal to the K-th per chunk, then their prefix
    int *sel_tab = eq_tab + MAX_CHUNKS;                    // [MAX_CHUNKS] selected rows per chunk, then their prefix
    unsigned *sel_bits = (unsigned *)(sel_tab + MAX_CHUNKS);       // [2 MAX_CHUNKS] the selection, bit j of word j / 32
    int *scan_tmp = (int *)(sel_bits + 2 * MAX_CHUNKS);    // [256 + 4]
    int *wsum = scan_tmp + 256 + 4;                        // [4]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = r0 + blockIdx.x;
    const float *srow = ws_s + (size_t)blockIdx.x * Mp;
    const long long my_lab = mode != 0 ? elab[row] : 0;

    // ---- the row's keys; E = eligible rows
    int mine = 0;
    for (int j = tid; j < M; j += 256) {
        bool ok = true;
        if (mode != 0) ok = (clab[j] == my_lab) == (mode == 2);
        keys[j] = ok ? order_key(srow[j]) : KEY_INELIGIBLE;
        mine += ok ? 1 : 0;
    }
    const int E = block_sum_i(mine, wsum);                 // (its barriers publish the keys)
    const int Ke = K < E ? K : E;
    if (Ke == 0) {
        if (selected)
            for (int w = tid; w < words; w += 256) selected[(size_t)row * words + w] = 0;
        if (tid == 0) {
            mean[row] = __builtin_inff();
            stdv[row] = 0.f;
            count[row] = 0;
        }
        return;
    }

    // ---- radix select: T = the Ke-th smallest key, need = how many of the keys equal to T belong to the selection.
    // Every eligible key is below KEY_INELIGIBLE and Ke <= E, so T is an eligible row's key.
    unsigned prefix = 0u, known = 0u;
    int need = Ke;                                         // rank (from 1) among the keys that match the prefix
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 28 - 4 * pass;
        unsigned long long lo = 0ull, hi = 0ull;           // counters of digits 0..7 / 8..15: at most 128 keys per thread
        for (int j = tid; j < M; j += 256) {
            const unsigned key = keys[j];
            if ((key & known) == prefix) {
                const unsigned d = (key >> shift) & 15u;
                if (d < 8u) lo += 1ull << (8u * d);
                else hi += 1ull << (8u * (d - 8u));
            }
        }
        dcnt[tid * 4 + 0] = (unsigned)lo;
        dcnt[tid * 4 + 1] = (unsigned)(lo >> 32);
        dcnt[tid * 4 + 2] = (unsigned)hi;
        dcnt[tid * 4 + 3] = (unsigned)(hi >> 32);
        ds_wave_sync();
        {   // lane = (part, digit): the digit's count over the part's 16 lanes (each part starts at another lane: no bank
            // is asked for two addresses), then over the four parts
            const int digit = lane & 15, part = lane >> 4;
            int s = 0;
            for (int i = 0; i < 16; ++i) {
                const int src = wave * 64 + part * 16 + ((i + 4 * part) & 15);
                s += (int)((dcnt[src * 4 + (digit >> 2)] >> (8 * (digit & 3))) & 255u);
            }
            s += ds_shfl_xor_i(s, 16);
            s += ds_shfl_xor_i(s, 32);
            if (lane < 16) wcnt[((pass & 1) * 4 + wave) * 16 + lane] = s;
        }
        __syncthreads();
        int below = 0, digit = 15;
        for (int d = 0; d < 16; ++d) {
            const int *w = wcnt + (pass & 1) * 64 + d;
            const int tot = w[0] + w[16] + w[32] + w[48];
            if (below + tot >= need) { digit = d; break; }
            below += tot;
        }
        need -= below;
        prefix |= (unsigned)digit << shift;
        known |= 15u << shift;
    }
    const unsigned T = prefix;
    const unsigned long long lt = (1ull << lane) - 1ull;

    // ---- ties at T in index order: the number of equal keys before each 64-row chunk
    for (int c = wave; c < n_chunks; c += 4) {
        const int j = c * 64 + lane;
        const unsigned long long b = ds_ballot(j < M && keys[j] == T);
        if (lane == 0) eq_tab[c] = __popcll(b);
    }
    __syncthreads();
    chunk_table_scan(eq_tab, n_chunks, scan_tmp);

    // ---- the selection: its bits, and the number of selected rows per chunk
    for (int c = wave; c < n_chunks; c += 4) {
        const int j = c * 64 + lane;
        const unsigned key = j < M ? keys[j] : KEY_INELIGIBLE;
        const bool eq = j < M && key == T;
        const unsigned long long be = ds_ballot(eq);
        const int rank = eq_tab[c] + __popcll(be & lt);
        const unsigned long long bs = ds_ballot(j < M && (key < T || (eq && rank < need)));
        if (lane == 0) {
            sel_tab[c] = __popcll(bs);
            sel_bits[2 * c] = (unsigned)bs;
            sel_bits[2 * c + 1] = (unsigned)(bs >> 32);
            if (selected) {
                if (2 * c < words) selected[(size_t)row * words + 2 * c] = (int)(unsigned)bs;
                if (2 * c + 1 < words) selected[(size_t)row * words + 2 * c + 1] = (int)(unsigned)(bs >> 32);
            }
        }
    }
    __syncthreads();                                       // the keys are dead from here on
    chunk_table_scan(sel_tab, n_chunks, scan_tmp);

    // ---- the selected rows as a list in index order, over the keys
    int *list = (int *)keys;
    for (int c = wave; c < n_chunks; c += 4) {
        const unsigned long long bs = (unsigned long long)sel_bits[2 * c] | ((unsigned long long)sel_bits[2 * c + 1] << 32);
        if ((bs >> lane) & 1ull) list[sel_tab[c] + __popcll(bs & lt)] = c * 64 + lane;
    }
    __syncthreads();

    // ---- their distances, four pairs at a time over a wave (PairwiseDistance's arithmetic), over the list: a wave
    // reads its four entries (a short last group repeats its first) before it writes any of them
    float *dist = (float *)keys;
    const float *qrow = emb + (size_t)row * D;
    for (int r = 4 * wave; r < Ke; r += 16) {
        const int j0 = list[r], j1 = list[r + 1 < Ke ? r + 1 : r], j2 = list[r + 2 < Ke ? r + 2 : r],
                  j3 = list[r + 3 < Ke ? r + 3 : r];
        const float s = row_sqdist_x4(qrow, cohort + (size_t)j0 * D, cohort + (size_t)j1 * D, cohort + (size_t)j2 * D,
                                      cohort + (size_t)j3 * D, D, lane);      // (its exchanges are behind every lane's reads)
        const int slot = r + ((lane >> 5) & 1) + 2 * ((lane >> 4) & 1);        // the pair this lane's quarter holds
        if ((lane & 15) == 0 && slot < Ke) dist[slot] = sqrtf(s + eps);
    }
    // ---- mean, then the deviations from it: thread t adds entries t, t + 256, ... in order, the lanes by butterfly,
    // the waves in wave order
    float part = 0.f;
    __syncthreads();
    for (int r = tid; r < Ke; r += 256) part += dist[r];
    const float mu = block_sum_f(part, (float *)wsum) / (float)Ke;
    part = 0.f;
    for (int r = tid; r < Ke; r += 256) {
        const float dv = dist[r] - mu;
        part += dv * dv;
    }
    const float ss = block_sum_f(part, (float *)wsum);
    if (tid == 0) {
        mean[row] = mu;
        stdv[row] = sqrtf(ss / (float)Ke);
        count[row] = Ke;
    }
}

__global__ void __launch_bounds__(256) score_norm_apply_kernel(const float *raw, const long long *ia, const long long *ib,
                                                               const float *mean_a, const float *std_a,
                                                               const float *mean_b, const float *std_b, float min_std,
                                                               float *out, int T) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const float x = raw[t];
    const long long a = ia ? ia[t] : t;
    const float za = (x - mean_a[a]) / fmaxf(std_a[a], min_std);
    if (!mean_b) {
        out[t] = za;
        return;
    }
    const long long b = ib ? ib[t] : t;
    const float zb = (x - mean_b[b]) / fmaxf(std_b[b], min_std);
    out[t] = 0.5f * (za + zb);
}

// The block of screening values that is alive between the two kernels is sized to stay in the last-level cache next
// to the cohort itself: 128 MiB of the 256 MiB on an MI355X, and at least 256 rows so that the one-workgroup-per-row
// select fills the chip.  Timed against 8 MiB and 32 MiB blocks (tools/score_norm_bench.py): a block of
// fewer rows than the chip runs workgroups costs 2-3x, 32 MiB against 128 MiB 3-10 %.
constexpr long long BLOCK_BYTES = 128ll << 20;

struct cohort_plan { int row_block, Mp; size_t off_gn, off_s, bytes; };

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

bool cohort_shape_ok(int N, int M, int D, int K, int row_block) {
    return N > 0 && N <= (1 << 30) && M > 0 && M <= DS_COHORT_MAX_M && D > 0 && D % 4 == 0 && D <= DS_NEAREST_MAX_D &&
           K >= 1 && K <= M && row_block >= 0;
}

cohort_plan plan_cohort(int N, int M, int row_block) {
    cohort_plan p;
    p.Mp = (M + 3) & ~3;
    long long rb = row_block;
    if (rb == 0) {
        rb = BLOCK_BYTES / ((long long)p.Mp * 4) / NQ * NQ;
        if (rb < 256) rb = 256;
    }
    p.row_block = rb < N ? (int)rb : N;
    p.off_gn = align16((size_t)N * 4);
    p.off_s = p.off_gn + align16((size_t)M * 4);
    p.bytes = p.off_s + align16((size_t)p.row_block * p.Mp * 4);
    return p;
}

}  // namespace

extern "C" long long ds_cohort_workspace_bytes(int N, int M, int D, int K, int row_block) {
    if (!cohort_shape_ok(N, M, D, K, row_block)) return DS_ERR_BAD_SHAPE;
    return (long long)plan_cohort(N, M, row_block).bytes;
}

extern "C" int ds_cohort_stats_f32(const float *emb, const float *cohort, const long long *emb_label,
                                   const long long *cohort_label, int mode, void *workspace, float *mean, float *std,
                                   int *count, int *selected, int N, int M, int D, int K, int row_block, void *stream) {
    DS_REQUIRE(emb && cohort && workspace && mean && std && count, DS_ERR_NULL);
    DS_REQUIRE(mode >= 0 && mode <= 2, DS_ERR_UNSUPPORTED);
    DS_REQUIRE(mode == 0 || (emb_label && cohort_label), DS_ERR_NULL);
    DS_REQUIRE(cohort_shape_ok(N, M, D, K, row_block), DS_ERR_BAD_SHAPE);
    DS_REQUIRE(DS_ALIGNED16(emb) && DS_ALIGNED16(cohort) && DS_ALIGNED16(workspace), DS_ERR_ALIGNMENT);
    const cohort_plan p = plan_cohort(N, M, row_block);
    char *ws = (char *)workspace;
    float *qn = (float *)ws, *gn = (float *)(ws + p.off_gn), *ws_s = (float *)(ws + p.off_s);
    DS_LAUNCH(row_sqnorm_kernel, (int)ds_ceil_div_ll((long long)N + M, 4), 256, 0, stream, emb, cohort, qn, gn, N, M, D);
    int rc = ds_last_launch_error();
    if (rc) return rc;
    const float eps = (float)(1e-4 / (double)D);           // PairwiseDistance's (ds_pairwise_distance_f32)
    const int n_tiles = ds_ceil_div(M, NG), n_chunks = ds_ceil_div(M, 64), words = ds_ceil_div(M, 32);
    const size_t screen_lds = ((size_t)TILE_FLOATS + NG + NQ) * 4;
    const size_t select_lds = ((size_t)n_chunks * 64 + SEL_AUX_WORDS) * 4;
    for (int r0 = 0; r0 < N; r0 += p.row_block) {
        const int r1 = r0 + p.row_block < N ? r0 + p.row_block : N;
        const int n_qblocks = ds_ceil_div(r1 - r0, NQ);
        int want = ds_ceil_div(2 * ds_cu_count(), n_qblocks);      // cohort ranges: the workgroups fill the chip twice over
        if (want > n_tiles) want = n_tiles;
        const int tiles_per_split = ds_ceil_div(n_tiles, want);
        const int n_splits = ds_ceil_div(n_tiles, tiles_per_split);
        DS_LAUNCH(cohort_screen_kernel, n_qblocks * n_splits, 256, screen_lds, stream, emb, cohort, (const float *)qn,
                  (const float *)gn, ws_s, r0, r1, M, p.Mp, D, tiles_per_split, n_qblocks);
        rc = ds_last_launch_error();
        if (rc) return rc;
        DS_LAUNCH_BIG_LDS(cohort_select_kernel, r1 - r0, 256, select_lds, stream, emb, cohort, (const float *)ws_s, emb_label,
                          cohort_label, mode, mean, std, count, selected, r0, M, p.Mp, D, K, words, eps);
        rc = ds_last_launch_error();
        if (rc) return rc;
    }
    return 0;
}

extern "C" int ds_score_norm_apply_f32(const float *raw, const long long *a_index, const long long *b_index,
                                       const float *mean_a, const float *std_a, const float *mean_b, const float *std_b,
                                       float min_std, float *out, int T, void *stream) {
    DS_REQUIRE(raw && mean_a && std_a && out, DS_ERR_NULL);
    DS_REQUIRE((mean_b == nullptr) == (std_b == nullptr), DS_ERR_NULL);
    DS_REQUIRE(T > 0, DS_ERR_BAD_SHAPE);
    DS_LAUNCH(score_norm_apply_kernel, ds_ceil_div(T, 256), 256, 0, stream, raw, a_index, b_index, mean_a, std_a, mean_b,
              std_b, min_std, out, T);
    return ds_last_launch_error();
}
