// screen_tile.h -- the screening distance of a block of query rows against a tile of gallery rows,
//     s(q, g) = (|q|^2 + |g|^2) - 2 q.g,    q.g from v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulation),
// shared by the two searches that select rows by it: the k-list search of identify.hip and the radix select of
// score_norm.hip.  Both run this one function, so a pair has ONE screening value: its bits depend on the pair alone,
// not on the kernel, the tile the pair falls in, the batch or the other rows.
#pragma once
#include <ds_device.h>
#include "row_distance.h"

namespace {

constexpr int NQ = 64;              // queries per workgroup
constexpr int NG = 128;             // gallery rows per tile: 32 per wave
constexpr int KC = 32;              // dimensions per staged chunk
constexpr int KP = KC + 4;          // row pitch of the staged chunk in floats (16-byte aligned, conflict-free b128 reads)
constexpr int SP = NG + 4;          // row pitch of the screening tile
constexpr int STAGE_FLOATS = (NQ + NG) * KP;
constexpr int TILE_FLOATS = NQ * SP > STAGE_FLOATS ? NQ * SP : STAGE_FLOATS;      // the two alias each other
constexpr int SLOTS = (NQ + NG) * (KC / 4) / 256;                                 // float4 per thread and chunk

// norms[r] = sum_k x[r,k]^2: one wavefront per row, lane l sums dimensions l, l + 64, ... in order, then the butterfly.
// The value of a row depends on nothing but the row.
__global__ void __launch_bounds__(256) row_sqnorm_kernel(const float *q, const float *g, float *qn, float *gn, int N,
                                                         int M, int D) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = row < N + M;
    const float *src = !live ? q : row < N ? q + (size_t)row * D : g + (size_t)(row - N) * D;
    float ss = 0.f;
    for (int k = lane; k < D; k += 64) {
        const float v = src[k];
        ss = __builtin_fmaf(v, v, ss);
    }
    ss = wave_sum(ss);
    if (live && lane == 0) {
        if (row < N) qn[row] = ss;
        else gn[row - N] = ss;
    }
}

// This thread's float4 pieces of one KC-dimension chunk of the NQ query rows from q0 and the NG gallery rows of `tile`,
// into registers (rows past N / M and dimensions past D are zeros).
__device__ __forceinline__ void screen_fetch(f32x4 (&pre)[SLOTS], const float *q, const float *g, int q0, int tile, int k0,
                                             int N, int M, int D, int tid) {
#pragma unroll
    for (int it = 0; it < SLOTS; ++it) {
        const int i = tid + it * 256;
        const int row = i / (KC / 4), c = i - row * (KC / 4);
        const int kk = k0 + c * 4;
        pre[it] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (kk < D) {
            if (row < NQ) {
                if (q0 + row < N) pre[it] = *(const f32x4 *)(q + (size_t)(q0 + row) * D + kk);
            } else {
                const long long j = (long long)tile * NG + (row - NQ);
                if (j < M) pre[it] = *(const f32x4 *)(g + (size_t)j * D + kk);
            }
        }
    }
}

// The screening values of the workgroup's NQ queries against gallery tile `tile`, left in LDS as stage[NQ][SP].
//   `pre` holds the tile's first chunk on entry (screen_fetch) and the first chunk of `next_tile` on return
//   (next_tile < 0: nothing more to fetch).
//   GEMM: wave w owns gallery rows 32 w .. 32 w + 31 of the tile and both 32-query halves (two 32x32 accumulators).  A
//   chunk of KC dimensions of the 64 + 128 rows is staged through LDS (next chunk prefetched into registers); a lane
//   reads 4 consecutive dimensions of its row with one b128 and feeds them to 4 MFMAs, so the dimensions of a pair are
//   always accumulated in the same order (per 8: 0, 4, 1, 5, 2, 6, 3, 7) -- wherever the pair falls.
//   `first_chunk()` runs between the two barriers of the first chunk: the caller loads what it keeps per tile (the
//   tile's norms into gn_s[NG], labels) there -- the last readers of the previous tile's are behind the first barrier.
//   qn_s[NQ] holds the queries' norms.  The function ends with a barrier: the tile is readable by every thread.
template <class FirstChunk>
__device__ __forceinline__ void screen_tile(float *stage, f32x4 (&pre)[SLOTS], const float *q, const float *g,
                                            const float *qn_s, const float *gn_s, int q0, int tile, int next_tile, int N,
                                            int M, int D, FirstChunk &&first_chunk) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_chunks = (D + KC - 1) / KC;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
    for (int ch = 0; ch < n_chunks; ++ch) {
        __syncthreads();                               // the previous chunk (or the previous tile's readers) is done
#pragma unroll
        for (int it = 0; it < SLOTS; ++it) {
            const int i = tid + it * 256;
            const int row = i / (KC / 4), c = i - row * (KC / 4);
            *(f32x4 *)(stage + row * KP + c * 4) = pre[it];
        }
        if (ch == 0) first_chunk();
        __syncthreads();
        if (ch + 1 < n_chunks) screen_fetch(pre, q, g, q0, tile, (ch + 1) * KC, N, M, D, tid);
        else if (next_tile >= 0) screen_fetch(pre, q, g, q0, next_tile, 0, N, M, D, tid);
        const float *qa = stage + (lane & 31) * KP + 4 * (lane >> 5);
        const float *ga = stage + (NQ + 32 * wave + (lane & 31)) * KP + 4 * (lane >> 5);
#pragma unroll
        for (int st = 0; st < KC / 8; ++st) {
            const f32x4 a0 = *(const f32x4 *)(qa + 8 * st);
            const f32x4 a1 = *(const f32x4 *)(qa + 32 * KP + 8 * st);
            const f32x4 b = *(const f32x4 *)(ga + 8 * st);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc0 = ds_mfma_32x32x2_f32(a0[u], b[u], acc0);
                acc1 = ds_mfma_32x32x2_f32(a1[u], b[u], acc1);
            }
        }
    }
    __syncthreads();                                   // every wave is done with the staged rows
    {
        const int col = 32 * wave + (lane & 31);
        const float gnj = gn_s[col];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            stage[row * SP + col] = __builtin_fmaf(-2.0f, acc0[r], qn_s[row] + gnj);
            stage[(row + 32) * SP + col] = __builtin_fmaf(-2.0f, acc1[r], qn_s[row + 32] + gnj);
        }
    }
    __syncthreads();
}

}  // namespace
