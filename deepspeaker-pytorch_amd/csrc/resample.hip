// resample.hip -- rational polyphase resampling of packed waveforms (the resampling half of the reference's
// librosa.load(filename, sr=16000, mono=True), audio_processing.py:10), with the mono down-mix and the int16 scaling:
//   y[m] = sum_k x[k] * h[H + m*M - k*L],  0 <= k < n,  0 <= H + m*M - k*L <= 2H,  n_out = ceil(n * L / M)
// h is the caller's windowed-sinc table of 2H + 1 taps (features.resample_taps: SciPy's resample_poly design), handed
// over in polyphase form: row p of [L][TP] holds the T = ceil((2H+1)/L) taps of phase p = (H + m*M) mod L in the order
// of ASCENDING input index (tap H + m*M - k*L at column k - k_first), zero where the table has no tap, TP = T | 1.
//   * ds_resample_plan: host arithmetic -- output lengths, input / output offsets, the tile table (tiles never straddle
//     utterances) and the tile size
//   * resample_poly_kernel: one workgroup per tile of RS_R * S outputs of one utterance.  The tile's input span (down-
//     mixed, scaled, zero outside the utterance) and the whole polyphase table are staged into LDS.  A thread computes
//     the RS_R outputs w, w + S, ... of the tile: S is a multiple of L, so they share one phase -- each tap is read
//     once and used RS_R times from a register -- and lanes hold consecutive outputs (coalesced stores; LDS reads of
//     the span at stride M/L, of the table at the odd row stride TP).  Every output is one fmaf chain over ascending
//     input index: deterministic, independent of tile, batch and call.  VALU / LDS / HBM work: there is no GEMM here
//     (as a Toeplitz product on the MFMA, L = 1 has one useful column and 160/441 is ~9x zero work).
#include <ds_device.h>
#include "ds_common.h"
#include "ragged_tiles.h"

namespace {

constexpr int RS_THREADS = 512;
constexpr int RS_R = 4;                          // outputs per thread item (one phase, taps shared from registers)
constexpr int RS_LDS_MAX = 96 * 1024;            // table + span of one tile
constexpr int RS_TABLE_MAX = 16384;              // polyphase table entries (L * TP): 64 KiB
constexpr int RS_MAX_CHANNELS = 8;

struct rs_geom {
    int L, M, H, T, TP, S, span;                 // S: outputs per tile row (multiple of L); tile = RS_R * S outputs
};

__host__ __device__ inline int rs_taps(int L, int H) { return (2 * H + 1 + L - 1) / L; }
// input samples one tile can touch: floor((L - 1 + (tile - 1) * M) / L) + T
__host__ __device__ inline long long rs_span(int L, int M, int T, int S) {
    return ((long long)(L - 1) + ((long long)RS_R * S - 1) * M) / L + T;
}

// the largest tile whose table and span fit the LDS budget; false = not supported
inline bool rs_geometry(int L, int M, int H, rs_geom *g) {
    if (L < 1 || M < 1 || H < 1 || L > RS_TABLE_MAX || M > (1 << 20) || H > (1 << 24)) return false;
    const int T = rs_taps(L, H), TP = T | 1;
    if ((long long)L * TP > RS_TABLE_MAX) return false;
    for (int target = 1024; target >= 32; target >>= 1) {
        const int S = L * ((target + L - 1) / L);
        const long long span = rs_span(L, M, T, S);
        if (4 * ((long long)L * TP + span) <= RS_LDS_MAX) {
            *g = rs_geom{L, M, H, T, TP, S, (int)span};
            return true;
        }
    }
    return false;
}

// frame f of interleaved [n][C] samples as mono: channels summed in order in f32, then divided by C in f32
template <typename T>
__device__ __forceinline__ float rs_mono(const T *x, long long f, int C) {
    if (C == 1) return ds_pcm<T>(x, f);
    float s = ds_pcm<T>(x, f * C);
    for (int c = 1; c < C; ++c) s += ds_pcm<T>(x, f * C + c);
    return s / (float)C;
}

// table: ragged_table<2> of (input frames, outputs), the outputs in tiles
constexpr int RS_IN = 0, RS_OUT = 1;

template <typename T>
__global__ void __launch_bounds__(RS_THREADS) resample_poly_kernel(const T *x, int C, ragged_table<2> tb,
                                                                   const float *taps, rs_geom g, float *out) {
    const int tile = blockIdx.x, t = threadIdx.x;
    const ragged_tile at = ragged_tile_of(tb, tile, RS_R * g.S);
    const int u = at.u;
    const long long s0 = tb.col(RS_IN)[u], n = tb.count(RS_IN, u);
    const long long o0 = tb.col(RS_OUT)[u], n_out = tb.count(RS_OUT, u), m0 = at.first;
    // output m0 + e reads inputs k0 + (pc + e*M) / L + [0, T) with the taps of phase (pc + e*M) % L
    const long long c0 = (long long)g.H + m0 * g.M;
    const long long k0 = c0 / g.L - g.T + 1;
    const int pc = (int)(c0 % g.L);

    float *tab = ds_dynamic_lds();                           // [L][TP]
    float *xs = tab + g.L * g.TP;                            // [span]
    const int n_tab = g.L * g.TP;
    for (int i = t; i < n_tab; i += RS_THREADS) tab[i] = taps[i];
#pragma unroll 4
    for (int s = t; s < g.span; s += RS_THREADS) {
        const long long k = k0 + s;
        xs[s] = (k >= 0 && k < n) ? rs_mono<T>(x, s0 + k, C) : 0.0f;
    }
    __syncthreads();

    const int row_step = (g.S / g.L) * g.M;                  // input distance of two outputs S apart
    const long long left = n_out - m0;                       // outputs of this utterance from the tile's first on
    for (int w = t; w < g.S; w += RS_THREADS) {
        if (w >= left) break;
        const int local = pc + w * g.M, off = local / g.L, p = local - off * g.L;
        const float *hp = tab + p * g.TP, *xp = xs + off;
        float acc[RS_R];
#pragma unroll
        for (int r = 0; r < RS_R; ++r) acc[r] = 0.0f;
        for (int j = 0; j < g.T; ++j) {
            const float h = hp[j];
#pragma unroll
            for (int r = 0; r < RS_R; ++r) acc[r] = fmaf(xp[r * row_step + j], h, acc[r]);
        }
        float *y = out + o0 + m0 + w;
#pragma unroll
        for (int r = 0; r < RS_R; ++r)
            if (w + (long long)r * g.S < left) y[r * g.S] = acc[r];
    }
}

}  // namespace

extern "C" int ds_resample_plan(const long long *lengths, int n_utt, int up, int down, int half_width, long long *table,
                                long long *counts) {
    DS_REQUIRE(lengths && counts, DS_ERR_NULL);
    DS_REQUIRE(n_utt > 0, DS_ERR_BAD_SHAPE);
    rs_geom g;
    DS_REQUIRE(rs_geometry(up, down, half_width, &g), DS_ERR_UNSUPPORTED);
    const long long tile_out = (long long)RS_R * g.S;
    ragged_plan<2> plan{table, n_utt};
    for (int u = 0; u < n_utt; ++u) {
        const long long len = lengths[u];
        DS_REQUIRE(len > 0 && len < (1LL << 40), DS_ERR_BAD_SHAPE);
        const long long no = (len * up + down - 1) / down;
        plan.add(u, {len, no}, (no + tile_out - 1) / tile_out);
        DS_REQUIRE(plan.tiles < (1LL << 31) && plan.total[RS_IN] < (1LL << 44) && plan.total[RS_OUT] < (1LL << 44),
                   DS_ERR_BAD_SHAPE);
    }
    plan.finish();
    counts[0] = plan.total[RS_OUT];
    counts[1] = plan.tiles;
    counts[2] = tile_out;
    return 0;
}

extern "C" int ds_resample_poly_f32(const void *samples, int in_int16, int channels, const long long *table, int n_utt,
                                    int n_tiles, const float *taps, int up, int down, int half_width, float *out,
                                    void *stream) {
    DS_REQUIRE(samples && table && taps && out, DS_ERR_NULL);
    DS_REQUIRE(n_utt > 0 && n_tiles > 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(in_int16 == 0 || in_int16 == 1, DS_ERR_UNSUPPORTED);
    DS_REQUIRE(channels >= 1 && channels <= RS_MAX_CHANNELS, DS_ERR_UNSUPPORTED);
    rs_geom g;
    DS_REQUIRE(rs_geometry(up, down, half_width, &g), DS_ERR_UNSUPPORTED);
    const size_t lds = 4 * ((size_t)g.L * g.TP + (size_t)g.span);
    if (in_int16)
        DS_LAUNCH_BIG_LDS(resample_poly_kernel<short>, n_tiles, RS_THREADS, lds, stream, (const short *)samples, channels,
                          ragged_table<2>{table, n_utt}, taps, g, out);
    else
        DS_LAUNCH_BIG_LDS(resample_poly_kernel<float>, n_tiles, RS_THREADS, lds, stream, (const float *)samples, channels,
                          ragged_table<2>{table, n_utt}, taps, g, out);
    return ds_last_launch_error();
}
