// augment.hip -- waveform augmentation of packed utterances: reverberation (a long FIR filter, one impulse response
// per utterance), additive noise at a signal-to-noise ratio, and the output level.  For utterance u of n samples x
// (int16 scaled by 1/32768), impulse response h of K taps with delay p, noise clips v_j:
//   r[m] = sum_k h[k] * x[m + p - k]                      0 <= m < n, 0 <= k < K, x zero outside [0, n);  r = x without h
//   s[m] = r[m] + sum_j g_j * v_j[(s_j + m) mod len_j]    g_j = sqrt(P_r / (P_vj * 10^(snr_j / 10))), 0 when a power is 0
//   y    = s * sqrt(P_x / P_s)  (level "input"; y = s when P_s = 0)   or   y = s  (level "none")
// P_* are mean squares over the utterance; P_vj is that of the whole clip, from the host.
//   * ds_augment_plan: host arithmetic -- offsets and the tile table (tiles never straddle utterances)
//   * augment_reverb_kernel: the hot path.  With m = 32a + i and the taps in blocks of 32,
//       r[32a + i] = sum_d sum_j H_d[i][j] * X[j][a - d],   H_d[i][j] = h[32d + i - j],   X[j][c] = x[32c + j + p]:
//     a tile of 32 x 128 outputs is the GEMM [32 x 32 D] . [32 D x 128] of Toeplitz blocks of h against the samples
//     folded into columns of 32, on v_mfma_f32_32x32x2_f32.  Every (tap, sample) pair appears once; only the first and
//     the last block are ragged.  One workgroup of 4 waves per tile, a wave per 32 columns.  The blocks are taken in
//     chunks of AUG_DC: a chunk's taps (in descending order, zero outside [0, K)) and its sample span (144 columns at
//     a row stride of 33, zero outside the utterance) are staged in LDS, both operands are 4-byte LDS reads at lane-
//     dependent addresses (the taps at stride 1 with the two k-slots one apart, the samples at stride 33: no bank
//     conflicts; two reads per MFMA of 64 cycles, so the loop is bound by the MFMA, not by the LDS), and the
//     chunks accumulate into the same registers in ascending order.  Every output is one fmaf chain -- blocks d
//     ascending, j ascending inside a block -- fixed by its position in its utterance: deterministic, independent of
//     tile, batch and call.  The tile leaves through LDS: coalesced stores, and the per-tile sums of x^2 and r^2 (f64,
//     one fixed order, the same for a copied and for a filtered tile) go to the caller's workspace.
//   * augment_mix_kernel: the utterance's P_r from the tiles' sums in one fixed order in f64, g_j rounded to f32 once,
//     s as one fmaf chain over j, in place; per-tile sums of s^2.
//   * augment_level_kernel: y = s * (float)sqrt(P_x / P_s), in place.
// Nothing is allocated, read back or synchronised.
#include <ds_device.h>
#include "ds_common.h"
#include "ragged_tiles.h"

namespace {

constexpr int AUG_THREADS = 256;                 // 4 waves, one 32 x 32 accumulator each
constexpr int AUG_COLS = 128;                    // columns of 32 outputs per tile
constexpr int AUG_TILE = 32 * AUG_COLS;          // outputs per tile
constexpr int AUG_DC = 17;                       // Toeplitz blocks per chunk: K = 512 taps are 16 + 1 (ragged) blocks
constexpr int AUG_KCHUNK = 32 * AUG_DC;          // taps per pass
constexpr int AUG_MAX_TAPS = 65536;
constexpr int AUG_MAX_NOISES = 8;
constexpr int AUG_XS = 33;                       // row stride of the staged sample columns
constexpr int AUG_SPAN_COLS = AUG_COLS + AUG_DC - 1;
constexpr int AUG_RED = 32;                      // floats at the base of the LDS: 16 doubles of the block reduction
constexpr int AUG_HS = AUG_KCHUNK + 32;          // staged taps of one chunk (32 DC + 31 used)
constexpr int AUG_LDS_FLOATS = AUG_RED + AUG_HS + AUG_SPAN_COLS * AUG_XS;
constexpr int AUG_WS = 3;                        // doubles per tile: sum x^2, sum r^2, sum s^2
constexpr int AUG_NT = 5;                        // int64 entries per (utterance, noise)

// the sum of v over the workgroup in one fixed order (butterfly inside a wave, then the waves in order), on every thread
__device__ __forceinline__ double aug_block_sum(double v, double *red) {
    for (int mask = 32; mask >= 1; mask >>= 1) v += ds_shfl_xor_f64(v, mask);
    const int t = threadIdx.x;
    __syncthreads();                                         // the previous use of red is over
    if ((t & 63) == 0) red[t >> 6] = v;
    __syncthreads();
    double s = red[0];
    for (int w = 1; w < AUG_THREADS / 64; ++w) s += red[w];
    return s;
}

// the utterance's sum of workspace slot `slot` over its tiles [t0, t1), one fixed order
__device__ __forceinline__ double aug_utt_sum(const double *ws, long long t0, long long t1, int slot, double *red) {
    double v = 0.0;
    for (long long i = t0 + threadIdx.x; i < t1; i += AUG_THREADS) v += ws[i * AUG_WS + slot];
    return aug_block_sum(v, red);
}

// table: ragged_table<1> of the samples, in tiles of AUG_TILE
// rir_tab (int64, device): [n_utt][3] = {offset of h in the bank, or -1; K; p}
template <typename T>
__global__ void __launch_bounds__(AUG_THREADS) augment_reverb_kernel(const T *x, ragged_table<1> tb, const float *bank,
                                                                     const long long *rir_tab, float *out, double *ws) {
    const int tile = blockIdx.x, t = threadIdx.x;
    const ragged_tile at = ragged_tile_of(tb, tile, AUG_TILE);
    const int u = at.u;
    const long long s0 = tb.col(0)[u], n = tb.count(0, u), m0 = at.first;
    const long long hoff = rir_tab ? rir_tab[3 * u] : -1;
    const bool filtered = hoff >= 0;

    float *lds = ds_dynamic_lds();
    double *red = (double *)lds;
    float *hs = lds + AUG_RED;                               // [32 DC + 31] taps of the chunk
    float *xs = hs + AUG_HS;                                 // [144][33] sample columns of the chunk; then the tile

    if (filtered) {
        const int K = (int)rir_tab[3 * u + 1], p = (int)rir_tab[3 * u + 2];
        const float *h = bank + hoff;
        // with p = 32 pd + pr the delay moves the samples, not the taps: blocks d = 0 .. (K + 30) / 32 hold every tap
        // (0 <= 32 d + i - j < K for some -31 <= i - j <= 31) whatever p is, against X[j][c] = x[32 c + j + pr], c = a + pd - d
        const int D = (K + 30) / 32 + 1, pr = p & 31;
        const long long a0 = m0 / 32 + p / 32;
        const int lane = t & 63, w = t >> 6, col = lane & 31, hi = lane >> 5;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        for (int e0 = 0; e0 < D; e0 += AUG_DC) {
            const int nb = D - e0 < AUG_DC ? D - e0 : AUG_DC, d0 = e0;
            if (e0) __syncthreads();                         // the previous chunk has been read
            const int ktop = 32 * (d0 + AUG_DC) - 1;         // the chunk's taps in DESCENDING order: hs[i] = h[ktop - i]
            for (int i = t; i < AUG_HS; i += AUG_THREADS) {
                const int k = ktop - i;
                hs[i] = (k >= 0 && k < K) ? h[k] : 0.0f;
            }
            const long long g0 = 32 * (a0 - d0 - AUG_DC + 1) + pr;     // first sample of the staged span
#pragma unroll 4
            for (int s = t; s < 32 * AUG_SPAN_COLS; s += AUG_THREADS) {
                const long long g = g0 + s;
                xs[(s >> 5) * AUG_XS + (s & 31)] = (g >= 0 && g < n) ? ds_pcm<T>(x, s0 + g) : 0.0f;
            }
            __syncthreads();
            // A[i][j] = hs[32 (DC - b) - 1 - i + j], B[j][a] = xs[(a - b + DC - 1) * 33 + j]; this lane's j = 2 jj + hi:
            // both operands walk up in j (immediate offsets) and down in b
            const float *ap = hs + AUG_KCHUNK - 1 - col + hi;
            const float *bp = xs + (32 * w + col + AUG_DC - 1) * AUG_XS + hi;
            for (int b = 0; b < nb; ++b) {
#pragma unroll
                for (int jj = 0; jj < 16; ++jj) acc = ds_mfma_32x32x2_f32(ap[2 * jj], bp[2 * jj], acc);
                ap -= 32;
                bp -= AUG_XS;
            }
        }
        __syncthreads();                                     // the last chunk has been read: xs becomes the tile
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * hi;
            xs[(32 * w + col) * AUG_XS + row] = acc[r];
        }
        __syncthreads();
    }

    const long long left = n - m0;
    double sx = 0.0, sr = 0.0;
#pragma unroll 4
    for (int m = t; m < AUG_TILE; m += AUG_THREADS) {
        if (m < left) {
            const float xv = ds_pcm<T>(x, s0 + m0 + m);
            const float rv = filtered ? xs[(m >> 5) * AUG_XS + (m & 31)] : xv;
            out[s0 + m0 + m] = rv;
            sx += (double)xv * (double)xv;
            sr += (double)rv * (double)rv;
        }
    }
    sx = aug_block_sum(sx, red);
    sr = aug_block_sum(sr, red);
    if (t == 0) {
        ws[(long long)tile * AUG_WS] = sx;
        ws[(long long)tile * AUG_WS + 1] = sr;
    }
}

// noise_tab (int64, device): [n_utt][J][5] = {offset of the clip in the bank, or -1; its length; the start in it;
// bits of its mean square (f64); bits of 10^(snr / 10) (f64)}
__global__ void __launch_bounds__(AUG_THREADS) augment_mix_kernel(float *data, ragged_table<1> tb, const float *bank,
                                                                  const long long *noise_tab, int J, double *ws) {
    const int tile = blockIdx.x, t = threadIdx.x;
    const ragged_tile at = ragged_tile_of(tb, tile, AUG_TILE);
    const int u = at.u;
    const long long s0 = tb.col(0)[u], n = tb.count(0, u), m0 = at.first;
    double *red = (double *)ds_dynamic_lds();
    const double p_r = aug_utt_sum(ws, tb.tile_off()[u], tb.tile_off()[u + 1], 1, red) / (double)n;

    float g[AUG_MAX_NOISES];
    const float *v[AUG_MAX_NOISES];
    unsigned len[AUG_MAX_NOISES], pos[AUG_MAX_NOISES];
#pragma unroll
    for (int j = 0; j < AUG_MAX_NOISES; ++j) {
        g[j] = 0.0f;
        v[j] = nullptr;
        len[j] = 1;
        pos[j] = 0;
        if (j < J) {
            const long long *e = noise_tab + ((long long)u * J + j) * AUG_NT;
            if (e[0] >= 0) {
                const double p_v = __builtin_bit_cast(double, e[3]), f = __builtin_bit_cast(double, e[4]);
                v[j] = bank + e[0];
                len[j] = (unsigned)e[1];
                pos[j] = (unsigned)((e[2] + m0 + t) % e[1]);
                g[j] = (p_r > 0.0 && p_v > 0.0) ? (float)sqrt(p_r / (p_v * f)) : 0.0f;
            }
        }
    }
    const long long left = n - m0;
    double ss = 0.0;
    for (int m = t; m < AUG_TILE; m += AUG_THREADS) {
        if (m < left) {
            float s = data[s0 + m0 + m];
#pragma unroll
            for (int j = 0; j < AUG_MAX_NOISES; ++j)
                if (v[j]) s = fmaf(g[j], v[j][pos[j]], s);
            data[s0 + m0 + m] = s;
            ss += (double)s * (double)s;
        }
#pragma unroll
        for (int j = 0; j < AUG_MAX_NOISES; ++j) {
            pos[j] += AUG_THREADS;
            if (pos[j] >= len[j]) pos[j] %= len[j];
        }
    }
    ss = aug_block_sum(ss, red);
    if (t == 0) ws[(long long)tile * AUG_WS + 2] = ss;
}

__global__ void __launch_bounds__(AUG_THREADS) augment_level_kernel(float *data, ragged_table<1> tb, int s_slot,
                                                                    const double *ws) {
    const int tile = blockIdx.x, t = threadIdx.x;
    const ragged_tile at = ragged_tile_of(tb, tile, AUG_TILE);
    const int u = at.u;
    const long long s0 = tb.col(0)[u], n = tb.count(0, u), m0 = at.first;
    double *red = (double *)ds_dynamic_lds();
    const double sum_x = aug_utt_sum(ws, tb.tile_off()[u], tb.tile_off()[u + 1], 0, red);
    const double sum_s = aug_utt_sum(ws, tb.tile_off()[u], tb.tile_off()[u + 1], s_slot, red);
    if (!(sum_s > 0.0)) return;                              // uniform over the workgroup: y = s
    const float scale = (float)sqrt(sum_x / sum_s);
    const long long left = n - m0;
    for (int m = t; m < AUG_TILE; m += AUG_THREADS)
        if (m < left) data[s0 + m0 + m] *= scale;
}

}  // namespace

extern "C" int ds_augment_plan(const long long *lengths, int n_utt, long long *table, long long *counts) {
    DS_REQUIRE(lengths && counts, DS_ERR_NULL);
    DS_REQUIRE(n_utt > 0, DS_ERR_BAD_SHAPE);
    ragged_plan<1> plan{table, n_utt};
    for (int u = 0; u < n_utt; ++u) {
        const long long len = lengths[u];
        DS_REQUIRE(len > 0 && len < (1LL << 40), DS_ERR_BAD_SHAPE);
        plan.add(u, {len}, (len + AUG_TILE - 1) / AUG_TILE);
        DS_REQUIRE(plan.tiles < (1LL << 31) && plan.total[0] < (1LL << 44), DS_ERR_BAD_SHAPE);
    }
    plan.finish();
    counts[0] = plan.total[0];
    counts[1] = plan.tiles;
    counts[2] = AUG_TILE;
    counts[3] = AUG_KCHUNK;
    return 0;
}

extern "C" long long ds_augment_workspace_bytes(int n_tiles) {
    return n_tiles > 0 ? (long long)n_tiles * AUG_WS * 8 : 0;
}

extern "C" int ds_augment_reverb_f32(const void *samples, int in_int16, const long long *table, int n_utt, int n_tiles,
                                     const float *rir_bank, const long long *rir_tab, int max_taps, float *out,
                                     double *workspace, void *stream) {
    DS_REQUIRE(samples && table && out && workspace, DS_ERR_NULL);
    DS_REQUIRE((rir_bank == nullptr) == (rir_tab == nullptr), DS_ERR_NULL);
    DS_REQUIRE(n_utt > 0 && n_tiles > 0 && max_taps >= 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(in_int16 == 0 || in_int16 == 1, DS_ERR_UNSUPPORTED);
    DS_REQUIRE(max_taps <= AUG_MAX_TAPS, DS_ERR_UNSUPPORTED);
    const size_t lds = 4 * (size_t)AUG_LDS_FLOATS;
    if (in_int16)
        DS_LAUNCH(augment_reverb_kernel<short>, n_tiles, AUG_THREADS, lds, stream, (const short *)samples,
                  ragged_table<1>{table, n_utt}, rir_bank, rir_tab, out, workspace);
    else
        DS_LAUNCH(augment_reverb_kernel<float>, n_tiles, AUG_THREADS, lds, stream, (const float *)samples,
                  ragged_table<1>{table, n_utt}, rir_bank, rir_tab, out, workspace);
    return ds_last_launch_error();
}

extern "C" int ds_augment_mix_f32(float *data, const long long *table, int n_utt, int n_tiles, const float *noise_bank,
                                  const long long *noise_tab, int n_noises, double *workspace, void *stream) {
    DS_REQUIRE(data && table && noise_bank && noise_tab && workspace, DS_ERR_NULL);
    DS_REQUIRE(n_utt > 0 && n_tiles > 0 && n_noises > 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(n_noises <= AUG_MAX_NOISES, DS_ERR_UNSUPPORTED);
    DS_LAUNCH(augment_mix_kernel, n_tiles, AUG_THREADS, 4 * AUG_RED, stream, data, ragged_table<1>{table, n_utt},
              noise_bank, noise_tab, n_noises, workspace);
    return ds_last_launch_error();
}

extern "C" int ds_augment_level_f32(float *data, const long long *table, int n_utt, int n_tiles, int mixed,
                                    const double *workspace, void *stream) {
    DS_REQUIRE(data && table && workspace, DS_ERR_NULL);
    DS_REQUIRE(n_utt > 0 && n_tiles > 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(mixed == 0 || mixed == 1, DS_ERR_UNSUPPORTED);
    DS_LAUNCH(augment_level_kernel, n_tiles, AUG_THREADS, 4 * AUG_RED, stream, data, ragged_table<1>{table, n_utt},
              mixed ? 2 : 1, workspace);
    return ds_last_launch_error();
}
