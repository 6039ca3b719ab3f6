// fbank.hip -- log-mel filterbank front end: waveforms -> [T_u, nfilt] features (the reference's mk_MFB,
// audio_processing.py:9-36: python_speech_features.fbank(nfilt=64, winlen=0.025), 20*log10(max(fb, 1e-5)),
// normalize_frames).
//   * ds_fbank_plan: host arithmetic -- frame counts, row offsets and the tile table (tiles never straddle utterances)
//   * fbank_logmel_kernel: one workgroup per tile of up to 64 frames of one utterance.  The tile's sample span is staged
//     into LDS with pre-emphasis applied; the DFT is a GEMM on v_mfma_f32_32x32x2_f32 whose A operand reads frame r at
//     LDS offset r*frame_step (the frame matrix is never materialised) and whose B operand is the [K][nfft] cos/sin
//     basis (read through L2).  Columns are ordered so that cos_k and sin_k of one bin land in the same lane: the power
//     spectrum is formed in registers.  Epilogue: sparse mel weights, floor, 20*log10, f32 store, and the tile's
//     per-filter {sum, sum of squares} in f64 for the normalisation.
//   * fbank_stats_kernel + fbank_apply_kernel: per utterance, the tiles' partials reduced in a fixed order (no atomics:
//     deterministic and batch-invariant), then mean (and std) removed in place.
#include <ds_device.h>
#include "ds_common.h"
#include "ragged_tiles.h"

namespace {

constexpr int FB_THREADS = 256;
constexpr int FB_LDS_MAX = 160 * 1024;

// LDS of one tile of `tm` frames: partial sums [2][4][nfilt] f64 | power [tm][nfft/2+1] f32 | samples [span] f32
__host__ __device__ inline int fb_span(int tm, int frame_len, int frame_step) {
    return (tm - 1) * frame_step + ((frame_len + 1) & ~1);
}
inline long long fb_lds_bytes(int tm, int frame_len, int frame_step, int nfft, int nfilt) {
    const long long span = fb_span(tm, frame_len, frame_step);
    return 64LL * nfilt + 4LL * tm * (nfft / 2 + 1) + 4 * ((span + 3) & ~3LL);
}
// 64 frames per tile where the LDS allows it, else 32; 0 = configuration not supported
inline int fb_tile_rows(int frame_len, int frame_step, int nfft, int nfilt) {
    if (frame_len < 1 || frame_step < 1 || frame_len > nfft || nfft < 64 || nfft > 1024 || (nfft & (nfft - 1)) ||
        nfilt < 4 || nfilt > 128 || (nfilt & 3))
        return 0;
    if (fb_lds_bytes(64, frame_len, frame_step, nfft, nfilt) <= FB_LDS_MAX) return 64;
    if (fb_lds_bytes(32, frame_len, frame_step, nfft, nfilt) <= FB_LDS_MAX) return 32;
    return 0;
}

// y[g] = x[g] - 0.97 * x[g-1] in f32 with TWO roundings (NumPy's float32 arithmetic): no fused multiply-add
__device__ __forceinline__ float fb_preemph(float x, float xm1) {
#pragma clang fp contract(off)
    const float p = 0.97f * xm1;
    return x - p;
}

// table: ragged_table<2> of (samples, frames), the frames in tiles
template <typename T, int MB>
__global__ void __launch_bounds__(FB_THREADS) fbank_logmel_kernel(
    const T *x, ragged_table<2> tb, const float *basis, const int *band, const float *mel_w, int wstride, int frame_len,
    int frame_step, int nfft, int nfilt, int log_scale, float *out, double *partial) {
    constexpr int TM = 32 * MB;
    const int tile = blockIdx.x, t = threadIdx.x;
    const ragged_tile at = ragged_tile_of(tb, tile, TM);
    const int u = at.u, rows = at.rows(tb.count(FB_FRAMES, u), TM);
    const long long frame0 = at.first, s0 = tb.col(FB_SAMPLES)[u], len = tb.count(FB_SAMPLES, u);
    const int nb = nfft / 2 + 1, kpad = (frame_len + 1) & ~1, span = fb_span(TM, frame_len, frame_step);

    double *part = (double *)ds_dynamic_lds();               // [2][4][nfilt]
    float *pw = (float *)(part + 8 * nfilt);                 // [TM][nb]
    float *xs = pw + TM * nb;                                // [span]

    // stage the tile's samples, pre-emphasised, zero past the utterance's end (padding comes after pre-emphasis)
    const long long g0 = frame0 * frame_step;
    for (int s = t; s < span; s += FB_THREADS) {
        const long long g = g0 + s;
        float y = 0.0f;
        if (g < len) {
            const float xg = ds_pcm<T>(x, s0 + g);
            y = g == 0 ? xg : fb_preemph(xg, ds_pcm<T>(x, s0 + g - 1));
        }
        xs[s] = y;
    }
    __syncthreads();

    // DFT GEMM: [TM frames] x [kpad samples] . [kpad][nfft basis columns].  Column pair p = 64 columns: cos_k at
    // 64p + j and sin_k at 64p + 32 + j for k = 32p + j (sin_0 = 0: that slot holds cos_{nfft/2}, the Nyquist bin)
    const int wave = t >> 6, lane = t & 63, j = lane & 31, kh = lane >> 5;
    const int n_pairs = nfft >> 6;
    const float inv_n = 1.0f / (float)nfft;
    for (int p = wave; p < n_pairs; p += FB_THREADS / 64) {
        f32x16 cc[MB], ss[MB];
#pragma unroll
        for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) cc[m][r] = ss[m][r] = 0.0f;
        const float *bp = basis + (size_t)kh * nfft + 64 * p + j;
        const float *ap = xs + j * frame_step + kh;
#pragma unroll 4
        for (int k0 = 0; k0 < kpad; k0 += 2) {
            const float bc = bp[(size_t)k0 * nfft], bs = bp[(size_t)k0 * nfft + 32];
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                const float a = ap[m * 32 * frame_step + k0];
                cc[m] = ds_mfma_32x32x2_f32(a, bc, cc[m]);
                ss[m] = ds_mfma_32x32x2_f32(a, bs, ss[m]);
            }
        }
        // power |X_k|^2 / nfft, formed in the lane that holds both halves of the bin
        const int k = 32 * p + j;
#pragma unroll
        for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                const double c = cc[m][r], s = ss[m][r];
                if (k == 0) {
                    pw[row * nb] = (float)(c * c * (double)inv_n);
                    pw[row * nb + nfft / 2] = (float)(s * s * (double)inv_n);
                } else {
                    pw[row * nb + k] = (float)((c * c + s * s) * (double)inv_n);
                }
            }
    }
    __syncthreads();

    // mel filterbank, floor, log
    ragged_tile_stats<FB_THREADS>(part, tile, rows, TM, nfilt, out + (tb.col(FB_FRAMES)[u] + frame0) * nfilt, partial,
                                  [&](int f, int r) {
        const int b0 = band[2 * f], cnt = band[2 * f + 1];
        const float *w = mel_w + (size_t)f * wstride, *pr = pw + r * nb + b0;
        double fb = 0.0;
        for (int i = 0; i < cnt; ++i) fb += (double)w[i] * (double)pr[i];
        if (fb == 0.0) fb = 2.220446049250313e-16;                      // numpy.finfo(float).eps
        const double v = log_scale ? 20.0 * log10(fb > 1e-5 ? fb : 1e-5) : fb;
        // the statistics are those of the STORED values: x - mean is then exactly 0 where an utterance's frames
        // are all equal (one frame, silence), as in the reference's float64 arithmetic
        return (float)v;
    });
}

// per utterance: mean and (std + 2e-12) of every filter over its frames, from its tiles' partials in a fixed order
__global__ void __launch_bounds__(FB_THREADS) fbank_stats_kernel(ragged_table<2> tb, int nfilt,
                                                                 const double *partial, double *stats) {
    double *lds = (double *)ds_dynamic_lds();                // [2][G][nfilt]
    const int u = blockIdx.x, t = threadIdx.x, G = FB_THREADS / nfilt;
    const int t0 = (int)tb.tile_off()[u], nt = (int)(tb.tile_off()[u + 1] - t0), chunk = (nt + G - 1) / G;
    if (t < G * nfilt) {
        const int f = t % nfilt, g = t / nfilt;
        const int a = t0 + g * chunk, b = (t0 + (g + 1) * chunk) < (t0 + nt) ? t0 + (g + 1) * chunk : t0 + nt;
        double sum = 0.0, sq = 0.0;
        for (int i = a; i < b; ++i) {
            const double *of_tile = ragged_tile_stats_at(partial, i, nfilt);
            sum += of_tile[f];
            sq += of_tile[nfilt + f];
        }
        lds[g * nfilt + f] = sum;
        lds[(G + g) * nfilt + f] = sq;
    }
    __syncthreads();
    for (int f = t; f < nfilt; f += FB_THREADS) {
        double sum = 0.0, sq = 0.0;
        for (int g = 0; g < G; ++g) {
            sum += lds[g * nfilt + f];
            sq += lds[(G + g) * nfilt + f];
        }
        const double n = (double)tb.count(FB_FRAMES, u);
        const double mean = sum / n, var = sq / n - mean * mean;
        stats[(size_t)u * 2 * nfilt + f] = mean;
        stats[(size_t)u * 2 * nfilt + nfilt + f] = sqrt(var > 0.0 ? var : 0.0) + 2e-12;
    }
}

// one workgroup per tile: x = (x - mean) [/ (std + 2e-12)], in place
__global__ void __launch_bounds__(FB_THREADS) fbank_apply_kernel(float *feat, ragged_table<2> tb,
                                                                 int nfilt, int tm, int use_scale, const double *stats) {
    double *st = (double *)ds_dynamic_lds();                 // [2][nfilt]
    const int tile = blockIdx.x, t = threadIdx.x;
    const ragged_tile at = ragged_tile_of(tb, tile, tm);
    const int u = at.u;
    for (int i = t; i < 2 * nfilt; i += FB_THREADS) st[i] = stats[(size_t)u * 2 * nfilt + i];
    __syncthreads();
    const int rows = at.rows(tb.count(FB_FRAMES, u), tm);
    float *y = feat + (tb.col(FB_FRAMES)[u] + at.first) * nfilt;
    for (int e = t; e < rows * nfilt; e += FB_THREADS) {
        const int f = e % nfilt;
        double v = (double)y[e] - st[f];
        if (use_scale) v = v / st[nfilt + f];
        y[e] = (float)v;
    }
}

// the staging arithmetic alone, for tests: y = pre-emphasis of one signal of n samples
template <typename T>
__global__ void __launch_bounds__(FB_THREADS) fbank_preemphasis_kernel(const T *x, long long n, float *y) {
    for (long long g = (long long)blockIdx.x * FB_THREADS + threadIdx.x; g < n; g += (long long)gridDim.x * FB_THREADS) {
        const float xg = ds_pcm<T>(x, g);
        y[g] = g == 0 ? xg : fb_preemph(xg, ds_pcm<T>(x, g - 1));
    }
}

template <typename T>
int fbank_launch(const T *x, ragged_table<2> tb, int n_tiles, int tm, const float *basis, const int *band,
                 const float *mel_w, int wstride, int frame_len, int frame_step, int nfft, int nfilt, int log_scale,
                 float *out, double *partial, void *stream) {
    const size_t lds = (size_t)fb_lds_bytes(tm, frame_len, frame_step, nfft, nfilt);
    if (tm == 64)
        DS_LAUNCH_BIG_LDS((fbank_logmel_kernel<T, 2>), n_tiles, FB_THREADS, lds, stream, x, tb, basis, band,
                          mel_w, wstride, frame_len, frame_step, nfft, nfilt, log_scale, out, partial);
    else
        DS_LAUNCH_BIG_LDS((fbank_logmel_kernel<T, 1>), n_tiles, FB_THREADS, lds, stream, x, tb, basis, band,
                          mel_w, wstride, frame_len, frame_step, nfft, nfilt, log_scale, out, partial);
    return ds_last_launch_error();
}

}  // namespace

extern "C" int ds_fbank_plan(const long long *lengths, int n_utt, int frame_len, int frame_step, int nfft, int nfilt,
                             long long *table, long long *counts) {
    DS_REQUIRE(lengths && counts, DS_ERR_NULL);
    DS_REQUIRE(n_utt > 0, DS_ERR_BAD_SHAPE);
    const int tm = fb_tile_rows(frame_len, frame_step, nfft, nfilt);
    DS_REQUIRE(tm > 0, DS_ERR_UNSUPPORTED);
    ragged_plan<2> plan{table, n_utt};
    for (int u = 0; u < n_utt; ++u) {
        const long long len = lengths[u];
        DS_REQUIRE(len > 0, DS_ERR_BAD_SHAPE);                // an empty signal has no frame (the reference fails too)
        // python_speech_features.sigproc.framesig: one frame up to frame_len samples, then one per started step
        const long long nf = len <= frame_len ? 1 : 1 + (len - frame_len + frame_step - 1) / frame_step;
        plan.add(u, {len, nf}, (nf + tm - 1) / tm);
    }
    const long long frames = plan.total[FB_FRAMES];
    DS_REQUIRE(plan.tiles < (1LL << 31) && frames * nfilt < (1LL << 40), DS_ERR_BAD_SHAPE);
    plan.finish();
    counts[0] = frames;
    counts[1] = plan.tiles;
    counts[2] = tm;
    return 0;
}

extern "C" long long ds_fbank_workspace_bytes(int n_utt, int n_tiles, int nfilt) {
    if (n_utt <= 0 || n_tiles <= 0 || nfilt <= 0) return DS_ERR_BAD_SHAPE;
    return 8LL * 2 * nfilt * ((long long)n_tiles + n_utt);
}

extern "C" int ds_fbank_logmel_f32(const void *samples, int in_int16, const long long *table, int n_utt, int n_tiles,
                                   const float *basis, const int *band, const float *mel_w, int wstride, int frame_len,
                                   int frame_step, int nfft, int nfilt, int log_scale, float *out, double *workspace,
                                   void *stream) {
    DS_REQUIRE(samples && table && basis && band && mel_w && out && workspace, DS_ERR_NULL);
    DS_REQUIRE(n_utt > 0 && n_tiles > 0 && wstride > 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(in_int16 == 0 || in_int16 == 1, DS_ERR_UNSUPPORTED);
    const int tm = fb_tile_rows(frame_len, frame_step, nfft, nfilt);
    DS_REQUIRE(tm > 0, DS_ERR_UNSUPPORTED);
    if (in_int16)
        return fbank_launch((const short *)samples, {table, n_utt}, n_tiles, tm, basis, band, mel_w, wstride, frame_len,
                            frame_step, nfft, nfilt, log_scale, out, workspace, stream);
    return fbank_launch((const float *)samples, {table, n_utt}, n_tiles, tm, basis, band, mel_w, wstride, frame_len,
                        frame_step, nfft, nfilt, log_scale, out, workspace, stream);
}

extern "C" int ds_fbank_normalize_f32(float *feat, const long long *table, int n_utt, int n_tiles, int nfilt,
                                      int tile_rows, int use_scale, double *workspace, void *stream) {
    DS_REQUIRE(feat && table && workspace, DS_ERR_NULL);
    DS_REQUIRE(n_utt > 0 && n_tiles > 0 && (tile_rows == 64 || tile_rows == 32), DS_ERR_BAD_SHAPE);
    DS_REQUIRE(nfilt >= 4 && nfilt <= 128 && (nfilt & 3) == 0, DS_ERR_UNSUPPORTED);
    const ragged_table<2> tb{table, n_utt};
    const double *partial = workspace;
    double *stats = workspace + (size_t)n_tiles * 2 * nfilt;
    DS_LAUNCH(fbank_stats_kernel, n_utt, FB_THREADS, 2 * FB_THREADS * 8, stream, tb, nfilt, partial, stats);
    const int rc = ds_last_launch_error();
    if (rc) return rc;
    DS_LAUNCH(fbank_apply_kernel, n_tiles, FB_THREADS, 2 * nfilt * 8, stream, feat, tb, nfilt, tile_rows,
              use_scale != 0, (const double *)stats);
    return ds_last_launch_error();
}

extern "C" int ds_fbank_preemphasis_f32(const void *samples, int in_int16, long long n, float *out, void *stream) {
    DS_REQUIRE(samples && out, DS_ERR_NULL);
    DS_REQUIRE(n > 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(in_int16 == 0 || in_int16 == 1, DS_ERR_UNSUPPORTED);
    const int grid = (int)(ds_ceil_div_ll(n, FB_THREADS) < 1024 ? ds_ceil_div_ll(n, FB_THREADS) : 1024);
    if (in_int16)
        DS_LAUNCH(fbank_preemphasis_kernel<short>, grid, FB_THREADS, 0, stream, (const short *)samples, n, out);
    else
        DS_LAUNCH(fbank_preemphasis_kernel<float>, grid, FB_THREADS, 0, stream, (const float *)samples, n, out);
    return ds_last_launch_error();
}
