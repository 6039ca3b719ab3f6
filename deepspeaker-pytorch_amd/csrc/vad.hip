// vad.hip -- energy-based voice-activity decision on the filterbank's own framing, and selection of the voiced rows
// (the rule of Kaldi's compute-vad-energy / select-voiced-frames; not bit-compatible with it).  For utterance u:
//   e[t]   = ln(max(sum_i (32768 x[t*step + i])^2, floor)),  0 <= i < frame_len, samples past the end are zero
//   thr    = energy_threshold + energy_mean_scale * mean_t e[t]                       (f64, fixed order)
//   voiced = count(e[lo..hi] > thr) >= proportion * (hi - lo + 1),  lo = max(0, t - ctx), hi = min(T - 1, t + ctx)
//   * vad_energy_kernel: one workgroup per tile of the FBANK table (ds_fbank_plan: samples and frames, the frames in
//     tiles).  The tile's sample span is staged into LDS once, on the int16 scale; a wavefront sums one frame: lane l
//     takes samples l, l + 64, ... in order (consecutive LDS words: no bank conflict), then a fixed xor butterfly.  The
//     order depends on nothing but the sample's place in its frame: deterministic, independent of tile, batch and call.
//   * the decision works on tiles of VAD_DT frames of one utterance (ds_vad_plan: the frames alone):
//       vad_threshold_kernel  one workgroup per utterance: the f64 mean in a fixed order (no atomics), the threshold
//       vad_vote_kernel       one workgroup per tile: e > thr of the tile and its halo in LDS, the clipped-window vote,
//                             the uint8 mask and the tile's kept count
//       vad_tile_scan_kernel  one workgroup per utterance: exclusive scan of its tiles' counts, the kept count
//       vad_scan_kernel       one workgroup per tile: exclusive scan of the mask inside the tile + the tile's base
//     A reduce-then-scan in separate launches: an utterance of any length, no workgroup ever waits for another.
//   * vad_select_kernel: one workgroup per tile of the table over the KEPT frames (the fbank table's layout).  Output row
//     k of an utterance is the frame j with mask[j] != 0 and scan[j] == k, found by bisection of the scan; rows are copied
//     a wavefront per 64 floats, and the tile's per-filter {sum, sum of squares} come out in f64 in fbank_logmel_kernel's
//     layout and order, so ds_fbank_normalize_f32 normalises the kept rows with the table over them.
#include <ds_device.h>
#include "ds_common.h"
#include "ragged_tiles.h"
#include <math.h>

namespace {

constexpr int VAD_THREADS = 256;
constexpr int VAD_DT = 1024;                     // frames per workgroup of the decision kernels (4 per thread)
constexpr int VAD_PER = VAD_DT / VAD_THREADS;
constexpr int VAD_MAX_CONTEXT = 64;              // halo frames on each side of a decision tile
constexpr int VAD_LDS_MAX = 160 * 1024;

inline long long vad_span(int tm, int frame_len, int frame_step) { return (long long)(tm - 1) * frame_step + frame_len; }

// table: ds_fbank_plan's, ragged_table<2> of (samples, frames), the frames in tiles of tm; the samples enter on the
// int16 scale
template <typename T>
__global__ void __launch_bounds__(VAD_THREADS) vad_energy_kernel(const T *x, ragged_table<2> tb, int tm,
                                                                 int frame_len, int frame_step, float floor_v,
                                                                 float log_floor, float *out) {
    const int tile = blockIdx.x, t = threadIdx.x;
    const ragged_tile at = ragged_tile_of(tb, tile, tm);
    const int u = at.u, rows = at.rows(tb.count(FB_FRAMES, u), tm);
    const long long frame0 = at.first, s0 = tb.col(FB_SAMPLES)[u], len = tb.count(FB_SAMPLES, u);
    const int span = (rows - 1) * frame_step + frame_len;

    float *es = ds_dynamic_lds();                            // [tm] frame sums
    float *xs = es + tm;                                     // [span]
    const long long g0 = frame0 * frame_step;
    for (int s = t; s < span; s += VAD_THREADS) {
        const long long g = g0 + s;
        xs[s] = g < len ? ds_pcm_i16<T>(x, s0 + g) : 0.0f;
    }
    __syncthreads();

    const int wave = t >> 6, lane = t & 63;
    for (int r = wave; r < rows; r += VAD_THREADS / 64) {
        const float *fr = xs + r * frame_step;
        float acc = 0.0f;
        for (int i = lane; i < frame_len; i += 64) acc = fmaf(fr[i], fr[i], acc);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc += ds_shfl_xor(acc, m);
        if (lane == 0) es[r] = acc;
    }
    __syncthreads();
    for (int r = t; r < rows; r += VAD_THREADS) {
        const float s = es[r];
        out[tb.col(FB_FRAMES)[u] + frame0 + r] = s > floor_v ? logf(s) : log_floor;
    }
}

// vtable: ds_vad_plan's, ragged_table<1> of the frames, in tiles of VAD_DT
__global__ void __launch_bounds__(VAD_THREADS) vad_threshold_kernel(const float *energy, ragged_table<1> vt,
                                                                    double energy_threshold,
                                                                    double energy_mean_scale, double *thr) {
    double *lds = (double *)ds_dynamic_lds();                // [VAD_THREADS]
    const int u = blockIdx.x, t = threadIdx.x;
    const long long f0 = vt.col(0)[u], T = vt.count(0, u);
    double s = 0.0;
    for (long long i = t; i < T; i += VAD_THREADS) s += (double)energy[f0 + i];
    lds[t] = s;
    __syncthreads();
    for (int w = VAD_THREADS / 2; w >= 1; w >>= 1) {         // a fixed tree
        if (t < w) lds[t] += lds[t + w];
        __syncthreads();
    }
    if (t == 0) thr[u] = T > 0 ? energy_threshold + energy_mean_scale * (lds[0] / (double)T) : 0.0;
}

// sum of the threads' `mine` in lds[0 .. VAD_THREADS) (int), returned to every thread
__device__ __forceinline__ int vad_block_sum(int *lds, int t, int mine) {
    lds[t] = mine;
    __syncthreads();
    for (int w = VAD_THREADS / 2; w >= 1; w >>= 1) {
        if (t < w) lds[t] += lds[t + w];
        __syncthreads();
    }
    const int total = lds[0];
    __syncthreads();
    return total;
}

__global__ void __launch_bounds__(VAD_THREADS) vad_vote_kernel(const float *energy, ragged_table<1> vt,
                                                               const double *thr, int ctx, double proportion,
                                                               unsigned char *mask, long long *tile_count) {
    int *red = (int *)ds_dynamic_lds();                      // [VAD_THREADS]
    unsigned char *above = (unsigned char *)(red + VAD_THREADS);   // [VAD_DT + 2 ctx]: frames first - ctx ...
    const int tile = blockIdx.x, t = threadIdx.x;
    const ragged_tile at = ragged_tile_of(vt, tile, VAD_DT);
    const int u = at.u;
    const long long f0 = vt.col(0)[u], T = vt.count(0, u), first = at.first;
    const int rows = at.rows(T, VAD_DT);
    const double th = thr[u];
    for (int i = t; i < rows + 2 * ctx; i += VAD_THREADS) {
        const long long f = first - ctx + i;                 // never a neighbouring utterance's frame
        above[i] = (f >= 0 && f < T && (double)energy[f0 + f] > th) ? 1 : 0;
    }
    __syncthreads();
    int kept = 0;
    for (int r = t; r < rows; r += VAD_THREADS) {
        const long long f = first + r;
        const long long lo = f - ctx > 0 ? f - ctx : 0, hi = f + ctx < T - 1 ? f + ctx : T - 1;
        int count = 0;
        for (int i = (int)(lo - first) + ctx; i <= (int)(hi - first) + ctx; ++i) count += above[i];
        const int v = (double)count >= proportion * (double)(hi - lo + 1) ? 1 : 0;
        mask[f0 + f] = (unsigned char)v;
        kept += v;
    }
    const int total = vad_block_sum(red, t, kept);
    if (t == 0) tile_count[tile] = total;
}

// a caller's own mask: the tile's count of non-zero entries
__global__ void __launch_bounds__(VAD_THREADS) vad_count_kernel(const unsigned char *mask, ragged_table<1> vt,
                                                                long long *tile_count) {
    int *red = (int *)ds_dynamic_lds();
    const int tile = blockIdx.x, t = threadIdx.x;
    const ragged_tile at = ragged_tile_of(vt, tile, VAD_DT);
    const long long f0 = vt.col(0)[at.u], first = at.first;
    const int rows = at.rows(vt.count(0, at.u), VAD_DT);
    int kept = 0;
    for (int r = t; r < rows; r += VAD_THREADS) kept += mask[f0 + first + r] != 0;
    const int total = vad_block_sum(red, t, kept);
    if (t == 0) tile_count[tile] = total;
}

// per utterance: its tiles' counts -> their exclusive scan (in place), and the kept count.  Thread t owns a contiguous
// run of tiles; the runs' totals are scanned by one thread (256 additions)
__global__ void __launch_bounds__(VAD_THREADS) vad_tile_scan_kernel(ragged_table<1> vt,
                                                                    long long *tile_count, long long *kept) {
    long long *lds = (long long *)ds_dynamic_lds();          // [VAD_THREADS + 1]
    const int u = blockIdx.x, t = threadIdx.x;
    const long long t0 = vt.tile_off()[u], nt = vt.tile_off()[u + 1] - t0, run = (nt + VAD_THREADS - 1) / VAD_THREADS;
    const long long a = t0 + t * run < t0 + nt ? t0 + t * run : t0 + nt;
    const long long b = a + run < t0 + nt ? a + run : t0 + nt;
    long long s = 0;
    for (long long i = a; i < b; ++i) s += tile_count[i];
    lds[t] = s;
    __syncthreads();
    if (t == 0) {
        long long acc = 0;
        for (int i = 0; i < VAD_THREADS; ++i) {
            const long long v = lds[i];
            lds[i] = acc;
            acc += v;
        }
        lds[VAD_THREADS] = acc;
    }
    __syncthreads();
    long long acc = lds[t];
    for (long long i = a; i < b; ++i) {
        const long long v = tile_count[i];
        tile_count[i] = acc;
        acc += v;
    }
    if (t == 0) kept[u] = lds[VAD_THREADS];
}

// scan[f] = kept frames of the utterance before f.  Thread t owns VAD_PER consecutive frames of the tile
__global__ void __launch_bounds__(VAD_THREADS) vad_scan_kernel(const unsigned char *mask, ragged_table<1> vt,
                                                               const long long *tile_base, int *scan) {
    int *lds = (int *)ds_dynamic_lds();                      // [2][VAD_THREADS]
    const int tile = blockIdx.x, t = threadIdx.x;
    const ragged_tile at = ragged_tile_of(vt, tile, VAD_DT);
    const long long f0 = vt.col(0)[at.u], first = at.first;
    const int rows = at.rows(vt.count(0, at.u), VAD_DT);
    const unsigned char *m = mask + f0 + first;
    int v[VAD_PER], mine = 0;
#pragma unroll
    for (int j = 0; j < VAD_PER; ++j) {
        const int r = t * VAD_PER + j;
        v[j] = (r < rows && m[r] != 0) ? 1 : 0;
        mine += v[j];
    }
    // inclusive scan of the threads' sums, ping-pong between the two halves
    int *src = lds, *dst = lds + VAD_THREADS;
    src[t] = mine;
    __syncthreads();
    for (int d = 1; d < VAD_THREADS; d <<= 1) {
        dst[t] = t >= d ? src[t] + src[t - d] : src[t];
        __syncthreads();
        int *swap = src;
        src = dst;
        dst = swap;
    }
    int acc = (int)tile_base[tile] + src[t] - mine;
    int *out = scan + f0 + first;
#pragma unroll
    for (int j = 0; j < VAD_PER; ++j) {
        const int r = t * VAD_PER + j;
        if (r < rows) out[r] = acc;
        acc += v[j];
    }
}

// ktable: ragged_table<2> as ds_fbank_plan's over the KEPT frames, in tiles of tm (its samples column is not read)
__global__ void __launch_bounds__(VAD_THREADS) vad_select_kernel(const float *feat, const unsigned char *mask,
                                                                 const int *scan, ragged_table<1> vt, ragged_table<2> kt,
                                                                 int nfilt, int tm, float *out, double *partial) {
    double *part = (double *)ds_dynamic_lds();               // [2][4][nfilt]
    long long *src_row = (long long *)(part + 8 * nfilt);    // [tm]
    const int tile = blockIdx.x, t = threadIdx.x;
    const ragged_tile at = ragged_tile_of(kt, tile, tm);
    const int u = at.u, rows = at.rows(kt.count(FB_FRAMES, u), tm);
    const long long k0 = at.first, f0 = vt.col(0)[u], T = vt.count(0, u);

    // output row k is the LAST frame j with scan[j] <= k (the scan steps up right after every kept frame)
    for (int r = t; r < rows; r += VAD_THREADS) {
        const long long k = k0 + r;
        long long lo = 0, hi = T - 1;
        while (lo < hi) {
            const long long mid = (lo + hi + 1) >> 1;
            if ((long long)scan[f0 + mid] <= k) lo = mid; else hi = mid - 1;
        }
        src_row[r] = (mask[f0 + lo] != 0 && (long long)scan[f0 + lo] == k) ? f0 + lo : -1;
    }
    __syncthreads();

    // copy and statistics
    ragged_tile_stats<VAD_THREADS>(part, tile, rows, tm, nfilt, out + (kt.col(FB_FRAMES)[u] + k0) * nfilt, partial,
                                   [&](int f, int r) {
        const long long j = src_row[r];
        return j >= 0 ? feat[j * nfilt + f] : 0.0f;                  // j < 0: scan and table disagree (not the library's)
    });
}

// the scan half of the decision: tile counts (already written) -> scan and kept
int vad_scan_launch(const unsigned char *mask, ragged_table<1> vt, int n_dtiles, long long *tile_count,
                    int *scan, long long *kept, void *stream) {
    DS_LAUNCH(vad_tile_scan_kernel, vt.n_utt, VAD_THREADS, (VAD_THREADS + 1) * 8, stream, vt, tile_count, kept);
    const int rc = ds_last_launch_error();
    if (rc) return rc;
    DS_LAUNCH(vad_scan_kernel, n_dtiles, VAD_THREADS, 2 * VAD_THREADS * 4, stream, mask, vt,
              (const long long *)tile_count, scan);
    return ds_last_launch_error();
}

}  // namespace

extern "C" int ds_vad_tile_frames(void) { return VAD_DT; }

extern "C" int ds_vad_plan(const long long *frame_off, int n_utt, long long *table, long long *counts) {
    DS_REQUIRE(frame_off && counts, DS_ERR_NULL);
    DS_REQUIRE(n_utt > 0, DS_ERR_BAD_SHAPE);
    ragged_plan<1> plan{table, n_utt};                       // offsets from frame_off[0] on
    for (int u = 0; u < n_utt; ++u) {
        const long long T = frame_off[u + 1] - frame_off[u];
        DS_REQUIRE(T >= 0 && T < (1LL << 31), DS_ERR_BAD_SHAPE);      // the scan inside an utterance is int32
        plan.add(u, {T}, (T + VAD_DT - 1) / VAD_DT);
        DS_REQUIRE(plan.tiles < (1LL << 31), DS_ERR_BAD_SHAPE);
    }
    plan.finish();
    counts[0] = plan.total[0];
    counts[1] = plan.tiles;
    counts[2] = VAD_DT;
    return 0;
}

extern "C" long long ds_vad_workspace_bytes(int n_utt, int n_dtiles) {
    if (n_utt <= 0 || n_dtiles <= 0) return DS_ERR_BAD_SHAPE;
    return 8LL * ((long long)n_utt + n_dtiles);
}

extern "C" int ds_vad_log_energy_f32(const void *samples, int in_int16, const long long *table, int n_utt, int n_tiles,
                                     int tile_rows, int frame_len, int frame_step, double energy_floor, float *out,
                                     void *stream) {
    DS_REQUIRE(samples && table && out, DS_ERR_NULL);
    DS_REQUIRE(n_utt > 0 && n_tiles > 0 && (tile_rows == 64 || tile_rows == 32), DS_ERR_BAD_SHAPE);
    DS_REQUIRE(in_int16 == 0 || in_int16 == 1, DS_ERR_UNSUPPORTED);
    DS_REQUIRE(frame_len >= 1 && frame_step >= 1, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(energy_floor > 0.0 && energy_floor < 3.0e38, DS_ERR_BAD_SHAPE);        // NaN fails both
    const long long lds = 4 * (tile_rows + vad_span(tile_rows, frame_len, frame_step));
    DS_REQUIRE(lds <= VAD_LDS_MAX, DS_ERR_UNSUPPORTED);
    const float floor_v = (float)energy_floor;
    DS_REQUIRE(floor_v > 0.0f, DS_ERR_BAD_SHAPE);
    const float log_floor = (float)log((double)floor_v);     // the floor's own log, rounded once: exact at the floor
    if (in_int16)
        DS_LAUNCH_BIG_LDS(vad_energy_kernel<short>, n_tiles, VAD_THREADS, (size_t)lds, stream, (const short *)samples,
                          ragged_table<2>{table, n_utt}, tile_rows, frame_len, frame_step, floor_v, log_floor, out);
    else
        DS_LAUNCH_BIG_LDS(vad_energy_kernel<float>, n_tiles, VAD_THREADS, (size_t)lds, stream, (const float *)samples,
                          ragged_table<2>{table, n_utt}, tile_rows, frame_len, frame_step, floor_v, log_floor, out);
    return ds_last_launch_error();
}

extern "C" int ds_vad_decide(const float *energy, const long long *vtable, int n_utt, int n_dtiles,
                             double energy_threshold, double energy_mean_scale, int frames_context,
                             double proportion_threshold, unsigned char *mask, int *scan, long long *kept,
                             void *workspace, void *stream) {
    DS_REQUIRE(energy && vtable && mask && scan && kept && workspace, DS_ERR_NULL);
    DS_REQUIRE(n_utt > 0 && n_dtiles > 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(frames_context >= 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(proportion_threshold > 0.0 && proportion_threshold <= 1.0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(energy_threshold - energy_threshold == 0.0 && energy_mean_scale - energy_mean_scale == 0.0,
               DS_ERR_BAD_SHAPE);                             // finite
    DS_REQUIRE(frames_context <= VAD_MAX_CONTEXT, DS_ERR_UNSUPPORTED);
    double *thr = (double *)workspace;
    long long *tile_count = (long long *)workspace + n_utt;
    const ragged_table<1> vt{vtable, n_utt};
    DS_LAUNCH(vad_threshold_kernel, n_utt, VAD_THREADS, VAD_THREADS * 8, stream, energy, vt,
              energy_threshold, energy_mean_scale, thr);
    int rc = ds_last_launch_error();
    if (rc) return rc;
    DS_LAUNCH(vad_vote_kernel, n_dtiles, VAD_THREADS, VAD_THREADS * 4 + VAD_DT + 2 * VAD_MAX_CONTEXT, stream, energy,
              vt, (const double *)thr, frames_context, proportion_threshold, mask, tile_count);
    rc = ds_last_launch_error();
    if (rc) return rc;
    return vad_scan_launch(mask, vt, n_dtiles, tile_count, scan, kept, stream);
}

extern "C" int ds_vad_scan(const unsigned char *mask, const long long *vtable, int n_utt, int n_dtiles, int *scan,
                           long long *kept, void *workspace, void *stream) {
    DS_REQUIRE(mask && vtable && scan && kept && workspace, DS_ERR_NULL);
    DS_REQUIRE(n_utt > 0 && n_dtiles > 0, DS_ERR_BAD_SHAPE);
    long long *tile_count = (long long *)workspace + n_utt;
    const ragged_table<1> vt{vtable, n_utt};
    DS_LAUNCH(vad_count_kernel, n_dtiles, VAD_THREADS, VAD_THREADS * 4, stream, mask, vt, tile_count);
    const int rc = ds_last_launch_error();
    if (rc) return rc;
    return vad_scan_launch(mask, vt, n_dtiles, tile_count, scan, kept, stream);
}

extern "C" int ds_vad_select_f32(const float *feat, const unsigned char *mask, const int *scan, const long long *vtable,
                                 const long long *ktable, int n_utt, int n_ktiles, int nfilt, int tile_rows, float *out,
                                 double *workspace, void *stream) {
    DS_REQUIRE(feat && mask && scan && vtable && ktable && out && workspace, DS_ERR_NULL);
    DS_REQUIRE(n_utt > 0 && n_ktiles > 0 && (tile_rows == 64 || tile_rows == 32), DS_ERR_BAD_SHAPE);
    DS_REQUIRE(nfilt >= 4 && nfilt <= 128 && (nfilt & 3) == 0, DS_ERR_UNSUPPORTED);
    DS_LAUNCH(vad_select_kernel, n_ktiles, VAD_THREADS, 64 * nfilt + 8 * tile_rows, stream, feat, mask, scan,
              ragged_table<1>{vtable, n_utt}, ragged_table<2>{ktable, n_utt}, nfilt, tile_rows, out, workspace);
    return ds_last_launch_error();
}
