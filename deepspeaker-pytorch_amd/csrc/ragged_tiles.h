// ragged_tiles.h -- the parts the waveform front end shares (fbank.hip, resample.hip, vad.hip, augment.hip): the tile
// table over a packed batch of utterances of unequal length, the PCM sample loader and the per-tile statistics.
//
// The table (int64; built on the host, read on the device) of n_utt utterances with C kinds of item each:
//   col_0[n_utt+1] | ... | col_{C-1}[n_utt+1] | tile_off[n_utt+1] | tile_utt[n_tiles]
// col_c[u] is the offset of utterance u's items of kind c in their packed array and col_c[n_utt] their total, so the
// utterance has col_c[u+1] - col_c[u] of them.  The items of the LAST column are cut into tiles of a fixed size, and a
// tile never straddles an utterance: utterance u owns the tiles tile_off[u] .. tile_off[u+1], and tile_utt[tile] is the
// utterance of a tile.  C = 2 for the filterbank (samples, frames) and the resampler (inputs, outputs); C = 1 for the
// voice-activity decision (frames) and the augmentation (samples).
#pragma once

constexpr int FB_SAMPLES = 0, FB_FRAMES = 1;     // the columns of ds_fbank_plan's table, which vad.hip reads too

template <int C>
struct ragged_table {
    const long long *table;
    int n_utt;
    __host__ __device__ const long long *col(int c) const { return table + (long long)c * (n_utt + 1); }
    __host__ __device__ const long long *tile_off() const { return col(C); }
    __host__ __device__ const long long *tile_utt() const { return col(C + 1); }
    __host__ __device__ long long count(int c, int u) const { return col(c)[u + 1] - col(c)[u]; }
};

// where a tile lies: its utterance and its first item inside the utterance
struct ragged_tile {
    int u;
    long long first;
    // the tile's live items in an utterance of n: all of items_per_tile but in the utterance's last tile
    __host__ __device__ int rows(long long n, int items_per_tile) const {
        return (int)(n - first < items_per_tile ? n - first : items_per_tile);
    }
};

template <int C>
__host__ __device__ inline ragged_tile ragged_tile_of(const ragged_table<C> &tb, int tile, int items_per_tile) {
    const int u = (int)tb.tile_utt()[tile];
    return {u, (tile - tb.tile_off()[u]) * items_per_tile};
}

// Host: the table utterance by utterance.  With a null table nothing is written and only the totals are kept: the
// first of a planner's two passes, which sizes the table of the second.
template <int C>
struct ragged_plan {
    long long *table;
    int n_utt;
    long long total[C] = {};                     // items of every column so far
    long long tiles = 0;
    long long *col(int c) const { return table + (long long)c * (n_utt + 1); }

    // utterance u (in order) has sizes[c] items of kind c, in n_tiles tiles
    void add(int u, const long long (&sizes)[C], long long n_tiles) {
        if (table) {
            for (int c = 0; c < C; ++c) col(c)[u] = total[c];
            col(C)[u] = tiles;
            for (long long i = 0; i < n_tiles; ++i) col(C + 1)[tiles + i] = u;
        }
        for (int c = 0; c < C; ++c) total[c] += sizes[c];
        tiles += n_tiles;
    }
    // the closing row
    void finish() {
        if (!table) return;
        for (int c = 0; c < C; ++c) col(c)[n_utt] = total[c];
        col(C)[n_utt] = tiles;
    }
};

// sample i of float32 or int16 PCM on the unit scale (int16 times 1/32768: exact in f32, librosa's scaling) ...
template <typename T> __device__ __forceinline__ float ds_pcm(const T *x, long long i);
template <> __device__ __forceinline__ float ds_pcm<float>(const float *x, long long i) { return x[i]; }
template <> __device__ __forceinline__ float ds_pcm<short>(const short *x, long long i) {
    return (float)x[i] * (1.0f / 32768.0f);
}
// ... and on the int16 scale: the integer itself, or the float times 32768 (a power of two: exact)
template <typename T> __device__ __forceinline__ float ds_pcm_i16(const T *x, long long i);
template <> __device__ __forceinline__ float ds_pcm_i16<float>(const float *x, long long i) { return x[i] * 32768.0f; }
template <> __device__ __forceinline__ float ds_pcm_i16<short>(const short *x, long long i) { return (float)x[i]; }

// The statistics of one tile of up to tile_rows rows of nfilt floats, for the per-utterance normalisation
// (fbank_stats_kernel).  Workspace: partial[n_tiles][2][nfilt] f64 = every filter's {sum, sum of squares} over the
// tile's live rows, followed by what the consumer adds.
template <typename D>                            // double or const double
__host__ __device__ inline D *ragged_tile_stats_at(D *partial, long long tile, int nfilt) {
    return partial + tile * 2 * nfilt;
}

// One workgroup of THREADS makes its tile's rows and their statistics: y = value(f, r) is stored to dst[r][f] and summed
// AS STORED, in f64: thread item (f, q) takes the rows of quarter q of the tile in order, then the four quarters are
// added in order.  The order depends on nothing but the row's place in its tile: deterministic, the same for every
// producer.  part: LDS [2][4][nfilt] f64.  The caller has synchronised whatever value() reads.
template <int THREADS, typename Value>
__device__ __forceinline__ void ragged_tile_stats(double *part, int tile, int rows, int tile_rows, int nfilt, float *dst,
                                                  double *partial, Value value) {
    const int t = threadIdx.x, rq = tile_rows / 4;
    for (int it = t; it < 4 * nfilt; it += THREADS) {
        const int f = it % nfilt, q = it / nfilt;
        double sum = 0.0, sq = 0.0;
        const int end = (q + 1) * rq < rows ? (q + 1) * rq : rows;
        for (int r = q * rq; r < end; ++r) {
            const float y = value(f, r);
            dst[(long long)r * nfilt + f] = y;
            sum += (double)y;
            sq += (double)y * (double)y;
        }
        part[q * nfilt + f] = sum;
        part[(4 + q) * nfilt + f] = sq;
    }
    __syncthreads();
    double *mine = ragged_tile_stats_at(partial, tile, nfilt);
    for (int f = t; f < nfilt; f += THREADS) {
        double sum = 0.0, sq = 0.0;
        for (int q = 0; q < 4; ++q) {
            sum += part[q * nfilt + f];
            sq += part[(4 + q) * nfilt + f];
        }
        mine[f] = sum;
        mine[nfilt + f] = sq;
    }
}
