// conv_mfma_bf16_kernel.h -- the bf16 / bf16x3 implicit-GEMM convolution kernel template and its launch
// dispatch.  Included by the per-(kernel size, arithmetic) translation units conv_mfma_bf16_k*.hip, which
// exist only so that the ~50 instantiations compile in parallel; the planner and the C ABI live in
// conv_mfma_bf16.hip.  Design notes: DESIGN_LOG.md section 3.3.
#pragma once
#include <ds_device.h>
#include <type_traits>
#include "ds_common.h"
#include "conv_mfma_f16_parts.h"      // ds_mfma_lpix


constexpr int CKB = 16;             // input channels per chunk = K of one bf16 MFMA
constexpr int PSB = 48;             // bytes per staged pixel record: 16 bf16 + 16 B pad


struct ConvKB {
    const float *x;
    const __bf16 *w_hi, *w_lo;      // packed [Cin/16][tap][Cout][16]
    float *y;
    const float *scale, *shift, *res;
    float *stats;
    int H, W, Cin;
    int Hr, Wc, Ho, Wo, Cout;
    int IS;
    int dh_min, dw_min;
    int rows_in, cols_in, seg_pix;
    int pitch, half;                // LDS records per tile row; first odd-column slot (stride-2 de-interleave)
    int RT, NI, segs_per_img, n_segs;
    int n_ntiles;
    int flags;
    unsigned y_bytes;               // size of y (and of the residual) in bytes, for the buffer descriptors
    int OS, OH0, OW0;               // output pixel (r, c) of the tile grid lands at (OS*r + OH0, OS*c + OW0) of y
    // BNB epilogue (ds_conv_dgrad_bnbwd_bf16): this launch is a data gradient whose output is dL/d(activation) of a
    // BatchNorm + clipped-ReLU layer; z = that layer's convolution output (same shape as y), tables [G][Cout] per
    // member of the batch, bn_mtiles = M tiles per member
    const float *bn_z, *bn_mean, *bn_invstd, *bn_msc, *bn_msh;
    int bn_mtiles;
    // bn_msc == nullptr: the mask comes from the layer's stored activation, passed as `res` (it is then NOT added):
    // the layers whose activation had a residual added before the clip.  The partial rows of member m start at row
    // m * bn_rows_member + bn_row0 (several launches -- the parity classes of a stride-2 data gradient -- share a table).
    int bn_rows_member, bn_row0;
};

struct PlanB {
    int cfg, grid, n_mtiles, nit;
    int pipe;                       // the pipelined walk (PIPE of the kernel): two pixel tiles in lds_bytes
    size_t lds_bytes;
    ConvKB k;
};

// THE tile configurations: a workgroup of WM x WN waves, each wave a register tile of MSUB x NSUB sub-tiles of 32 pixels
// x 32 output channels.  The planner (conv_mfma_bf16.hip) sizes its plans from the rows, launch_b instantiates the
// kernels from them; `cfg` everywhere is an index into this table.
struct TileCfgB {
    int MSUB, NSUB, WM, WN;
    int wg_per_cu;                  // resident workgroups per CU
    size_t lds_cap;                 // bytes of LDS a workgroup may plan with
    int items_per_thread;           // float4 staging slots a thread has at most (NIT of the kernel)
    bool x3_only;                   // 160x64 / 128x64 register tiles: tuned for, and only built for, bf16x3; LDS above
                                    // the default 64 KiB is opted into at launch
    constexpr int MT() const { return MSUB * WM * 32; }             // pixels per tile
    constexpr int NTILE() const { return NSUB * WN * 32; }          // output channels per tile
    constexpr int NTHR() const { return WM * WN * 64; }
    // the epilogue's per-wave transposition buffers (they alias the pixel tile): EPI_BYTES of the kernel
    constexpr size_t epi_bytes() const { return (size_t)WM * WN * 32 * (NSUB * 32 + 4) * 4; }
};
constexpr int kNumCfgB = 9;
constexpr TileCfgB kCfgB[kNumCfgB] = {
    {2, 1, 2, 2, 3, 64 * 1024, 16, false},          // 128 x 64
    {5, 1, 1, 4, 2, 64 * 1024, 16, false},          // 160 x 128
    {4, 1, 2, 2, 2, 64 * 1024, 16, false},          // 256 x 64
    {5, 2, 1, 2, 2, 80 * 1024, 32, true},           // 160 x 128: two waves, 160x64 register tile each, one wave per SIMD
    // one workgroup per CU, four waves with a 160x64 register tile each and the whole 160 KiB of LDS: the
    // stride-2 layers, whose input tile is 4x the output tile, keep full M tiles this way
    {5, 2, 1, 4, 1, 160 * 1024 - 64, 32, true},     // 160 x 256
    {5, 2, 2, 2, 1, 160 * 1024 - 64, 32, true},     // 320 x 128
    {5, 2, 2, 1, 2, 80 * 1024, 32, true},           // 320 x 64: the 2-wave shape for 64-channel layers
    {4, 2, 1, 2, 2, 80 * 1024, 32, true},           // 128 x 128: 128x64 register tiles where 160-row tiles quantise badly
    {4, 2, 1, 4, 1, 160 * 1024 - 64, 32, true},     // 128 x 256: the same with the whole LDS (three 10x4 maps of the last 5x5 layer)
};

// The latency rows: a register tile of ONE 32 x 32 sub-tile per wave, so a wave issues 3 MFMAs per k-step of a bf16x3
// product where the smallest row above issues 6 -- for launches so small that the chip is nowhere near full and the
// time of the launch is one wave's walk over the contraction.  A table of their own: the planner only looks at them
// under DS_CONV_PLAN_LATENCY (or when one is forced), and `cfg` = kNumCfgB + row.  bf16x3 only; the kernels are the
// launch_nit_b instantiations (256 threads, default LDS), in translation units of their own.
constexpr int kNumCfgBLat = 2;
constexpr TileCfgB kCfgBLat[kNumCfgBLat] = {
    {1, 1, 2, 2, 2, 64 * 1024, 16, true},           // 64 x 64 (the 3x3 instances hold ~210 registers: two waves per SIMD)
    {1, 1, 1, 4, 2, 64 * 1024, 16, true},           // 32 x 128
};
constexpr int kNumCfgBAll = kNumCfgB + kNumCfgBLat;
constexpr const TileCfgB &ds_bf16_cfg(int cfg) { return cfg < kNumCfgB ? kCfgB[cfg] : kCfgBLat[cfg - kNumCfgB]; }

// The pipelined walk (PIPE of the kernel) is built for the rows a launch of less than one wave per SIMD is planned
// onto: the latency rows and the 128 x 64 row of kCfgB.  Its two pixel tiles may take more than a row's lds_cap (which
// sizes ONE tile): the launch opts into the whole LDS, and a workgroup of such a launch has its CU to itself anyway.
constexpr bool ds_bf16_has_pipe(int cfg) { return cfg == 0 || (cfg >= kNumCfgB && cfg < kNumCfgBAll); }
constexpr size_t kLdsCapPipeB = 160 * 1024 - 64;

// one entry point per translation unit (kernel size x arithmetic)
void ds_bf16_launch_k3x3(const PlanB &pl, void *stream);
void ds_bf16_launch_k5x3(const PlanB &pl, void *stream);
void ds_bf16_launch_k3x1(const PlanB &pl, void *stream);
void ds_bf16_launch_k5x1(const PlanB &pl, void *stream);
void ds_bf16_launch_k3x3g(const PlanB &pl, void *stream);      // 3x3 bf16x3 with the BatchNorm-backward epilogue
void ds_bf16_launch_k3x3l(const PlanB &pl, void *stream);      // the latency rows (pl.cfg >= kNumCfgB), bf16x3
void ds_bf16_launch_k5x3l(const PlanB &pl, void *stream);
void ds_bf16_launch_k3x3p(const PlanB &pl, void *stream);      // the pipelined walk (pl.pipe, ds_bf16_has_pipe(pl.cfg)), bf16x3
void ds_bf16_launch_k5x3p(const PlanB &pl, void *stream);

#ifdef DS_BF16_KERNEL_TU
namespace {

// NIT: float4 staging slots per thread (compile time, so all loads of a chunk are issued together);
// PREF: the next chunk's pixels are loaded into registers BEFORE this chunk's matrix work and converted
// / written to LDS after it (small tiles); otherwise they are loaded right after the barrier (big
// tiles, where 16 slots would not fit next to the accumulators).
// BNB: the epilogue is the first half of a BatchNorm backward (see ConvKB): y = (acc [+ res]) * [0 < z*msc+msh < 20]
// and the per-tile partial sums are { sum y, sum y * xhat }, xhat = (z - mean) * invstd, instead of { sum, sum sq }.
// PIPE (bf16x3, register tiles of at most two sub-tiles): the walk for launches that put at most one wave on a SIMD, where
// no other wave covers this one's LDS, barrier and L2 latency.  The pixel tile is double-buffered in LDS: while the taps
// of chunk c read buffer c & 1, the pixels of chunk c + 1 are converted and stored into the other buffer between the
// MFMAs (and the pixels of chunk c + 2 requested into the registers that frees), so one LDS-only barrier per chunk
// replaces two __syncthreads(); the next tap's pixel fragments are fetched in front of this tap's MFMAs and the filter
// ring is refilled behind them.  Every output element is accumulated over the same k-steps in the same term order as
// in the classic walk: the results are the same bits.
template <int KS, int MSUB, int NSUB, int WM, int WN, bool X3, int NIT, bool PREF, bool BNB = false, bool PIPE = false>
__global__ void __launch_bounds__(WM * WN * 64) conv_mfma_bf16_kernel(const ConvKB p) {
    constexpr int NTHR = WM * WN * 64;
    constexpr int MT = MSUB * WM * 32;
    constexpr int NTILE = NSUB * WN * 32;
    constexpr int NT = KS * KS;
    // PIPE, 5x5 with a single sub-tile: a tap is 3 MFMAs (~100 cycles), and a refill 4 taps ahead would be shorter than a
    // filter slice's way from beyond the L2; the ring holds a whole chunk's taps there
    constexpr int RING = (KS == 3) ? (MSUB <= 2 ? 9 : 3) : (KS == 5 ? ((PIPE && MSUB * NSUB == 1) ? 25 : 5) : 1);
    // 160x64 register tiles run one wave per SIMD: nothing else hides LDS latency there, so the next
    // tap's pixel fragments are fetched before (X3: in between) this tap's matrix work
    constexpr bool APREF = (MSUB * NSUB >= 8);
    constexpr bool ILV = X3 && APREF;

    char *lds = (char *)ds_dynamic_lds();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, lhi = lane >> 5;
    const int tile_n = blockIdx.x % p.n_ntiles;
    const int tile_m = blockIdx.x / p.n_ntiles;
    const int seg0 = tile_m * p.NI;
    const int pix_per_seg = p.RT * p.Wc;
    const int tile_pix = p.NI * p.seg_pix;
    // the pixel-tile region doubles as the epilogue's transposition buffers (32 x (NSUB*32+4) floats per wave)
    constexpr int EPI_BYTES = WM * WN * 32 * (NSUB * 32 + 4) * 4;
    const int tile_bytes = (X3 ? 2 : 1) * tile_pix * PSB;
    const int tiles_bytes = (PIPE ? 2 : 1) * tile_bytes;       // PIPE: two pixel tiles, [buffer][hi | lo][tile_pix][PSB]
    const int stage_bytes = tiles_bytes > EPI_BYTES ? tiles_bytes : EPI_BYTES;
    char *lds_hi = lds;                                        // [tile_pix][PSB]
    char *lds_lo = lds + (X3 ? tile_pix * PSB : 0);
    int *out_off = (int *)(lds + stage_bytes);                 // [MT]
    int *seg_lo = out_off + MT;                                // [NI] first in-image row of each segment's tile
    int *seg_cnt = seg_lo + p.NI;                              // [NI] number of in-image rows
    float *red = (float *)(seg_cnt + p.NI);                    // [WM][NTILE][2]

    // the first filter slices are requested before anything else: their latency hides behind the tables
    const int n_chunks = p.Cin / CKB;
    const int n_base = tile_n * NTILE + wn * NSUB * 32;
    const size_t lane_w = ((size_t)(n_base + l31) * CKB + 8 * lhi);      // in bf16 elements
    const size_t w_tap_stride = (size_t)p.Cout * CKB;
    const int last_tap = n_chunks * NT - 1;

    bf16x8 bq_hi[RING][NSUB], bq_lo[X3 ? RING : 1][NSUB];
#pragma unroll
    for (int d = 0; d < RING; ++d)
#pragma unroll
        for (int ns = 0; ns < NSUB; ++ns) {
            const int g = d < last_tap ? d : last_tap;
            const size_t o = lane_w + (size_t)g * w_tap_stride + (size_t)ns * 32 * CKB;
            bq_hi[d][ns] = *(const bf16x8 *)(p.w_hi + o);
            if constexpr (X3) bq_lo[d][ns] = *(const bf16x8 *)(p.w_lo + o);
        }

    const float rcp_pps = 1.0f / (float)pix_per_seg, rcp_wc = 1.0f / (float)p.Wc, rcp_w = 1.0f / (float)p.W,
                rcp_spi = 1.0f / (float)p.segs_per_img;
    for (int seg = tid; seg < p.NI; seg += NTHR) {
        const int gseg = seg0 + seg;
        int lo = 0, cnt = 0;
        if (gseg < p.n_segs) {
            const int b = ds_div_small(gseg, p.segs_per_img, rcp_spi);
            const int h0 = p.IS * (gseg - b * p.segs_per_img) * p.RT + p.dh_min;      // image row of tile row 0
            lo = h0 < 0 ? -h0 : 0;
            const int hi = p.H - h0 < p.rows_in ? p.H - h0 : p.rows_in;
            cnt = hi > lo ? hi - lo : 0;
        }
        seg_lo[seg] = lo;
        seg_cnt[seg] = cnt;
    }

    f32x16 acc[MSUB][NSUB];
#pragma unroll
    for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
        for (int ns = 0; ns < NSUB; ++ns)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ms][ns][r] = 0.0f;

    // ---- staging descriptors (chunk-invariant) of this thread's items: 4 channels of one in-image pixel each.
    // Item idx -> (quarter q, column c, valid row) in segment order; slots past the last item load x[0..3]
    // and drop it into the unused pad bytes of pixel record 0, so the chunk loop has no branches.
    int g_off[NIT], l_off[NIT];
    __syncthreads();                            // seg_lo / seg_cnt are complete
    {
        // a thread's items ascend by NTHR/4 pixels: (row, column) advance incrementally and the segment
        // walk never restarts
        const int q = tid & 3;
        const int dvr = ds_div_small(NTHR / 4, p.W, rcp_w), dc = NTHR / 4 - dvr * p.W;
        int vr = ds_div_small(tid >> 2, p.W, rcp_w);
        int c = (tid >> 2) - vr * p.W;
        int seg = -1, row0 = 0, cnt = 0, lo = 0, img_row = 0;
        auto next_seg = [&]() {
            row0 += cnt;
            ++seg;
            cnt = 0;
            if (seg < p.NI) {
                cnt = seg_cnt[seg];
                lo = seg_lo[seg];
                const int gseg = seg0 + seg;
                const int b = ds_div_small(gseg, p.segs_per_img, rcp_spi);
                img_row = b * p.H + p.IS * (gseg - b * p.segs_per_img) * p.RT + p.dh_min;   // of tile row 0
            }
        };
        next_seg();
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            while (seg < p.NI && vr >= row0 + cnt) next_seg();
            g_off[it] = 0;
            l_off[it] = 32;
            if (seg < p.NI) {
                const int rr = lo + vr - row0;
                // stride-2 layers keep even tile columns in slots [0, half) and odd ones in [half, cols_in),
                // so that the 32 lanes of a fragment read (stride-2 columns) touch CONSECUTIVE records
                const int cc = c - p.dw_min;
                const int pc = (p.IS == 2) ? ((cc & 1) ? p.half + (cc >> 1) : (cc >> 1)) : cc;
                g_off[it] = ((img_row + rr) * p.W + c) * p.Cin + q * 4;
                l_off[it] = (seg * p.seg_pix + rr * p.pitch + pc) * PSB + q * 8;
            }
            c += dc;
            vr += dvr;
            if (c >= p.W) {
                c -= p.W;
                ++vr;
            }
        }
    }
    f32x4 st[NIT];
    if constexpr (PREF) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) st[it] = *(const f32x4 *)(p.x + g_off[it]);
    }
    // ---- everything below overlaps the first chunk's loads ----
    // Only in-image pixels are ever staged: the zero halo (and the row padding) is written once, here.
    for (int i = tid; i < tiles_bytes / 16; i += NTHR) *(f32x4 *)(lds + 16 * i) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int m = tid; m < MT; m += NTHR) {
        const int seg = ds_div_small(m, pix_per_seg, rcp_pps);
        const int rem = m - seg * pix_per_seg;
        const int r = ds_div_small(rem, p.Wc, rcp_wc), c = rem - r * p.Wc;
        const int gseg = seg0 + seg;
        int off = -1;
        if (seg < p.NI && gseg < p.n_segs) {
            const int b = ds_div_small(gseg, p.segs_per_img, rcp_spi);
            const int rr = (gseg - b * p.segs_per_img) * p.RT + r;
            if (rr < p.Hr) off = ((b * p.Ho + p.OS * rr + p.OH0) * p.Wo + p.OS * c + p.OW0) * p.Cout;
        }
        out_off[m] = off;
    }
    const int lpix = ds_mfma_lpix(l31);        // conflict-free service groups of the fragment reads
    int a_off[MSUB];                                           // byte offset of this lane's fragment
#pragma unroll
    for (int ms = 0; ms < MSUB; ++ms) {
        const int m = (wm * MSUB + ms) * 32 + lpix;
        const int seg = ds_div_small(m, pix_per_seg, rcp_pps);
        const int rem = m - seg * pix_per_seg;
        const int r = ds_div_small(rem, p.Wc, rcp_wc), c = rem - r * p.Wc;
        const int pix = (seg < p.NI) ? seg * p.seg_pix + (p.IS * r) * p.pitch + c : 0;
        a_off[ms] = pix * PSB + 16 * lhi;
    }

    // CVI: the next chunk's pixels are split into hi/lo IN PLACE (4 floats -> 4+4 bf16, the same 16 bytes)
    // between the MFMAs of this chunk's later taps; between two chunks only the LDS writes remain.
    constexpr bool CVI = ILV && PREF;
    constexpr int CV_FIRST = 3;                 // taps left for the prefetch to land before conversion starts
    auto split_item = [&](int it) {
        const f32x4 v = st[it];
        bf16x8 pk;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const __bf16 h = (__bf16)v[j];
            pk[j] = h;
            pk[4 + j] = (__bf16)(v[j] - (float)h);
        }
        st[it] = __builtin_bit_cast(f32x4, pk);
    };
    if constexpr (CVI) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) split_item(it);
    }

    if constexpr (PIPE) {
        static_assert(X3 && PREF && !BNB && MSUB * NSUB <= 2 && NT % RING == 0, "the pipelined walk: bf16x3, small register tiles");
        constexpr int NM = 3 * MSUB * NSUB, NR = 2 * NSUB;
        const int plane = tile_pix * PSB;       // the lo records of a tile follow its hi records
        auto tap_off = [&](int tt) {
            const int kw = tt % KS;
            return ((tt / KS) * p.pitch + (p.IS == 2 ? (kw & 1) * p.half + (kw >> 1) : kw)) * PSB;
        };
        // item `it`: the pixels held in st -> hi / lo records of the tile at `buf`; st then takes the item's pixels of
        // chunk cn, which have a whole chunk's matrix work to arrive
        auto put_item = [&](int it, char *buf, int cn) {
            const f32x4 v = st[it];
            bf16x4 h, l;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                h[j] = (__bf16)v[j];
                l[j] = (__bf16)(v[j] - (float)h[j]);
            }
            *(bf16x4 *)(buf + l_off[it]) = h;
            *(bf16x4 *)(buf + plane + l_off[it]) = l;
            st[it] = *(const f32x4 *)(p.x + g_off[it] + cn * CKB);
        };
        __syncthreads();                        // both tiles are zeroed
#pragma unroll
        for (int it = 0; it < NIT; ++it) put_item(it, lds, n_chunks > 1 ? 1 : 0);
        __syncthreads();
        // ONE barrier per chunk, executed by every wave n_chunks times whatever n_chunks is: behind it every wave has
        // read the last fragment of buffer chunk & 1 (the next chunk overwrites it) and has stored its share of the
        // other buffer (the next chunk reads it).  The last chunk stores pixels nobody reads into the free buffer.
        for (int chunk = 0; chunk < n_chunks; ++chunk) {
            const int rd = (chunk & 1) * tile_bytes;
            char *wr = lds + (tile_bytes - rd);
            const int cn = chunk + 2 < n_chunks ? chunk + 2 : n_chunks - 1;
            const int g0 = chunk * NT;
            const char *a_cur[MSUB];
            bf16x8 a_hi[2][MSUB], a_lo[2][MSUB];
#pragma unroll
            for (int ms = 0; ms < MSUB; ++ms) {
                a_cur[ms] = lds + rd + a_off[ms];
                a_lo[0][ms] = *(const bf16x8 *)(a_cur[ms] + plane + tap_off(0));
                a_hi[0][ms] = *(const bf16x8 *)(a_cur[ms] + tap_off(0));
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int slot = t % RING, cur = t & 1, rslot = (t + RING - 1) % RING;
                __builtin_amdgcn_sched_barrier(0);
                // the next tap's fragments: in flight for the three (six) MFMAs of this tap
                if (t + 1 < NT) {
                    const int toff = tap_off(t + 1);
#pragma unroll
                    for (int ms = 0; ms < MSUB; ++ms) a_lo[cur ^ 1][ms] = *(const bf16x8 *)(a_cur[ms] + plane + toff);
#pragma unroll
                    for (int ms = 0; ms < MSUB; ++ms) a_hi[cur ^ 1][ms] = *(const bf16x8 *)(a_cur[ms] + toff);
                }
                int gn = g0 + t - 1 + RING;                 // refills the slot the previous tap consumed
                gn = gn < last_tap ? gn : last_tap;
                const __bf16 *rhi = p.w_hi + lane_w + (size_t)gn * w_tap_stride;
                const __bf16 *rlo = p.w_lo + lane_w + (size_t)gn * w_tap_stride;
                const int i0 = (NIT * t) / NT, i1 = (NIT * (t + 1)) / NT;      // this tap's share of the pixel items
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < NM; ++q) {
                    const int term = q / (MSUB * NSUB), ms = (q % (MSUB * NSUB)) / NSUB, ns = q % NSUB;
                    if (term == 0) acc[ms][ns] = ds_mfma_32x32x16_bf16(bq_hi[slot][ns], a_lo[cur][ms], acc[ms][ns]);
                    else if (term == 1) acc[ms][ns] = ds_mfma_32x32x16_bf16(bq_lo[slot][ns], a_hi[cur][ms], acc[ms][ns]);
                    else acc[ms][ns] = ds_mfma_32x32x16_bf16(bq_hi[slot][ns], a_hi[cur][ms], acc[ms][ns]);
                    if (t > 0 && q < NR) {
                        if (q & 1) bq_lo[rslot][q >> 1] = *(const bf16x8 *)(rlo + (size_t)(q >> 1) * 32 * CKB);
                        else bq_hi[rslot][q >> 1] = *(const bf16x8 *)(rhi + (size_t)(q >> 1) * 32 * CKB);
                    }
#pragma unroll
                    for (int it = i0; it < i1; ++it)
                        if (NR + (it - i0) % (NM - NR) == q) put_item(it, wr, cn);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            {
                int gn = g0 + NT - 1 + RING;
                gn = gn < last_tap ? gn : last_tap;
#pragma unroll
                for (int ns = 0; ns < NSUB; ++ns) {
                    const size_t o = lane_w + (size_t)gn * w_tap_stride + (size_t)ns * 32 * CKB;
                    bq_hi[(NT - 1) % RING][ns] = *(const bf16x8 *)(p.w_hi + o);
                    bq_lo[(NT - 1) % RING][ns] = *(const bf16x8 *)(p.w_lo + o);
                }
            }
            ds_lds_barrier();
        }
    } else                                     // the classic walk: one pixel tile, two barriers per chunk
    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        __syncthreads();                       // previous chunk's fragment reads are done
        if constexpr (!PREF) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) st[it] = *(const f32x4 *)(p.x + g_off[it] + chunk * CKB);
        }
        if constexpr (CVI) {                   // records were split during the previous chunk's taps
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const bf16x8 pk = __builtin_bit_cast(bf16x8, st[it]);
                *(bf16x4 *)(lds_hi + l_off[it]) = __builtin_shufflevector(pk, pk, 0, 1, 2, 3);
                *(bf16x4 *)(lds_lo + l_off[it]) = __builtin_shufflevector(pk, pk, 4, 5, 6, 7);
            }
        } else {
            // ---- convert: f32 pixels -> bf16 hi (+ lo) records ----
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const f32x4 v = st[it];
                bf16x4 h;
#pragma unroll
                for (int j = 0; j < 4; ++j) h[j] = (__bf16)v[j];
                *(bf16x4 *)(lds_hi + l_off[it]) = h;
                if constexpr (X3) {
                    bf16x4 l;
#pragma unroll
                    for (int j = 0; j < 4; ++j) l[j] = (__bf16)(v[j] - (float)h[j]);
                    *(bf16x4 *)(lds_lo + l_off[it]) = l;
                }
            }
        }
        __syncthreads();
        if constexpr (PREF) {                  // next chunk's pixels fly while this one computes
            const int cn = chunk + 1 < n_chunks ? chunk + 1 : chunk;
#pragma unroll
            for (int it = 0; it < NIT; ++it) st[it] = *(const f32x4 *)(p.x + g_off[it] + cn * CKB);
        }
        const int g0 = chunk * NT;
        bf16x8 a_hi[APREF ? 2 : 1][MSUB], a_lo[APREF ? 2 : 1][X3 ? MSUB : 1];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if constexpr (ILV) {
                // One wave per SIMD: nothing but this wave's own instruction order hides the LDS / L2
                // latency, so the next tap's fragment reads and the ring refills are dealt out between
                // PAIRS of MFMAs (each MFMA holds the matrix pipe for 8 issue slots) instead of in a
                // block in front of them.
                constexpr int NM = 3 * MSUB * NSUB, NA = 2 * MSUB, NL = NA + 2 * NSUB;
                const int slot = t % RING, cur = t & 1;
                auto tap_off = [&](int tt) {
                    const int kw = tt % KS;
                    return ((tt / KS) * p.pitch + (p.IS == 2 ? (kw & 1) * p.half + (kw >> 1) : kw)) * PSB;
                };
                if (t == 0) {
                    const int toff = tap_off(0);
#pragma unroll
                    for (int ms = 0; ms < MSUB; ++ms) {
                        a_lo[0][ms] = *(const bf16x8 *)(lds_lo + a_off[ms] + toff);
                        a_hi[0][ms] = *(const bf16x8 *)(lds_hi + a_off[ms] + toff);
                    }
                }
                const bool more = t + 1 < NT;
                const char *nlo = lds_lo + tap_off(more ? t + 1 : t);
                const char *nhi = lds_hi + tap_off(more ? t + 1 : t);
                int gn = g0 + t - 1 + RING;                 // refills the slot the previous tap consumed
                gn = gn < last_tap ? gn : last_tap;
                const int rslot = (t + RING - 1) % RING;
                const __bf16 *rhi = p.w_hi + lane_w + (size_t)gn * w_tap_stride;
                const __bf16 *rlo = p.w_lo + lane_w + (size_t)gn * w_tap_stride;
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < NM; ++q) {
                    const int term = q / (MSUB * NSUB), ms = (q % (MSUB * NSUB)) / NSUB, ns = q % NSUB;
                    if (term == 0) acc[ms][ns] = ds_mfma_32x32x16_bf16(bq_hi[slot][ns], a_lo[cur][ms], acc[ms][ns]);
                    else if (term == 1) acc[ms][ns] = ds_mfma_32x32x16_bf16(bq_lo[slot][ns], a_hi[cur][ms], acc[ms][ns]);
                    else acc[ms][ns] = ds_mfma_32x32x16_bf16(bq_hi[slot][ns], a_hi[cur][ms], acc[ms][ns]);
                    if constexpr (CVI) {
                        if (!(q & 1) && t >= CV_FIRST) {          // one pixel item split per even slot
                            constexpr int SPAN = NT - CV_FIRST;
                            const int it = (NIT * (t - CV_FIRST)) / SPAN + (q >> 1);
                            if (it < (NIT * (t - CV_FIRST + 1)) / SPAN) {
                                split_item(it);
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                    }
                    if (q & 1) {
                        const int l = q >> 1;
                        if (l < NA) {
                            if (more) {
                                const int lm = l % MSUB;
                                if (l < MSUB) a_lo[cur ^ 1][lm] = *(const bf16x8 *)(nlo + a_off[lm]);
                                else a_hi[cur ^ 1][lm] = *(const bf16x8 *)(nhi + a_off[lm]);
                            }
                        } else if (l < NL) {
                            const int ln = (l - NA) >> 1;
                            if (t > 0) {
                                if ((l - NA) & 1) bq_lo[rslot][ln] = *(const bf16x8 *)(rlo + (size_t)ln * 32 * CKB);
                                else bq_hi[rslot][ln] = *(const bf16x8 *)(rhi + (size_t)ln * 32 * CKB);
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                continue;
            }
            const int slot = t % RING;
            if (t > 0) {                       // refill the slot the previous tap consumed
                int gn = g0 + t - 1 + RING;
                gn = gn < last_tap ? gn : last_tap;
#pragma unroll
                for (int ns = 0; ns < NSUB; ++ns) {
                    const size_t o = lane_w + (size_t)gn * w_tap_stride + (size_t)ns * 32 * CKB;
                    bq_hi[(t - 1) % RING][ns] = *(const bf16x8 *)(p.w_hi + o);
                    if constexpr (X3) bq_lo[(t - 1) % RING][ns] = *(const bf16x8 *)(p.w_lo + o);
                }
            }
            auto tap_off = [&](int tt) {
                const int kw = tt % KS;
                return ((tt / KS) * p.pitch + (p.IS == 2 ? (kw & 1) * p.half + (kw >> 1) : kw)) * PSB;
            };
            const int cur = APREF ? (t & 1) : 0;
            if (!APREF || t == 0) {
                const int toff = tap_off(t);
#pragma unroll
                for (int ms = 0; ms < MSUB; ++ms) {
                    a_hi[cur][ms] = *(const bf16x8 *)(lds_hi + a_off[ms] + toff);
                    if constexpr (X3) a_lo[cur][ms] = *(const bf16x8 *)(lds_lo + a_off[ms] + toff);
                }
            }
            if constexpr (APREF) {
                if (t + 1 < NT) {
                    const int toff = tap_off(t + 1);
#pragma unroll
                    for (int ms = 0; ms < MSUB; ++ms) {
                        a_hi[cur ^ 1][ms] = *(const bf16x8 *)(lds_hi + a_off[ms] + toff);
                        if constexpr (X3) a_lo[cur ^ 1][ms] = *(const bf16x8 *)(lds_lo + a_off[ms] + toff);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            // term-major order: consecutive MFMAs always hit DIFFERENT accumulators (a dependent
            // accumulate chain stalls the matrix pipe); small cross terms first, the leading term last
            if constexpr (X3) {
#pragma unroll
                for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
                    for (int ns = 0; ns < NSUB; ++ns)
                        acc[ms][ns] = ds_mfma_32x32x16_bf16(bq_hi[slot][ns], a_lo[cur][ms], acc[ms][ns]);
#pragma unroll
                for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
                    for (int ns = 0; ns < NSUB; ++ns)
                        acc[ms][ns] = ds_mfma_32x32x16_bf16(bq_lo[slot][ns], a_hi[cur][ms], acc[ms][ns]);
            }
#pragma unroll
            for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
                for (int ns = 0; ns < NSUB; ++ns)
                    acc[ms][ns] = ds_mfma_32x32x16_bf16(bq_hi[slot][ns], a_hi[cur][ms], acc[ms][ns]);
            __builtin_amdgcn_sched_barrier(0);
        }
        {
            int gn = g0 + NT - 1 + RING;
            gn = gn < last_tap ? gn : last_tap;
#pragma unroll
            for (int ns = 0; ns < NSUB; ++ns) {
                const size_t o = lane_w + (size_t)gn * w_tap_stride + (size_t)ns * 32 * CKB;
                bq_hi[(NT - 1) % RING][ns] = *(const bf16x8 *)(p.w_hi + o);
                if constexpr (X3) bq_lo[(NT - 1) % RING][ns] = *(const bf16x8 *)(p.w_lo + o);
            }
        }
    }

    // ---- epilogue ----
    // The filters were the A operand of every MFMA, so the accumulators hold the TRANSPOSED product: a lane
    // owns one output pixel (l31 of the 32-pixel sub-tile) and, per register quad g, four consecutive output
    // channels 8g + 4*lhi .. +3.  Each 32-pixel sub-tile is turned around through a wave-private LDS buffer
    // (the pixel tile's space, free now) so that residual loads and stores move whole pixel rows: the
    // NSUB*32 channels of a pixel are contiguous across NSUB*8 lanes, 16 bytes per lane.
    constexpr int TP = NSUB * 32 + 4;           // buffer row pitch in floats (conflict-free 16-byte writes)
    constexpr int LPP = NSUB * 8;               // lanes per pixel row
    constexpr int PPI = 64 / LPP;               // pixel rows per instruction
    constexpr int NRI = 32 / PPI;               // instructions per sub-tile
    const int flags = p.flags;
    __syncthreads();                            // every wave is done reading the pixel tile
    float *tb = (float *)lds + wave * (32 * TP);
    const int my_c = (lane % LPP) * 4, my_p = lane / LPP;
    const int col = n_base + my_c;
    f32x4 sc4 = {1.0f, 1.0f, 1.0f, 1.0f}, sh4 = {0.0f, 0.0f, 0.0f, 0.0f};
    if (flags & DS_EPI_AFFINE) {
        sc4 = *(const f32x4 *)(p.scale + col);
        sh4 = *(const f32x4 *)(p.shift + col);
    }
    // Rows of a ragged tile get an out-of-range buffer offset (the store is dropped, the load returns
    // zeros) and a layer without residual reads "out of range" too: no branch around any memory
    // instruction, so the waits on the residual rows never include the stores issued in between.
    const ds_buffer ybuf = ds_make_buffer(p.y, p.y_bytes);
    const ds_buffer rbuf = ds_make_buffer((flags & DS_EPI_RESIDUAL) ? (const void *)p.res : (const void *)p.y,
                                          (flags & DS_EPI_RESIDUAL) ? p.y_bytes : 0u);
    float ps1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ps2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    unsigned voff[2][NRI];
    f32x4 resv[2][NRI];
    f32x4 zv[BNB ? 2 : 1][BNB ? NRI : 1];
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 mu4 = zero4, is4 = zero4, msc4 = zero4, msh4 = zero4;
    const ds_buffer zbuf = ds_make_buffer(BNB ? (const void *)p.bn_z : (const void *)p.y, BNB ? p.y_bytes : 0u);
    if constexpr (BNB) {
        const size_t mo = (size_t)(tile_m / p.bn_mtiles) * p.Cout + col;      // this tile's member of the batch
        mu4 = *(const f32x4 *)(p.bn_mean + mo);
        is4 = *(const f32x4 *)(p.bn_invstd + mo);
        if (p.bn_msc) {
            msc4 = *(const f32x4 *)(p.bn_msc + mo);
            msh4 = *(const f32x4 *)(p.bn_msh + mo);
        }
    }
    const bool mask_from_res = BNB && p.bn_msc == nullptr;
    auto fetch_rows = [&](int ms, int buf) {    // byte offsets and residual rows of sub-tile ms
#pragma unroll
        for (int k = 0; k < NRI; ++k) {
            const int off = out_off[(wm * MSUB + ms) * 32 + k * PPI + my_p];
            voff[buf][k] = off >= 0 ? (unsigned)(off + col) * 4u : DS_BUFFER_OOB;
        }
#pragma unroll
        for (int k = 0; k < NRI; ++k) resv[buf][k] = ds_buffer_load_f32x4(rbuf, voff[buf][k]);
        if constexpr (BNB) {
#pragma unroll
            for (int k = 0; k < NRI; ++k) zv[buf][k] = ds_buffer_load_f32x4(zbuf, voff[buf][k]);
        }
    };
    fetch_rows(0, 0);
#pragma unroll
    for (int ms = 0; ms < MSUB; ++ms) {
        const int cb = ms & 1;
        if (ms + 1 < MSUB) fetch_rows(ms + 1, cb ^ 1);
#pragma unroll
        for (int ns = 0; ns < NSUB; ++ns)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = acc[ms][ns][4 * g + j];
                *(f32x4 *)(tb + lpix * TP + ns * 32 + 8 * g + 4 * lhi) = v;
            }
        ds_wave_sync();
#pragma unroll
        for (int k = 0; k < NRI; ++k) {
            f32x4 v = *(const f32x4 *)(tb + (k * PPI + my_p) * TP + my_c);
            const bool live = voff[cb][k] != DS_BUFFER_OOB;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float t = v[j];
                if constexpr (BNB) {
                    // the layer's clipped-ReLU mask from its own pre-activation (the fma bn_apply_kernel evaluates)
                    const float zz = zv[cb][k][j];
                    const float rr = resv[cb][k][j];
                    const float am = mask_from_res ? rr : ds_bn_affine(zz, msc4[j], msh4[j]);
                    t += mask_from_res ? 0.0f : rr;
                    t = (am > 0.0f && am < 20.0f) ? t : 0.0f;
                    ps1[j] += live ? t : 0.0f;
                    ps2[j] += live ? t * ((zz - mu4[j]) * is4[j]) : 0.0f;
                    v[j] = t;
                    continue;
                }
                if (flags & DS_EPI_STATS) {
                    ps1[j] += live ? t : 0.0f;
                    ps2[j] += live ? t * t : 0.0f;
                }
                t = t * sc4[j] + sh4[j];
                t += resv[cb][k][j];
                if (flags & DS_EPI_CLIP) t = fminf(fmaxf(t, 0.0f), 20.0f);
                v[j] = t;
            }
            ds_buffer_store_f32x4(ybuf, voff[cb][k], v);
        }
        ds_wave_sync();                         // the buffer is rewritten by the next sub-tile
    }
    if (flags & DS_EPI_STATS) {
        // per-channel sums over this wave's pixels: fold the PPI lane groups that share a channel quad
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int mk = LPP; mk < 64; mk <<= 1) {
                ps1[j] += ds_shfl_xor(ps1[j], mk);
                ps2[j] += ds_shfl_xor(ps2[j], mk);
            }
            if (my_p == 0) {
                const int c = wn * NSUB * 32 + my_c + j;
                red[(wm * NTILE + c) * 2 + 0] = ps1[j];
                red[(wm * NTILE + c) * 2 + 1] = ps2[j];
            }
        }
        __syncthreads();
        for (int c = tid; c < NTILE; c += NTHR) {
            float a1 = 0.0f, a2 = 0.0f;
            for (int k = 0; k < WM; ++k) {
                a1 += red[(k * NTILE + c) * 2 + 0];
                a2 += red[(k * NTILE + c) * 2 + 1];
            }
            size_t row = tile_m;
            if constexpr (BNB) row = (size_t)(tile_m / p.bn_mtiles) * p.bn_rows_member + p.bn_row0 + tile_m % p.bn_mtiles;
            float *dst = p.stats + (row * p.Cout + tile_n * NTILE + c) * 2;
            dst[0] = a1;
            dst[1] = a2;
        }
    }
}

template <int KS, int MSUB, int NSUB, int WM, int WN, bool X3, bool BNB = false>
static void launch_nit_b(const PlanB &pl, void *stream) {
    if (pl.nit <= 4)
        DS_LAUNCH((conv_mfma_bf16_kernel<KS, MSUB, NSUB, WM, WN, X3, 4, true, BNB>), pl.grid, 256, pl.lds_bytes, stream, pl.k);
    else if (pl.nit <= 8)      // register-prefetch the next chunk where the accumulators leave room (MSUB <= 4)
        DS_LAUNCH((conv_mfma_bf16_kernel<KS, MSUB, NSUB, WM, WN, X3, 8, (MSUB <= 4), BNB>), pl.grid, 256, pl.lds_bytes, stream, pl.k);
    else
        DS_LAUNCH((conv_mfma_bf16_kernel<KS, MSUB, NSUB, WM, WN, X3, 16, false, BNB>), pl.grid, 256, pl.lds_bytes, stream, pl.k);
}

template <int KS, int MSUB, int NSUB, int WM, int WN, bool BNB = false>
static void launch_big_b(const PlanB &pl, void *stream) {
    constexpr int NTHR = WM * WN * 64;
    if (pl.nit <= 8)
        DS_LAUNCH_BIG_LDS((conv_mfma_bf16_kernel<KS, MSUB, NSUB, WM, WN, true, 8, true, BNB>), pl.grid, NTHR, pl.lds_bytes, stream, pl.k);
    else if (pl.nit <= 16)
        DS_LAUNCH_BIG_LDS((conv_mfma_bf16_kernel<KS, MSUB, NSUB, WM, WN, true, 16, true, BNB>), pl.grid, NTHR, pl.lds_bytes, stream, pl.k);
    else
        DS_LAUNCH_BIG_LDS((conv_mfma_bf16_kernel<KS, MSUB, NSUB, WM, WN, true, 32, false, BNB>), pl.grid, NTHR, pl.lds_bytes, stream, pl.k);
}

// run-time cfg -> compile-time row: f(std::integral_constant<int, cfg>)
template <int N = 0, class F>
static void ds_bf16_with_cfg(int cfg, F &&f) {
    if constexpr (N < kNumCfgB) {
        if (cfg == N) f(std::integral_constant<int, N>{});
        else ds_bf16_with_cfg<N + 1>(cfg, f);
    }
}

template <int KS, bool X3, bool BNB = false>
static void launch_b(const PlanB &pl, void *stream) {
    ds_bf16_with_cfg(pl.cfg, [&](auto c) {
        constexpr TileCfgB cf = kCfgB[decltype(c)::value];
        if constexpr (!cf.x3_only) launch_nit_b<KS, cf.MSUB, cf.NSUB, cf.WM, cf.WN, X3, BNB>(pl, stream);
        else if constexpr (X3) launch_big_b<KS, cf.MSUB, cf.NSUB, cf.WM, cf.WN, BNB>(pl, stream);
    });
}

// the same for the latency rows: pl.cfg - kNumCfgB -> row of kCfgBLat
template <int KS, int N = 0>
static void launch_lat_b(const PlanB &pl, void *stream) {
    if constexpr (N < kNumCfgBLat) {
        constexpr TileCfgB cf = kCfgBLat[N];
        static_assert(cf.NTHR() == 256, "launch_nit_b launches 256 threads");
        if (pl.cfg - kNumCfgB == N) launch_nit_b<KS, cf.MSUB, cf.NSUB, cf.WM, cf.WN, true>(pl, stream);
        else launch_lat_b<KS, N + 1>(pl, stream);
    }
}

// the pipelined walk of one row: always with the register prefetch, whatever the items per thread (the launch has a
// SIMD's whole register file to itself)
template <int KS, int MSUB, int NSUB, int WM, int WN>
static void launch_pipe_nit_b(const PlanB &pl, void *stream) {
    static_assert(WM * WN * 64 == 256, "256 threads");
    if (pl.nit <= 4)
        DS_LAUNCH_BIG_LDS((conv_mfma_bf16_kernel<KS, MSUB, NSUB, WM, WN, true, 4, true, false, true>), pl.grid, 256, pl.lds_bytes, stream, pl.k);
    else if (pl.nit <= 8)
        DS_LAUNCH_BIG_LDS((conv_mfma_bf16_kernel<KS, MSUB, NSUB, WM, WN, true, 8, true, false, true>), pl.grid, 256, pl.lds_bytes, stream, pl.k);
    else
        DS_LAUNCH_BIG_LDS((conv_mfma_bf16_kernel<KS, MSUB, NSUB, WM, WN, true, 16, true, false, true>), pl.grid, 256, pl.lds_bytes, stream, pl.k);
}

// pl.cfg -> the rows of ds_bf16_has_pipe
template <int KS>
static void launch_pipe_b(const PlanB &pl, void *stream) {
    constexpr TileCfgB c0 = kCfgB[0], l0 = kCfgBLat[0], l1 = kCfgBLat[1];
    static_assert(kNumCfgBLat == 2 && ds_bf16_has_pipe(0) && ds_bf16_has_pipe(kNumCfgB) && ds_bf16_has_pipe(kNumCfgB + 1), "");
    if (pl.cfg == 0) launch_pipe_nit_b<KS, c0.MSUB, c0.NSUB, c0.WM, c0.WN>(pl, stream);
    else if (pl.cfg == kNumCfgB) launch_pipe_nit_b<KS, l0.MSUB, l0.NSUB, l0.WM, l0.WN>(pl, stream);
    else if (pl.cfg == kNumCfgB + 1) launch_pipe_nit_b<KS, l1.MSUB, l1.NSUB, l1.WM, l1.WN>(pl, stream);
}

}  // namespace
#endif
