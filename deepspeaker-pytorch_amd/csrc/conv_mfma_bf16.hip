// conv_mfma_bf16.hip -- implicit-GEMM convolution on the gfx950 bf16 matrix cores
// (v_mfma_f32_32x32x16_bf16, f32 accumulate), the throughput variants of conv_mfma_f32.hip for the
// forward convolutions of reference model.py:69,73,192,197,202 (+ the same fused BatchNorm-affine /
// residual / clipped-ReLU epilogue, model.py:70-80,188-205).
//
//   X3 = false ("bf16"):   one MFMA per k-step, operands rounded to bf16.  ~8 bits of mantissa: the
//                          embedding drifts ~6e-3 from the reference -- a speed mode.
//   X3 = true  ("bf16x3"): every f32 operand is split x = hi + lo (two bf16) and the product is taken
//                          as hi*hi + hi*lo + lo*hi on the matrix cores -- f32-class accuracy (~1e-5
//                          relative per term) at up to 1/3 of the bf16 peak, i.e. > 5x the f32-MFMA rate.
//
// Activations stay f32 channels-last in HBM; they are converted (and split) while being staged into
// LDS, so the kernel is a drop-in for ds_conv_fwd_f32.  Tiling / segment / halo logic is the same as the
// f32 kernel's (see that file); differences: 16 input channels per chunk (= one MFMA k-step per tap),
// LDS pixel records of 16 bf16 (+16 B pad, conflict-free ds_read_b128), no register prefetch of the
// activation tile (two workgroups per CU overlap staging with the other's matrix work).
#include <ds_device.h>
#include <algorithm>
#include "ds_common.h"

#include "conv_mfma_bf16_kernel.h"
#include "conv_plan.h"

namespace {

// OIHW f32 -> [Cin/16][tap][Cout][16] bf16 hi (+ lo = bf16(w - hi))
// dgrad != 0: the transposed, spatially flipped bank of the stride-1 data gradient (N = Cin, K = Cout)
__device__ __forceinline__ void pack_conv_weight_bf16_body(const float *w, __bf16 *hi, __bf16 *lo, int Cout, int Cin, int KS,
                                                           int dgrad, int block, int n_blocks) {
    const int T = KS * KS;
    const long long n = (long long)Cout * Cin * T;
    const int N = dgrad ? Cin : Cout;
    for (long long i = (long long)block * 256 + threadIdx.x; i < n; i += (long long)n_blocks * 256) {
        const int kk = (int)(i & 15);
        long long r = i >> 4;
        const int nn = (int)(r % N);
        r /= N;
        const int t = (int)(r % T);
        const int kc = (int)(r / T);
        const int k = kc * 16 + kk;
        const int tt = dgrad ? (T - 1 - t) : t;
        const int kh = tt / KS, kw = tt - kh * KS;
        const int co = dgrad ? k : nn, ci = dgrad ? nn : k;
        const float v = w[(((size_t)co * Cin + ci) * KS + kh) * KS + kw];
        const __bf16 h = (__bf16)v;
        hi[i] = h;
        if (lo) lo[i] = (__bf16)(v - (float)h);
    }
}

__global__ void __launch_bounds__(256) pack_conv_weight_bf16_kernel(const float *w, __bf16 *hi, __bf16 *lo, int Cout,
                                                                    int Cin, int KS, int dgrad) {
    pack_conv_weight_bf16_body(w, hi, lo, Cout, Cin, KS, dgrad, (int)blockIdx.x, (int)gridDim.x);
}

// all filters of a weight version in one launch: job j owns the workgroups [first[j], first[j + 1])
struct PackBatchB {
    const float *w[DS_PACK_BATCH_MAX];
    __bf16 *hi[DS_PACK_BATCH_MAX], *lo[DS_PACK_BATCH_MAX];
    int Cout[DS_PACK_BATCH_MAX], Cin[DS_PACK_BATCH_MAX], KS[DS_PACK_BATCH_MAX], dgrad[DS_PACK_BATCH_MAX];
    int first[DS_PACK_BATCH_MAX + 1];
    int n;
};

__global__ void __launch_bounds__(256) pack_conv_weight_bf16_batch_kernel(const PackBatchB J) {
    int j = 0;
    while (j + 1 < J.n && (int)blockIdx.x >= J.first[j + 1]) ++j;
    pack_conv_weight_bf16_body(J.w[j], J.hi[j], J.lo[j], J.Cout[j], J.Cin[j], J.KS[j], J.dgrad[j], (int)blockIdx.x - J.first[j],
                               J.first[j + 1] - J.first[j]);
}

// LDS cycles (1 = conflict-free) of one ds_read_b128 fragment read for a candidate row pitch: simulates
// the two 16-lane service groups of lanes 0..31 (the upper half-wave behaves identically; each group
// holds 16 consecutive pixels, see `lpix` in the kernel) over every 32-row sub-tile of the M tile.  Bank slot of a record = (record * PSB / 16) mod 16.
// NOT the fp16 planner's function of the same name: that one serves lanes reading the same address together and maps
// the pixels past the tile's last segment with ds_f16_frag_pixel, as its kernels do; this kernel does neither.
static double frag_read_cost(int MT, int NI, int RT, int Wc, int IS, int rows_in, int pitch) {
    const int pix_per_seg = RT * Wc, seg_pix = rows_in * pitch;
    double total = 0.0;
    int n = 0;
    for (int m0 = 0; m0 + 32 <= MT; m0 += 32) {
        for (int g = 0; g < 2; ++g) {
            int cnt[16] = {0};
            int worst = 0;
            for (int j = 0; j < 16; ++j) {
                const int m = m0 + 16 * g + j;       // the lane -> pixel permutation makes a group's pixels consecutive
                const int seg = m / pix_per_seg, rem = m % pix_per_seg;
                const int r = rem / Wc, c = rem % Wc;
                const int rec = (seg < NI) ? seg * seg_pix + (IS * r) * pitch + c : 0;
                const int slot = (rec * (PSB / 16)) & 15;
                if (++cnt[slot] > worst) worst = cnt[slot];
            }
            total += worst;
            ++n;
        }
    }
    return n ? total / n : 1.0;
}

// ---- host-side plan: the shared tile search (conv_plan.h) over the rows of kCfgB (conv_mfma_bf16_kernel.h) ----
static int g_forced_cfg_b = -1;      // tuning hook (tools/bf16_cfg_ab.py): plan with this tile configuration only
static int g_walk_b = 0;             // tuning hook (ds_conv_bf16_set_walk): 0 = the planner's choice, 1 = classic, 2 = pipelined

// what a caller of plan_bf16 lets it choose from beyond the rows of kCfgB
constexpr int kPlanLatRows = 1;      // the caller can launch a latency row (kCfgBLat): the forced-configuration hook may name one
constexpr int kPlanLatency = 2;      // DS_CONV_PLAN_LATENCY: plan a launch that leaves the chip short of waves for its latency

// LDS of a launch whose pixel tile holds tile_pix records: the tile (hi + lo planes for bf16x3), which the epilogue's
// buffers alias, then the out_off [MT], seg_lo / seg_cnt [NI] and statistics [WM][NTILE][2] tables.  The launch asks
// for kLdsSlackB bytes more than this; the configurations' caps are compared against this figure.
constexpr size_t kLdsSlackB = 16;
// The pipelined walk (`pipe`) holds two such tiles.
static size_t plan_lds_bytes(const TileCfgB &cf, size_t tile_pix, bool x3, int NI, bool pipe = false) {
    return std::max(tile_pix * PSB * (x3 ? 2 : 1) * (pipe ? 2 : 1), cf.epi_bytes()) + (size_t)cf.MT() * 4 + (size_t)NI * 8 +
           (size_t)cf.WM * cf.NTILE() * 8;
}

// `s` describes the tile grid: input [B,H,W,Cin], KS x KS taps, stride s->stride, output grid Ho x Wo computed
// with `pad`.  The forward convolution writes that grid densely; the stride-2 data gradient runs four such
// grids (parity classes) whose outputs interleave in y (out_* arguments).
//
// mode & kPlanLatency (bf16x3 forward launches only): the search above is run first, and its plan stands wherever it puts
// at least one wave on every SIMD of the chip -- such a launch is bound by throughput, which is what that search and
// its tie-breaks were tuned for (so the plans of a 768-utterance batch are the same with and without the flag).  A
// smaller launch takes as long as one wave's walk over the contraction, so the rows of kCfgB AND kCfgBLat are searched
// again for the least
//     (rounds the launch needs: its waves over the chip's SIMDs, rounded up) x (MFMAs of a wave per k-step)
// -- waves that share a SIMD share its matrix pipe, so a round is one wave per SIMD.  Ties go to the larger tile, then
// to the fewer workgroups (fuller tiles: less filter traffic and fewer CUs taken from whatever runs next to the launch
// for the same latency), then to the first search's objective.  Every row
// accumulates an output element over the same k-steps in the same order (hi*lo, lo*hi, hi*hi per step), so the choice
// of row never changes a bit of the result.
//
// The walk: exactly the launches the flag re-plans -- bf16x3 forward launches that put less than one wave on every SIMD
// -- take the pipelined walk of the kernel (PIPE; same bits again) where the planned row has one (ds_bf16_has_pipe) and
// its two pixel tiles fit the LDS; every other launch keeps the classic walk.  ds_conv_bf16_set_walk(1) keeps it
// everywhere; (2) asks for the pipelined walk in every bf16x3 forward launch and is an error
// (DS_ERR_UNSUPPORTED), not a silent classic walk, where the row has none or the tiles do not fit.
static int plan_bf16(PlanB &pl, const ds_conv_shape *s, bool x3, int out_stride = 1, int out_h0 = 0, int out_w0 = 0,
                     int out_H = 0, int out_W = 0, int grid_H = 0, int grid_W = 0, int mode = 0) {
    int Ho, Wo;
    const int rc = ds_plan_check_shape(s, CKB, false, Ho, Wo, grid_H, grid_W);
    if (rc != DS_OK) return rc;
    const int pad = s->KS / 2;
    const int yH = out_H > 0 ? out_H : Ho, yW = out_W > 0 ? out_W : Wo;
    DS_REQUIRE((long long)s->B * Ho < (1ll << 24), DS_ERR_BAD_SHAPE);                  // reciprocal index arithmetic
    DS_REQUIRE((long long)s->B * yH * yW * s->Cout < (1ll << 30), DS_ERR_BAD_SHAPE);   // 32-bit byte offsets
    const int IS = s->stride;
    double best = -1.0;
    int bc = -1, brt = 0, bni = 0;
    long long bwaves = 0, bcost = 0, bblocks = 0;
    bool latency = false;           // the second search
    auto search = [&](int c) {
        const TileCfgB &cf = ds_bf16_cfg(c);
        if (s->Cout % cf.NTILE()) return;
        if (cf.x3_only && !x3) return;
        if (g_forced_cfg_b >= 0 && c != g_forced_cfg_b) return;
        const long long item_cap = (long long)cf.items_per_thread * cf.NTHR();
        // feasibility with the widest row pitch the conflict search may pick (cols_in + 4); the pitch itself is chosen
        // once, for the winning geometry (this function runs on every launch).  Staged items: 4-channel quarters of
        // the in-image pixels only
        auto fits = [&](int n, int rows_in, int cols_in) {
            return plan_lds_bytes(cf, (size_t)n * rows_in * (cols_in + 4), x3, n) <= cf.lds_cap &&
                   (long long)n * std::min(rows_in, s->H) * s->W * (CKB / 4) <= item_cap;
        };
        ds_plan_segmentations(s->B, Ho, Wo, cf.MT(), IS, s->KS, s->KS, fits, [&](int rt, int ni, long long n_mt) {
            const long long blocks = n_mt * (s->Cout / cf.NTILE());
            double eff = ds_plan_fill_occupancy(s->B, Ho, Wo, n_mt, cf.MT(), blocks, cf.wg_per_cu);
            // a launch with fewer waves than the chip has SIMDs leaves matrix cores idle: 256 two-wave workgroups (the
            // 10x4 layers of one 256-utterance member) ran 156 us where 256 four-wave ones ran 128 (tools/conv_bf16_ab.py)
            const long long waves = blocks * (cf.NTHR() / 64);
            if (waves < kPlanSIMDs) eff *= (double)waves / (double)kPlanSIMDs;
            // ties: 160x64 register tiles first; for 64 output channels the four-wave 256x64 tile beats the two-wave
            // 320x64 one (same tool: 484 against 525 us at 768 utterances, 173 against 185 at 256)
            int pref[kNumCfgBAll] = {0, 2, 7, 8, 5, 6, 1, 4, 3, 0, 0};
#ifdef DS_BF16_PREF_TOP
            pref[DS_BF16_PREF_TOP] = 9;                               // A/B builds (tools/conv_bf16_ab.py): another tie-break
#endif
            eff += 1e-9 * rt + 1e-6 * pref[c];
            bool better = eff > best;
            const long long cost = ds_ceil_div_ll(waves, kPlanSIMDs) * ((x3 ? 3 : 1) * cf.MSUB * cf.NSUB);
            if (latency && bc >= 0) {
                const TileCfgB &bf = ds_bf16_cfg(bc);
                const int area = cf.MT() * cf.NTILE(), barea = bf.MT() * bf.NTILE();
                if (cost != bcost) better = cost < bcost;
                else if (area != barea) better = area > barea;
                else if (blocks != bblocks) better = blocks < bblocks;
            }
            if (better) { best = eff; bc = c; brt = rt; bni = ni; bwaves = waves; bcost = cost; bblocks = blocks; }
        });
    };
    const bool forced_lat = (mode & kPlanLatRows) && g_forced_cfg_b >= kNumCfgB;
    for (int c = 0; c < (forced_lat ? kNumCfgBAll : kNumCfgB); ++c) search(c);
    const bool sub_chip = (mode & kPlanLatency) && x3 && bc >= 0 && bwaves < kPlanSIMDs;
    if (sub_chip && g_forced_cfg_b < 0) {
        latency = true;
        best = -1.0;
        bc = -1;
        for (int c = 0; c < kNumCfgBAll; ++c) search(c);
    }
    if (bc < 0) return DS_ERR_UNSUPPORTED;
    const TileCfgB &cf = ds_bf16_cfg(bc);
    ConvKB &k = pl.k;
    k.H = s->H; k.W = s->W; k.Cin = s->Cin;
    k.Hr = Ho; k.Wc = Wo; k.Ho = yH; k.Wo = yW; k.Cout = s->Cout;
    k.OS = out_stride; k.OH0 = out_h0; k.OW0 = out_w0;
    k.IS = IS; k.dh_min = -pad; k.dw_min = -pad;
    pl.cfg = bc;
    ds_plan_fill_geometry(pl, s->B, Ho, Wo, IS, s->KS, s->KS, s->Cout, cf.NTILE(), brt, bni);
    k.half = (k.cols_in + 1) / 2;
    // row pitch: the cheapest fragment read among cols_in .. cols_in+4 records per row
    int best_pitch = k.cols_in;
    double best_cost = 1e30;
    for (int pt = k.cols_in; pt <= k.cols_in + 4; ++pt) {
        const double c = frag_read_cost(cf.MT(), bni, brt, Wo, IS, k.rows_in, pt);
        if (c < best_cost - 1e-9) { best_cost = c; best_pitch = pt; }
    }
    k.pitch = best_pitch;
    k.seg_pix = k.rows_in * k.pitch;
    k.y_bytes = (unsigned)((long long)s->B * yH * yW * s->Cout * 4);
    pl.pipe = 0;
    if (x3 && (mode & kPlanLatRows) && (g_walk_b == 2 || (g_walk_b == 0 && sub_chip))) {
        const bool can = ds_bf16_has_pipe(bc) && plan_lds_bytes(cf, (size_t)k.NI * k.seg_pix, true, k.NI, true) + kLdsSlackB <= kLdsCapPipeB;
        if (!can && g_walk_b == 2) return DS_ERR_UNSUPPORTED;
        pl.pipe = can;
    }
    pl.lds_bytes = plan_lds_bytes(cf, (size_t)k.NI * k.seg_pix, x3, k.NI, pl.pipe != 0) + kLdsSlackB;
    pl.nit = ds_ceil_div(k.NI * std::min(k.rows_in, s->H) * s->W * (CKB / 4), cf.NTHR());
    // a plain launch until a fused entry point says otherwise: no BatchNorm-backward epilogue
    k.bn_z = k.bn_mean = k.bn_invstd = k.bn_msc = k.bn_msh = nullptr;
    k.bn_mtiles = 1; k.bn_rows_member = 0; k.bn_row0 = 0;
    return DS_OK;
}

// the operands of a launch (every entry point; the fused ones then add the bn_* fields)
static void set_operands(ConvKB &k, const float *x, const void *w_hi, const void *w_lo, float *y, const float *scale,
                         const float *shift, const float *res, float *stats, int flags) {
    k.x = x; k.w_hi = (const __bf16 *)w_hi; k.w_lo = (const __bf16 *)w_lo; k.y = y;
    k.scale = scale; k.shift = shift; k.res = res; k.stats = stats;
    k.flags = flags;
}

// kernel size x arithmetic -> the translation unit that holds those instantiations
template <int KS, bool X3>
static void launch_b(const PlanB &pl, void *stream) {
    if (pl.pipe) {                      // the pipelined walk: bf16x3 only (plan_bf16)
        if (KS == 3) ds_bf16_launch_k3x3p(pl, stream); else ds_bf16_launch_k5x3p(pl, stream);
        return;
    }
    if (pl.cfg >= kNumCfgB) {           // a latency row: bf16x3 only (plan_bf16 offers them to no other arithmetic)
        if (KS == 3) ds_bf16_launch_k3x3l(pl, stream); else ds_bf16_launch_k5x3l(pl, stream);
        return;
    }
    if (KS == 3) { if (X3) ds_bf16_launch_k3x3(pl, stream); else ds_bf16_launch_k3x1(pl, stream); }
    else         { if (X3) ds_bf16_launch_k5x3(pl, stream); else ds_bf16_launch_k5x1(pl, stream); }
}

}  // namespace

// One filter of a pack call, single or batched; *n = its elements.  The two callers report an unsupported KS with
// different codes (DS_ERR_BAD_SHAPE from the single-filter entry points, DS_ERR_UNSUPPORTED from the batch): each keeps
// its code, `bad_ks`.
static int pack_job_check(const void *w_oihw, const void *w_hi, int Cout, int Cin, int KS, int dgrad, int bad_ks, long long *n) {
    DS_REQUIRE(w_oihw && w_hi, DS_ERR_NULL);
    DS_REQUIRE((dgrad == 0 || dgrad == 1) && Cout > 0 && Cin > 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(KS == 3 || KS == 5, bad_ks);
    DS_REQUIRE((dgrad ? Cout : Cin) % CKB == 0, DS_ERR_BAD_SHAPE);
    *n = (long long)Cout * Cin * KS * KS;
    return DS_OK;
}

static int pack_bf16(const float *w_oihw, void *w_hi, void *w_lo, int Cout, int Cin, int KS, int dgrad, void *stream) {
    long long n;
    const int rc = pack_job_check(w_oihw, w_hi, Cout, Cin, KS, dgrad, DS_ERR_BAD_SHAPE, &n);
    if (rc != DS_OK) return rc;
    long long g = (n + 255) / 256;
    DS_LAUNCH(pack_conv_weight_bf16_kernel, (int)(g > 4096 ? 4096 : g), 256, 0, stream, w_oihw, (__bf16 *)w_hi,
              (__bf16 *)w_lo, Cout, Cin, KS, dgrad);
    return ds_last_launch_error();
}

extern "C" int ds_pack_conv_weights_bf16_batch(const ds_pack_job *jobs, int n_jobs, void *stream) {
    DS_REQUIRE(jobs != nullptr, DS_ERR_NULL);
    DS_REQUIRE(n_jobs > 0 && n_jobs <= DS_PACK_BATCH_MAX, DS_ERR_BAD_SHAPE);
    PackBatchB J;
    J.n = n_jobs;
    int blocks = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const ds_pack_job &b = jobs[j];
        long long n;
        const int rc = pack_job_check(b.w_oihw, b.out, b.Cout, b.Cin, b.KS, b.mode, DS_ERR_UNSUPPORTED, &n);
        if (rc != DS_OK) return rc;
        J.w[j] = b.w_oihw; J.hi[j] = (__bf16 *)b.out; J.lo[j] = (__bf16 *)b.out2;
        J.Cout[j] = b.Cout; J.Cin[j] = b.Cin; J.KS[j] = b.KS; J.dgrad[j] = b.mode;
        const long long g = (n + 255) / 256;
        J.first[j] = blocks;
        blocks += (int)(g > 512 ? 512 : g);
    }
    J.first[n_jobs] = blocks;
    DS_LAUNCH(pack_conv_weight_bf16_batch_kernel, blocks, 256, 0, stream, J);
    return ds_last_launch_error();
}

extern "C" int ds_pack_conv_weight_bf16(const float *w_oihw, void *w_hi, void *w_lo, int Cout, int Cin, int KS,
                                        void *stream) {
    return pack_bf16(w_oihw, w_hi, w_lo, Cout, Cin, KS, 0, stream);
}

extern "C" int ds_pack_conv_weight_dgrad_bf16(const float *w_oihw, void *w_hi, void *w_lo, int Cout, int Cin, int KS,
                                              void *stream) {
    return pack_bf16(w_oihw, w_hi, w_lo, Cout, Cin, KS, 1, stream);
}

// the plan mode of a forward launch with these `flags`
static int fwd_plan_mode(int flags) { return kPlanLatRows | ((flags & DS_CONV_PLAN_LATENCY) ? kPlanLatency : 0); }

extern "C" int ds_conv_bf16_stats_rows(const ds_conv_shape *s, int x3) {
    PlanB pl;
    int rc = plan_bf16(pl, s, x3 != 0, 1, 0, 0, 0, 0, 0, 0, fwd_plan_mode(0));
    return rc == DS_OK ? pl.n_mtiles : rc;
}

// tuning hook: cfg in [0, 9) = plan every bf16 convolution with that tile configuration, 9 and 10 = the latency rows
// (bf16x3 forward launches only: every other launch is then refused); anything else = the planner's choice
extern "C" void ds_conv_bf16_set_forced_cfg(int cfg) { g_forced_cfg_b = (cfg >= 0 && cfg < kNumCfgBAll) ? cfg : -1; }

// tuning hook: the walk of the bf16x3 forward launches (see plan_bf16); anything but 1 and 2 = the planner's choice
extern "C" void ds_conv_bf16_set_walk(int walk) { g_walk_b = (walk == 1 || walk == 2) ? walk : 0; }

// the walk ds_conv_fwd_bf16 would launch `s` with under `flags`: 1 = classic, 2 = pipelined, or an error code
extern "C" int ds_conv_bf16_plan_walk(const ds_conv_shape *s, int x3, int flags) {
    PlanB pl;
    const int rc = plan_bf16(pl, s, x3 != 0, 1, 0, 0, 0, 0, 0, 0, fwd_plan_mode(flags));
    return rc == DS_OK ? (pl.pipe ? 2 : 1) : rc;
}

extern "C" int ds_conv_bf16_plan_describe(const ds_conv_shape *s, int x3, int *out8) {
    return ds_conv_bf16_plan_describe_hinted(s, x3, 0, out8);
}

extern "C" int ds_conv_bf16_plan_describe_hinted(const ds_conv_shape *s, int x3, int flags, int *out8) {
    DS_REQUIRE(out8 != nullptr, DS_ERR_NULL);
    PlanB pl;
    int rc = plan_bf16(pl, s, x3 != 0, 1, 0, 0, 0, 0, 0, 0, fwd_plan_mode(flags));
    if (rc != DS_OK) return rc;
    const TileCfgB &cf = ds_bf16_cfg(pl.cfg);
    out8[0] = cf.MT(); out8[1] = cf.NTILE(); out8[2] = pl.k.RT; out8[3] = pl.k.NI;
    out8[4] = pl.grid; out8[5] = (int)pl.lds_bytes; out8[6] = cf.NTHR(); out8[7] = pl.k.pitch;
    return DS_OK;
}

extern "C" int ds_conv_fwd_bf16(const ds_conv_shape *s, const float *x, const void *w_hi, const void *w_lo,
                                const float *scale, const float *shift, const float *residual, float *y,
                                float *stats_partial, int flags, void *stream) {
    DS_REQUIRE(x && w_hi && y, DS_ERR_NULL);
    DS_REQUIRE(!(flags & DS_EPI_AFFINE) || (scale && shift), DS_ERR_NULL);
    DS_REQUIRE(!(flags & DS_EPI_RESIDUAL) || residual, DS_ERR_NULL);
    DS_REQUIRE(!(flags & DS_EPI_STATS) || stats_partial, DS_ERR_NULL);
    // the statistics rows are sized by ds_conv_bf16_stats_rows, i.e. by the plan without the flag
    DS_REQUIRE(!((flags & DS_CONV_PLAN_LATENCY) && (flags & DS_EPI_STATS)), DS_ERR_UNSUPPORTED);
    DS_REQUIRE(DS_ALIGNED16(x) && DS_ALIGNED16(w_hi) && DS_ALIGNED16(y) && DS_ALIGNED16(w_lo), DS_ERR_ALIGNMENT);
    const bool x3 = w_lo != nullptr;
    PlanB pl;
    int rc = plan_bf16(pl, s, x3, 1, 0, 0, 0, 0, 0, 0, fwd_plan_mode(flags));
    if (rc != DS_OK) return rc;
    set_operands(pl.k, x, w_hi, w_lo, y, scale, shift, residual, stats_partial, flags & ~DS_CONV_PLAN_LATENCY);
    if (s->KS == 3) { if (x3) launch_b<3, true>(pl, stream); else launch_b<3, false>(pl, stream); }
    else            { if (x3) launch_b<5, true>(pl, stream); else launch_b<5, false>(pl, stream); }
    return ds_last_launch_error();
}

// banks of the 5x5 stride-2 data gradient: parity class (ph, pw) of dX only receives taps kh = ph (mod 2),
// kw = pw (mod 2), at input offsets d = (p + 2 - k) / 2 in {1, 0, -1} -- a 3x3 stride-1 convolution over dY
// per class; classes with two taps per axis carry zero filters for the third (window row/col 0, d = -1).
// Layout: [class ph*2+pw][Cout/16][tap (d_h+1)*3 + (d_w+1)][Cin][16] bf16 hi (+ lo).
__global__ void __launch_bounds__(256) pack_conv_dgrad_s2_bf16_kernel(const float *w, __bf16 *hi, __bf16 *lo, int Cout,
                                                                      int Cin) {
    const long long per_class = (long long)9 * Cout * Cin;
    const long long n = 4 * per_class;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int cls = (int)(i / per_class);
        long long r = i - cls * per_class;
        const int kk = (int)(r & 15);
        r >>= 4;
        const int ci = (int)(r % Cin);
        r /= Cin;
        const int t = (int)(r % 9);
        const int kc = (int)(r / 9);
        const int co = kc * 16 + kk;                    // contraction channel = forward output channel
        const int ph = cls >> 1, pw = cls & 1;
        const int dh = t / 3 - 1, dw = t % 3 - 1;       // input offset of this window position
        const int kh = ph + 2 - 2 * dh, kw = pw + 2 - 2 * dw;
        float v = 0.0f;
        if (kh >= 0 && kh < 5 && kw >= 0 && kw < 5) v = w[(((size_t)co * Cin + ci) * 5 + kh) * 5 + kw];
        const __bf16 h = (__bf16)v;
        hi[i] = h;
        lo[i] = (__bf16)(v - (float)h);
    }
}

extern "C" int ds_pack_conv_weight_dgrad_s2_bf16(const float *w_oihw, void *w_hi, void *w_lo, int Cout, int Cin,
                                                 void *stream) {
    DS_REQUIRE(w_oihw && w_hi && w_lo, DS_ERR_NULL);
    DS_REQUIRE(Cout > 0 && Cin > 0 && (Cout % CKB) == 0, DS_ERR_BAD_SHAPE);
    const long long n = (long long)36 * Cout * Cin;
    long long g = (n + 255) / 256;
    DS_LAUNCH(pack_conv_dgrad_s2_bf16_kernel, (int)(g > 4096 ? 4096 : g), 256, 0, stream, w_oihw, (__bf16 *)w_hi,
              (__bf16 *)w_lo, Cout, Cin);
    return ds_last_launch_error();
}

// One parity class (conv_plan.h) of the 5x5 stride-2 data gradient of forward shape `s`: a 3x3 stride-1 bf16x3
// convolution over the dY grid whose Hr x Wc outputs land on every other pixel of dX.  The class must not be empty.
static int plan_s2_class(PlanB &pl, const ds_conv_shape *s, const ds_s2_class &c) {
    ds_conv_shape t = {s->B, ds_s2_dy_rows(s->H), ds_s2_dy_cols(s->W), s->Cout, s->Cin, 3, 1};
    return plan_bf16(pl, &t, true, 2, c.ph, c.pw, s->H, s->W, c.Hr, c.Wc);
}
// the filter bank of class cls (layout: pack_conv_dgrad_s2_bf16_kernel)
static const __bf16 *s2_bank(const void *w, const ds_conv_shape *s, int cls) {
    return (const __bf16 *)w + cls * ((size_t)9 * s->Cout * s->Cin);
}

// data gradient on the bf16 matrix cores.  3x3 stride 1: the forward kernel on dY with the flipped /
// transposed bank (ds_pack_conv_weight_dgrad_bf16).  5x5 stride 2: four parity-class launches over the dY
// grid with the banks of ds_pack_conv_weight_dgrad_s2_bf16, outputs interleaved in dX.
extern "C" int ds_conv_dgrad_bf16(const ds_conv_shape *s, const float *gy, const void *w_hi, const void *w_lo,
                                  float *gx, void *stream) {
    DS_REQUIRE(s, DS_ERR_NULL);
    if (s->stride == 1) {
        DS_REQUIRE(s->KS == 3, DS_ERR_UNSUPPORTED);
        ds_conv_shape t = *s;
        t.Cin = s->Cout;
        t.Cout = s->Cin;
        return ds_conv_fwd_bf16(&t, gy, w_hi, w_lo, nullptr, nullptr, nullptr, gx, nullptr, 0, stream);
    }
    DS_REQUIRE(s->KS == 5 && s->stride == 2 && gy && w_hi && w_lo && gx, DS_ERR_UNSUPPORTED);
    DS_REQUIRE(DS_ALIGNED16(gy) && DS_ALIGNED16(w_hi) && DS_ALIGNED16(w_lo) && DS_ALIGNED16(gx), DS_ERR_ALIGNMENT);
    for (int cls = 0; cls < 4; ++cls) {
        const ds_s2_class c = ds_s2_class_of(s->H, s->W, cls);
        if (c.empty()) continue;
        PlanB pl;
        int rc = plan_s2_class(pl, s, c);
        if (rc != DS_OK) return rc;
        set_operands(pl.k, gy, s2_bank(w_hi, s, cls), s2_bank(w_lo, s, cls), gx, nullptr, nullptr, nullptr, nullptr, 0);
        launch_b<3, true>(pl, stream);
        rc = ds_last_launch_error();
        if (rc) return rc;
    }
    return DS_OK;
}


// M tiles per member of a plan whose batch is G members, or DS_ERR_UNSUPPORTED where a tile would straddle two
static int member_mtiles(const PlanB &pl, int B, int G) {
    const long long segs_per_member = (long long)(B / G) * pl.k.segs_per_img;
    DS_REQUIRE(segs_per_member % pl.k.NI == 0, DS_ERR_UNSUPPORTED);
    return (int)(segs_per_member / pl.k.NI);
}

// The 3x3 stride-1 data gradient FUSED with the first half of the BatchNorm backward of the layer it feeds
// (autograd of clip(bn(conv(.))) under loss.backward(), reference train_triplet.py:223 over model.py:69-75,188-203):
//   gy = (dgrad(gz_up) [+ g2]) * [0 < z * mask_scale + mask_shift < 20],  partial[tile] = { sum gy, sum gy * xhat }
// `s` is the FORWARD shape of the convolution whose data gradient this is (as ds_conv_dgrad_bf16); z / gy / g2 are
// [B,H,W,Cin]; the batch consists of G members with their own statistics (tables [G][Cin]); the M tiles of the launch
// must not straddle members (ds_conv_dgrad_bnbwd_bf16_rows reports the partial rows per member, or an error).
static int plan_bnbwd(PlanB &pl, const ds_conv_shape *s, int G) {
    DS_REQUIRE(s, DS_ERR_NULL);
    DS_REQUIRE(s->KS == 3 && s->stride == 1 && G > 0 && s->B % G == 0, DS_ERR_UNSUPPORTED);
    ds_conv_shape t = *s;
    t.Cin = s->Cout;
    t.Cout = s->Cin;
    int rc = plan_bf16(pl, &t, true);
    if (rc != DS_OK) return rc;
    const int rows = member_mtiles(pl, s->B, G);
    if (rows < 0) return rows;
    pl.k.bn_mtiles = rows;
    pl.k.bn_rows_member = rows;
    pl.k.bn_row0 = 0;
    return DS_OK;
}

extern "C" int ds_conv_dgrad_bnbwd_bf16_rows(const ds_conv_shape *s, int G) {
    PlanB pl;
    int rc = plan_bnbwd(pl, s, G);
    return rc == DS_OK ? pl.k.bn_mtiles : rc;
}

extern "C" int ds_conv_dgrad_bnbwd_bf16(const ds_conv_shape *s, const float *gz_up, const void *w_hi, const void *w_lo,
                                        const float *g2, const float *z, const float *mean, const float *invstd,
                                        const float *mask_scale, const float *mask_shift, int G, float *gy,
                                        float *partial, void *stream) {
    DS_REQUIRE(s && gz_up && w_hi && w_lo && z && mean && invstd && mask_scale && mask_shift && gy && partial, DS_ERR_NULL);
    DS_REQUIRE(DS_ALIGNED16(gz_up) && DS_ALIGNED16(w_hi) && DS_ALIGNED16(w_lo) && DS_ALIGNED16(z) && DS_ALIGNED16(gy) &&
                   DS_ALIGNED16(mean) && DS_ALIGNED16(invstd) && DS_ALIGNED16(mask_scale) && DS_ALIGNED16(mask_shift) &&
                   (!g2 || DS_ALIGNED16(g2)), DS_ERR_ALIGNMENT);
    PlanB pl;
    int rc = plan_bnbwd(pl, s, G);
    if (rc != DS_OK) return rc;
    set_operands(pl.k, gz_up, w_hi, w_lo, gy, nullptr, nullptr, g2, partial, DS_EPI_STATS | (g2 ? DS_EPI_RESIDUAL : 0));
    pl.k.bn_z = z; pl.k.bn_mean = mean; pl.k.bn_invstd = invstd; pl.k.bn_msc = mask_scale; pl.k.bn_msh = mask_shift;
    ds_bf16_launch_k3x3g(pl, stream);
    return ds_last_launch_error();
}

// The same fusion for the 5x5 stride-2 data gradient, which feeds the activation of a BasicBlock's OUTPUT,
// out = clip(bn2(conv2(y)) + r) (model.py:76-80): that clip's mask cannot be re-derived from z alone, so it is read from
// the stored activation `act` ([B,H,W,Cin], the 5x5 layer's input); no second gradient is added.  Four parity-class
// launches (ds_conv_dgrad_bf16) write interleaved pixels of gy and consecutive blocks of partial rows: class cls owns
// rows[cls] partial rows per member (0: an empty class, not launched), `total` of them together.
struct S2BnbwdPlans {
    PlanB pl[4];
    int rows[4], total;
};

static int plan_s2_bnbwd(S2BnbwdPlans &P, const ds_conv_shape *s, int G) {
    DS_REQUIRE(s, DS_ERR_NULL);
    DS_REQUIRE(s->KS == 5 && s->stride == 2 && G > 0 && s->B % G == 0, DS_ERR_UNSUPPORTED);
    P.total = 0;
    for (int cls = 0; cls < 4; ++cls) {
        const ds_s2_class c = ds_s2_class_of(s->H, s->W, cls);
        P.rows[cls] = 0;
        if (c.empty()) continue;
        int rc = plan_s2_class(P.pl[cls], s, c);
        if (rc != DS_OK) return rc;
        const int rows = member_mtiles(P.pl[cls], s->B, G);
        if (rows < 0) return rows;
        P.rows[cls] = rows;
        P.total += rows;
    }
    return DS_OK;
}

extern "C" int ds_conv_dgrad_s2_bnbwd_bf16_rows(const ds_conv_shape *s, int G) {
    S2BnbwdPlans P;
    int rc = plan_s2_bnbwd(P, s, G);
    return rc == DS_OK ? P.total : rc;
}

extern "C" int ds_conv_dgrad_s2_bnbwd_bf16(const ds_conv_shape *s, const float *gz_up, const void *w_hi, const void *w_lo,
                                           const float *act, const float *z, const float *mean, const float *invstd,
                                           int G, float *gy, float *partial, void *stream) {
    DS_REQUIRE(s && gz_up && w_hi && w_lo && act && z && mean && invstd && gy && partial, DS_ERR_NULL);
    DS_REQUIRE(s->KS == 5 && s->stride == 2 && G > 0 && s->B % G == 0, DS_ERR_UNSUPPORTED);
    DS_REQUIRE(DS_ALIGNED16(gz_up) && DS_ALIGNED16(w_hi) && DS_ALIGNED16(w_lo) && DS_ALIGNED16(act) && DS_ALIGNED16(z) &&
                   DS_ALIGNED16(gy) && DS_ALIGNED16(mean) && DS_ALIGNED16(invstd), DS_ERR_ALIGNMENT);
    S2BnbwdPlans P;
    int rc = plan_s2_bnbwd(P, s, G);
    if (rc != DS_OK) return rc;
    if (P.total <= 0) return DS_ERR_UNSUPPORTED;
    int row0 = 0;
    for (int cls = 0; cls < 4; ++cls) {
        if (P.rows[cls] == 0) continue;
        PlanB &pl = P.pl[cls];
        // res = the mask's source (not added: bn_msc == nullptr)
        set_operands(pl.k, gz_up, s2_bank(w_hi, s, cls), s2_bank(w_lo, s, cls), gy, nullptr, nullptr, act, partial,
                     DS_EPI_STATS | DS_EPI_RESIDUAL);
        pl.k.bn_z = z; pl.k.bn_mean = mean; pl.k.bn_invstd = invstd;
        pl.k.bn_mtiles = P.rows[cls];
        pl.k.bn_rows_member = P.total;
        pl.k.bn_row0 = row0;
        ds_bf16_launch_k3x3g(pl, stream);
        rc = ds_last_launch_error();
        if (rc) return rc;
        row0 += P.rows[cls];
    }
    return DS_OK;
}
