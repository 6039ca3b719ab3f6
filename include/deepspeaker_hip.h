/*
 * deepspeaker_hip.h -- C ABI of libdeepspeaker_hip.so (MI355X / gfx950).
 *
 * The reference (qqueing/DeepSpeaker-pytorch) is pure Python: it has no FFI or
 * plugin interface.  Its hot path is the Python surface of model.py as used by
 * train_triplet.py; every tensor op that surface executes
 * through ATen/cuDNN is replaced here by one entry point.  Each declaration
 * cites the reference line(s) whose arithmetic it takes over.
 *
 * Conventions (all entry points):
 *   - plain device pointers and sizes, no torch types; `stream` is a hipStream_t
 *     passed as void* (the caller's current stream).  Work is only enqueued: no
 *     entry point synchronises the device or a stream (ds_event_elapsed_ms, a
 *     read-out helper, waits for its `stop` event), so calls are re-entrant and
 *     hipGraph-capturable.
 *   - the caller owns ALL device memory: tensor buffers (inputs, outputs, scratch)
 *     and the tile-scheduling workspace of the persistent fp16 kernels
 *     (ds_sched_workspace_bytes / ds_sched_set_workspace below).  The library never
 *     allocates, frees, memsets or synchronises.  State the LIBRARY keeps -- all of
 *     it host-side, each item behind its own lock or thread-local:
 *       (1) the table of which 64-byte slots of the caller's scheduler workspaces
 *           have been handed out: a ring of 8 per (device, stream) for eager
 *           launches, one slot for good per launch captured into a graph
 *           (csrc/bn_pack.hip ds_sched_slot); a launch that finds no free slot
 *           returns DS_ERR_NO_WORKSPACE;
 *       (2) the armed event pair of ds_launch_timing_arm: thread-local, consumed by
 *           the calling thread's next MFMA launch (csrc/ds_device.h);
 *       (3) process-wide tuning hooks, ds_conv_f16_set_layout_padding and
 *           ds_conv_{f32,f16,bf16}_set_forced_cfg (off by default; A/B and test hooks that
 *           change speed, never results);
 *       (4) the cached compute-unit count per device (read once).
 *     Nothing else is kept between calls.
 *   - return value: 0 = DS_OK, negative = argument error (below), positive = the
 *     hipError_t of a failed launch.  Nothing throws, aborts or prints.
 *   - activations are channels-last fp32:  [B, T', F', C]  (the reference's NCHW
 *     tensors [B, C, T', F'] permuted; for the network input C = 1, so the
 *     reference's [B,1,T,64] buffer is consumed bit-for-bit as [B,T,64,1]).
 *     ds_nchw_to_nhwc_f32 / ds_nhwc_to_nchw_f32 convert for per-op use.
 *   - convolution weights are consumed in a packed layout produced once per
 *     weight version by ds_pack_* from the reference's OIHW / [out,in] tensors.
 *   - pointers must be 16-byte aligned (every torch allocation is).
 */
#ifndef DEEPSPEAKER_HIP_H
#define DEEPSPEAKER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DS_OK               0
#define DS_ERR_BAD_SHAPE   (-1)
#define DS_ERR_ALIGNMENT   (-2)
#define DS_ERR_NULL        (-3)
#define DS_ERR_UNSUPPORTED (-4)
#define DS_ERR_NO_WORKSPACE (-5)    /* a persistent launch found no free tile-scheduling slot: ds_sched_set_workspace */

/* epilogue flags of the convolution entry points */
#define DS_EPI_AFFINE   1   /* y = acc * scale[c] + shift[c]   (BatchNorm with fixed statistics) */
#define DS_EPI_RESIDUAL 2   /* y += residual                    (model.py:79)                      */
#define DS_EPI_CLIP     4   /* y = min(max(y, 0), 20)           (model.py:36-44)                   */
#define DS_EPI_STATS    8   /* also emit per-tile column sums {sum, sum of squares} of the RAW
                               accumulator (train-mode BatchNorm statistics)                       */

#define DS_EPI_OUT_F32  16  /* fp16 convolution: store the result as f32 (the layer feeding the f32 tail)     */
#define DS_EPI_OUT_F16  32  /* conv1 (ds_conv5x5s2_c1_fwd_bf16): store the result as fp16                    */

#define DS_EPI_OUT_PLANES16  256 /* fp16 convolution: store y channel-plane-major, [Cout/16][B*Ho*Wo][16] fp16          */
#define DS_CONV_IN_PLANES16  512 /* fp16 5x5 convolution: x is channel-plane-major [Cin/16][B*H*W][16]: every
                                    16-channel chunk then reads whole 128-byte lines (a 64-channel channels-last
                                    record is one line, of which a chunk would use a quarter)                       */
#define DS_CONV_PLAN_LATENCY 8192 /* ds_conv_fwd_bf16, bf16x3: a launch too small to put a wave on every SIMD is planned
                                     for its latency -- the tile that makes a wave's walk over the contraction shortest,
                                     the one-sub-tile latency rows included -- instead of for the CU time it takes.  The
                                     result is bit-identical with and without the flag; not with DS_EPI_STATS (whose
                                     rows are sized by the plan without it)                                            */
#define DS_CONV_HINT_SINGLE_BUFFER 64  /* fp16 convolution: plan with one LDS pixel tile (tuning / test hint)  */
#define DS_CONV_HINT_CHUNK16      128  /* fp16 5x5 convolution: plan with 16-channel chunks (tuning / test hint)  */
#define DS_CONV_HINT_NO_WIDE     2048  /* fp16 convolution: keep 64-channel-wide register tiles where the persistent kernel
                                        * would take 128-wide ones (tuning / test hint: bit-identical)                */
#define DS_CONV_HINT_ONE_QUEUE   4096  /* fp16 convolution, persistent kernel: one tile queue for the whole grid instead
                                        * of one per XCD (tuning / test hint: bit-identical)                         */
#define DS_CONV_HINT_NO_PERSIST  1024  /* fp16 convolution: one tile per workgroup even where the persistent kernel
                                        * applies (tuning / test hint: the two kernels are bit-identical)          */

#define DS_CONV_CK      8   /* input-channel chunk of the packed weight layout */

int ds_version(void);            /* 100: round 1; 200: round 2 (fp16 path, grouped BatchNorm backward, ds_bn_bwd_partial_rows takes C);
                                    300 / 301: round 3 (persistent fp16 kernels, split grouped BatchNorm backward; + ds_conv_dgrad_bnbwd_bf16);
                                    400: round 4 (fp16 training step: ds_*_f16 train entry points, ds_wgrad_f16, probes of the
                                    near-tie refinement, launch-bound timing); 500: round 5; 600: round 6 (caller-owned
                                    scheduler workspace); 700: log-mel filterbank front end (ds_fbank_*); 800: speaker identification
                                    (ds_nearest_*, ds_segment_mean_rows_f32, ds_rank_hits_i32); 900: polyphase resampler
                                    (ds_resample_plan, ds_resample_poly_f32); 1000: energy VAD (ds_vad_*); 1100: angular-margin softmax head;
                                    1200: score normalisation (ds_cohort_*, ds_score_norm_apply_f32); 1300: waveform augmentation
                                    (ds_augment_*) */
/* launch timing without marker packets: the next MFMA convolution / filter-gradient launch of the calling thread
 * records its own execution into the armed pair (hipExtLaunchKernelGGL); ds_launch_timing_end() disarms and returns
 * how many such launches happened since arming (1 = the timed call was a single kernel) */
int ds_event_create(void **out_event);
int ds_event_destroy(void *event);
int ds_event_elapsed_ms(void *start, void *stop, float *ms);     /* waits for `stop` */
int ds_launch_timing_arm(void *start, void *stop);
int ds_launch_timing_end(void);
const char *ds_error_string(int code);

/* ---- tile-scheduling workspace of the persistent kernels (ds_conv_fwd_f16, ds_conv_block_f16) ----
 * Those kernels draw tiles from device-side counters ("slots", 64 bytes each, left zeroed by the kernel that used them).
 * The memory is the caller's: hand over ZEROED device memory of ds_sched_workspace_bytes() on the current device before
 * the first such launch there (again whenever a launch returns DS_ERR_NO_WORKSPACE: every launch captured into a graph
 * keeps one slot for good) and keep it allocated.  ds_sched_free_slots(): slots of the current device not handed out yet. */
size_t ds_sched_workspace_bytes(void);
int ds_sched_set_workspace(void *zeroed_device_memory, size_t bytes);
long long ds_sched_free_slots(void);
/* measurement only: one launch of independent fp16 (bf16 != 0: bf16) 32x32x16 MFMAs issued back to back from registers on
 * every SIMD, random operand bits -- the matrix cores' power- / clock-limited rate on THIS chip.  *flop_out receives the
 * floating-point operations of the launch; the caller times it with its own events (bench.py:
 * roofline.mfma_register_only_tflops).  Not on any product path. */
int ds_mfma_rate_probe(int bf16, int iters, float *sink, double *flop_out, void *stream);
/* the same launch with fp16 operands taken from REAL tensors: A fragments (8 consecutive halfs each) from `a_f16` (n_a
 * halfs, e.g. a packed filter bank), B fragments from `b_f16` (n_b halfs, e.g. an fp16 activation tensor); 16-byte
 * aligned.  What the matrix cores sustain on the operand values the convolutions see (bench.py:
 * roofline.mfma_register_only_real_operands_tflops). */
int ds_mfma_rate_probe_data(const void *a_f16, long long n_a, const void *b_f16, long long n_b, int iters, float *sink,
                            double *flop_out, void *stream);

/* ---- layout ---------------------------------------------------------------------------------- */
int ds_nchw_to_nhwc_f32(const float *x, float *y, int B, int C, int H, int W, void *stream);
int ds_nhwc_to_nchw_f32(const float *x, float *y, int B, int C, int H, int W, void *stream);

/* ---- weight packing (one-off per weight version; not on the per-batch path) ------------------- */
/* Many filters in ONE launch (a training step re-packs every filter after every optimizer step: 22 launches of ~5 us
 * each in the fp16 mode, 19 in the bf16x3 mode, became one each).  A job = one ds_pack_conv_weight_{f16,bf16} call:
 * mode 0 forward bank, 1 stride-1 data-gradient bank (transposed, flipped), 2 (f16 only) the 5x5 stride-2 layer's
 * parity-class data-gradient bank.  out2: the bf16 "lo" bank (bf16 family; may be NULL), unused by the f16 family.
 * At most DS_PACK_BATCH_MAX jobs per call. */
#define DS_PACK_BATCH_MAX 32
typedef struct ds_pack_job {
    const float *w_oihw;
    void *out, *out2;
    int Cout, Cin, KS, mode;
} ds_pack_job;
int ds_pack_conv_weights_f16_batch(const ds_pack_job *jobs, int n_jobs, void *stream);
int ds_pack_conv_weights_bf16_batch(const ds_pack_job *jobs, int n_jobs, void *stream);
/* OIHW [Cout,Cin,KS,KS] -> [Cin/8][KS*KS][Cout][8].  dgrad != 0 packs the transposed, spatially
 * flipped filter bank used by ds_conv_dgrad_f32 (Cout and Cin swap roles).
 * Replaces: nothing in the reference (cuDNN picks its own filter layout, model.py:47-50,93-106). */
int ds_pack_conv_weight_f32(const float *w_oihw, float *w_packed, int Cout, int Cin, int KS,
                            int dgrad, void *stream);
/* conv1 weight [64,1,5,5] -> [25][64]  (model.py:93) */
int ds_pack_conv1_weight_f32(const float *w_oihw, float *w_packed, int Cout, void *stream);
/* fc weight [N, C*F] indexed c*F+f (model.py:164,208) -> 1x1-conv packing over k' = f*C + c,
 * the order in which ds_avgpool_time_f32 emits the pooled features. */
int ds_pack_fc_weight_f32(const float *w, float *w_packed, int N, int C, int F, void *stream);
/* the transposed bank for the fc data gradient (gpooled = gf . W), same k' order */
int ds_pack_fc_weight_dgrad_f32(const float *w, float *w_packed, int N, int C, int F, void *stream);

/* ---- BatchNorm ---------------------------------------------------------------------------------- */
/* eval mode: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale
 * (model.py:70,74,188,193,198,203 with module.eval()). */
int ds_bn_fold_f32(const float *gamma, const float *beta, const float *running_mean,
                   const float *running_var, float eps, float *scale, float *shift, int C,
                   void *stream);
/* train mode: reduce the per-tile partial sums written under DS_EPI_STATS, produce batch mean /
 * invstd, the affine (scale, shift) that normalises with them, and update the running statistics
 * in place (momentum, unbiased variance) exactly like nn.BatchNorm2d.train() -- SURVEY 8(a) a2. */
int ds_bn_stats_finalize_f32(const float *partial, int n_partial, long long count,
                             const float *gamma, const float *beta, float eps, float momentum,
                             float *running_mean, float *running_var, float *batch_mean,
                             float *batch_invstd, float *scale, float *shift, int C, void *stream);
/* y = [clip]( x * scale[c] + shift[c] [+ residual] ) over n_pix pixels of C channels. */
int ds_bn_apply_f32(const float *x, const float *scale, const float *shift, const float *residual,
                    float *y, long long n_pix, int C, int flags, void *stream);

/* ---- convolutions ------------------------------------------------------------------------------- */
typedef struct ds_conv_shape {
    int B, H, W, Cin;   /* input  [B,H,W,Cin]                        */
    int Cout, KS;       /* square KS x KS filter, padding KS/2       */
    int stride;         /* 1 or 2                                    */
} ds_conv_shape;

int ds_conv_out_dims(const ds_conv_shape *s, int *Ho, int *Wo);
/* number of [Cout][2] partial-statistics rows DS_EPI_STATS writes for this shape */
int ds_conv_stats_rows(const ds_conv_shape *s);

/* tiling the planner picks for a shape: out8 = {M tile, N tile, rows per segment, segments per tile,
 * workgroups, LDS bytes, staging slots per thread, M tiles} (introspection for tests / DESIGN.md) */
int ds_conv_plan_describe(const ds_conv_shape *s, int *out8);
/* test hook, as ds_conv_f16_set_forced_cfg: plan the f32 forward and both data gradients with tile configuration `cfg`
 * only (0: 128x64, 1: 160x128, 2: 256x64; anything else: the planner's choice) */
void ds_conv_f32_set_forced_cfg(int cfg);
int ds_conv5x5s2_c1_stats_rows(int B, int H);
/* conv1: 5x5 stride 2 pad 2, Cin = 1 -> 64 channels (model.py:93,187) fused with the following
 * BatchNorm affine + clipped ReLU (model.py:188-189).  x is the network input [B,H,W]. */
int ds_conv5x5s2_c1_fwd_f32(const float *x, const float *w_packed, const float *scale,
                            const float *shift, float *y, float *stats_partial, int B, int H,
                            int W, int Cout, int flags, void *stream);
/* the same layer on the bf16 matrix cores with split operands (bf16x3); same packed bank and statistics rows.
 * y is f32 [B,Ho,Wo,64], or fp16 with DS_EPI_OUT_F16 (the input of the fp16 convolution path) */
int ds_conv5x5s2_c1_fwd_bf16(const float *x, const float *w_packed, const float *scale,
                             const float *shift, void *y, float *stats_partial, int B, int H,
                             int W, int Cout, int flags, void *stream);
/* generic implicit-GEMM convolution on the f32 matrix cores: 3x3 s1 p1 (model.py:47-50,69,73),
 * 5x5 s2 p2 (model.py:98,102,106 / :192,197,202) and 1x1 (the fc GEMM, model.py:209), with the
 * BatchNorm / residual / clipped-ReLU epilogue selected by `flags`. */
int ds_conv_fwd_f32(const ds_conv_shape *s, const float *x, const float *w_packed,
                    const float *scale, const float *shift, const float *residual, float *y,
                    float *stats_partial, int flags, void *stream);

/* ---- bf16 matrix-core variants of the forward convolutions (v_mfma_f32_32x32x16_bf16, f32 accumulate;
 *      same epilogue flags, f32 channels-last activations in and out -> drop-in for ds_conv_fwd_f32).
 *      w_lo == NULL: plain bf16 operands (speed mode, ~6e-3 embedding drift on this network);
 *      w_lo != NULL: "bf16x3" -- both operands split hi+lo, product = hi*hi + hi*lo + lo*hi: f32-class
 *      accuracy at up to 1/3 of the bf16 peak.  KS in {3, 5}; Cin % 16 == 0. ----------------------- */
int ds_pack_conv_weight_bf16(const float *w_oihw, void *w_hi, void *w_lo, int Cout, int Cin, int KS,
                             void *stream);             /* -> [Cin/16][KS*KS][Cout][16] bf16 (x2) */
int ds_pack_conv_weight_dgrad_bf16(const float *w_oihw, void *w_hi, void *w_lo, int Cout, int Cin,
                                   int KS, void *stream);   /* flipped / transposed bank, stride 1 */
/* the four parity-class banks of the 5x5 stride-2 data gradient: 36 * Cout * Cin bf16 each (hi, lo) */
int ds_pack_conv_weight_dgrad_s2_bf16(const float *w_oihw, void *w_hi, void *w_lo, int Cout, int Cin,
                                      void *stream);
/* data gradient: 3x3 stride 1 (banks of ds_pack_conv_weight_dgrad_bf16) or 5x5 stride 2 (banks of
 * ds_pack_conv_weight_dgrad_s2_bf16; `s` is the FORWARD layer shape in both cases) */
int ds_conv_dgrad_bf16(const ds_conv_shape *s, const float *gy, const void *w_hi, const void *w_lo,
                       float *gx, void *stream);
int ds_conv_bf16_stats_rows(const ds_conv_shape *s, int x3);
/* tiling the bf16 planner picks: out8 = {M tile, N tile, rows per segment, segments per tile, workgroups,
 * LDS bytes, threads per workgroup, LDS row pitch in pixel records} */
int ds_conv_bf16_plan_describe(const ds_conv_shape *s, int x3, int *out8);
/* the same under the DS_CONV_PLAN_LATENCY bit of `flags` (what ds_conv_fwd_bf16 would launch) */
int ds_conv_bf16_plan_describe_hinted(const ds_conv_shape *s, int x3, int flags, int *out8);
void ds_conv_bf16_set_forced_cfg(int cfg);  /* tuning hook, as ds_conv_f16_set_forced_cfg */
/* tuning hook: how the bf16x3 forward launches walk the contraction.  0 (default): the pipelined walk (two pixel tiles
 * in LDS, one barrier per chunk, fragment and filter fetches inside the MFMA stream) for the launches
 * DS_CONV_PLAN_LATENCY re-plans, the classic walk for every other; 1: classic everywhere; 2: pipelined for every
 * bf16x3 forward launch -- DS_ERR_UNSUPPORTED where the planned tile has no such kernel.  Both walks give the same bits. */
void ds_conv_bf16_set_walk(int walk);
/* the walk ds_conv_fwd_bf16 would take under `flags`: 1 = classic, 2 = pipelined, or an error code */
int ds_conv_bf16_plan_walk(const ds_conv_shape *s, int x3, int flags);
int ds_conv_fwd_bf16(const ds_conv_shape *s, const float *x, const void *w_hi, const void *w_lo,
                     const float *scale, const float *shift, const float *residual, float *y,
                     float *stats_partial, int flags, void *stream);

/* ---- fp16 matrix cores: the eval-forward throughput path ------------------------------------------
 * Same layers and epilogue as ds_conv_fwd_f32 (model.py:69-80,192-205 in module.eval()), computed with
 * v_mfma_f32_32x32x16_f16 (fp16 operands, f32 accumulate) on fp16 channels-last activations
 * [B,H,W,C].  One MFMA per product: the embedding lands 3.7e-4 from the reference (contract 1e-3).
 * x, residual, y are fp16 buffers (y is f32 with DS_EPI_OUT_F32); DS_EPI_STATS is not supported. */
/* OIHW f32 -> [Cin/16][KS*KS][Cout][16] fp16 (round to nearest even) */
int ds_pack_conv_weight_f16(const float *w_oihw, void *w_f16, int Cout, int Cin, int KS, void *stream);
int ds_conv_fwd_f16(const ds_conv_shape *s, const void *x_f16, const void *w_f16, const float *scale,
                    const float *shift, const void *residual_f16, void *y, int flags, void *stream);
/* The same for SMALL launches (serving latency, reference model.py:185-218 on one or a few utterances): when the tile
 * grid cannot fill the GPU the contraction is split over up to 8 workgroups per tile (raw f32 partial sums in
 * `workspace`) and a second kernel folds them in fixed order and applies the epilogue.  Differs from
 * ds_conv_fwd_f16 by the f32 summation order only; large launches take the one-pass path. */
long long ds_conv_f16_splitk_workspace_bytes(const ds_conv_shape *s);
int ds_conv_fwd_f16_splitk(const ds_conv_shape *s, const void *x_f16, const void *w_f16, const float *scale,
                           const float *shift, const void *residual_f16, void *y, int flags, void *workspace,
                           long long ws_bytes, void *stream);
/* out8 = {M tile, N tile, rows per segment, segments per tile, workgroups, LDS bytes, threads per workgroup,
 * 1000 * double-buffered + 100 * (16-channel chunks) + staging items per thread} */
int ds_conv_f16_plan_describe(const ds_conv_shape *s, int *out8);
/* the same under the DS_CONV_HINT_* / DS_CONV_IN_PLANES16 bits of `flags` (what ds_conv_fwd_f16 would launch) */
int ds_conv_f16_plan_describe_hinted(const ds_conv_shape *s, int flags, int *out8);
/* the pixel tile's LDS layout in that plan: out4 = {records per tile row, bytes per tile row, bytes per segment,
 * 1000 x LDS cycles of one fragment read (1000 = free of bank conflicts)} */
int ds_conv_f16_plan_lds_layout(const ds_conv_shape *s, int flags, int *out4);
/* tuning hook: 1 = pad tile rows / segments by 16-byte units until a fragment read is free of bank conflicts in the
 * planner's model; default 0 (whole records only: measured equal, tools/ab_layout.py) */
void ds_conv_f16_set_layout_padding(int on);
void ds_conv_f16_set_forced_cfg(int cfg);   /* tuning hook: plan with tile configuration `cfg` only (-1: the planner's choice) */
/* One whole BasicBlock in eval mode as ONE kernel (reference model.py:66-82):
 *     y = clip(bn2(conv3x3(clip(bn1(conv3x3(x))))) + x)
 * for the shallow stages (W = 32 with 64 channels, W = 16 with 128: ds_conv_block_f16_supported), where a workgroup
 * of the single-layer kernel spends more time in its prologue and epilogue than contracting.  The intermediate
 * activation lives in LDS only.  Bit-identical to two ds_conv_fwd_f16 calls.  flags: DS_EPI_OUT_F32, DS_EPI_OUT_PLANES16. */
int ds_conv_block_f16_supported(int B, int H, int W, int C);
int ds_conv_block_f16(const void *x_f16, const void *wa_f16, const void *wb_f16, const float *scale_a,
                      const float *shift_a, const float *scale_b, const float *shift_b, void *y, int B, int H, int W,
                      int C, int flags, void *stream);
/* the same block over a zero-padded batch of utterances of different lengths (BASELINE configs[4]): `lens` (device,
 * int32 [B]) = the rows of each image that belong to its utterance; rows past them come out zero after both layers, as
 * ds_mask_rows leaves them in the unfused sequence */
int ds_conv_block_f16_masked(const void *x_f16, const void *wa_f16, const void *wb_f16, const float *scale_a,
                             const float *shift_a, const float *scale_b, const float *shift_b, void *y, const int *lens,
                             int B, int H, int W, int C, int flags, void *stream);
int ds_cast_f32_to_f16(const float *x, void *y_f16, long long n, void *stream);
int ds_cast_f16_to_f32(const void *x_f16, float *y, long long n, void *stream);

/* ---- tail: temporal average pool, L2 normalisation --------------------------------------------- */
/* x [B,Hr,Wc,C] -> pooled [B, Wc*C] (index f*C + c), mean over Hr  (model.py:111,207-208) */
int ds_avgpool_time_f32(const float *x, float *pooled, int B, int Hr, int Wc, int C, void *stream);
/* e = alpha * f / sqrt(sum f^2 + eps) per row  (model.py:172-183, 210-213) */
int ds_l2norm_scale_f32(const float *f, float *e, int B, int D, float alpha, float eps,
                        void *stream);

/* out2[0] = max |a - b|, out2[1] = max |b| over n floats (one workgroup, fixed fold order): the embedding-error
 * measure of the tests (max |d| / max |ref|) on the device -- what the fp16 precision guard of
 * DeepSpeakerModel.forward (model.py:185-218 in eval mode) compares its fp16 and f32-class sample rows with */
int ds_max_abs_diff_f32(const float *a, const float *b, long long n, float *out2, void *stream);

/* fused projection + normalisation: f = pooled . W^T + b  (model.py:209), e = alpha f / |f|
 * (model.py:210-213).  Split-K MFMA GEMM + a deterministic reduce; `workspace` holds
 * ds_fc_workspace_floats(B,K,N) floats; `bias` and `e` may be NULL (plain GEMM, used by the backward
 * pass for gpooled = gf . W). */
long long ds_fc_workspace_floats(int B, int K, int N);
int ds_fc_l2norm_fwd_f32(const float *pooled, const float *w_packed, const float *bias,
                         float *workspace, float *f, float *e, int B, int K, int N, float alpha,
                         float eps, void *stream);

/* ---- loss side ----------------------------------------------------------------------------------- */
/* d[i] = sqrt(sum_k (x1[i,k]-x2[i,k])^2 + 1e-4/D)   (PairwiseDistance, model.py:13-18, p = 2) */
int ds_pairwise_distance_f32(const float *x1, const float *x2, float *d, int N, int D,
                             void *stream);
/* the same for any norm p > 0: pow(sum_k |x1 - x2|^p + 1e-4 / D, 1 / p) (reference model.py:13-18 with self.norm = p;
 * the reference's own call sites pass 2), and its gradient */
int ds_pairwise_distance_p_f32(const float *x1, const float *x2, float *d, int N, int D, float p, void *stream);
int ds_pairwise_distance_p_bwd_f32(const float *x1, const float *x2, const float *d, const float *gd, float *g1,
                                   float *g2, int N, int D, float p, void *stream);
/* TripletMarginLoss.forward (model.py:27-33): writes d_p[N], d_n[N] and loss[1] = mean hinge. */
int ds_triplet_margin_fwd_f32(const float *a, const float *p, const float *n, float margin,
                              float *d_p, float *d_n, float *loss, int N, int D, void *stream);
/* the reference's triplet "mining" (train_triplet.py:251-262): idx = ascending i with
 * d_n[i] - d_p[i] < margin; count[0] = number selected; mean_diff[0] = mean(d_n - d_p). */
int ds_triplet_filter_f32(const float *d_p, const float *d_n, float margin, long long *idx,
                          int *count, float *mean_diff, int N, void *stream);
/* The loss side of one triplet step in two launches (distances, then one scan): loss (model.py:27-33), the
 * ordered filter + mean(d_n - d_p) (train_triplet.py:253-262) and, when amb_cap > 0, the ordered list of near
 * ties |d_n - d_p - margin| < band (first amb_cap of them; unused slots hold 0; amb_count = true count).  The near
 * ties are what a reduced-precision forward may decide differently from the reference: the caller re-embeds them
 * at f32-class precision, patches their distances with ds_refine_distances_f32 (e_ref rows: anchors | positives |
 * negatives, cap each) and re-runs the scan with ds_triplet_scan_f32. */
int ds_triplet_tail_f32(const float *a, const float *p, const float *n, float margin, float band, float *d_p,
                        float *d_n, float *loss, long long *idx, int *count, float *mean_diff, long long *amb_idx,
                        int *amb_count, int amb_cap, int N, int D, void *stream);
int ds_triplet_scan_f32(const float *d_p, const float *d_n, float margin, float *loss, long long *idx, int *count,
                        float *mean_diff, int N, void *stream);
int ds_refine_distances_f32(const float *e_ref, const long long *amb_idx, const int *amb_count, int cap, float *d_p,
                            float *d_n, int D, void *stream);
/* Round 4: the same two calls with PROBES -- how the band of the near-tie refinement checks itself.  The refinement
 * re-embeds all `cap` slots whether near ties fill them or not; ds_triplet_tail_probe_f32 puts the triplets
 * (probe_base + k) mod N, k = 0, 1, ... into the slots the near ties leave unused (probe_base < 0: none, == ds_triplet_tail_f32),
 * and ds_refine_distances_probe_f32 patches ALL cap slots and reports err[0] = max over the slots of
 * |(d_n - d_p) at f32-class precision - (d_n - d_p) before| (the fp16 forward's error on the filter's decision variable,
 * train_triplet.py:251-253) and err[1] = the number of slots sampled (as float); "before" is read from d_p_before /
 * d_n_before, the unpatched distances the scan chose the slots on (buffers other than d_p / d_n).  With the path's own
 * embeddings emb_a / emb_p / emb_n [N][D] (all or none) also err[2] = max |e_ref - emb| and err[3] = max |e_ref| over the
 * 3 * cap sampled rows: the path's distance to the 1e-3 embedding contract, watched on the same sample (err holds 4 floats).
 * One workgroup, no atomics. */
int ds_triplet_tail_probe_f32(const float *a, const float *p, const float *n, float margin, float band, float *d_p,
                              float *d_n, float *loss, long long *idx, int *count, float *mean_diff, long long *amb_idx,
                              int *amb_count, int amb_cap, int probe_base, int N, int D, void *stream);
int ds_refine_distances_probe_f32(const float *e_ref, const long long *amb_idx, const int *amb_count, int cap, float *d_p,
                                  float *d_n, const float *d_p_before, const float *d_n_before, const float *emb_a,
                                  const float *emb_p, const float *emb_n, int D, float *err, void *stream);
/* Round 6: the same in one launch instead of five (two clones, the patch, two read-back copies): d_p / d_n [N] are WRITTEN
 * (= d_p_before / d_n_before with the cap slots patched) and err5 holds five floats, err5[4] = the near-tie count. */
int ds_refine_distances_fused_f32(const float *e_ref, const long long *amb_idx, const int *amb_count, int cap, float *d_p,
                                  float *d_n, const float *d_p_before, const float *d_n_before, const float *emb_a,
                                  const float *emb_p, const float *emb_n, int N, int D, float *err5, void *stream);


/* ---- backward of the convolution stack (torch autograd of nn.Conv2d / nn.BatchNorm2d under
 *      loss.backward(), train_triplet.py:223,290) -------------------------------- */
/* filter bank of the 5x5 stride-2 data gradient: four parity classes, see ds_conv_dgrad_f32 */
int ds_pack_conv_dgrad_s2_f32(const float *w_oihw, float *w_packed, int Cout, int Cin, void *stream);
/* gx[B,H,W,Cin] = dL/dx given gy[B,Ho,Wo,Cout] = dL/dy of the convolution described by `s` (the
 * FORWARD shape).  w_dgrad_packed: ds_pack_conv_weight_f32(..., dgrad=1) for stride 1,
 * ds_pack_conv_dgrad_s2_f32 for the 5x5 stride-2 layers. */
int ds_conv_dgrad_f32(const ds_conv_shape *s, const float *gy, const float *w_dgrad_packed,
                      float *gx, void *stream);
/* gw_oihw[Cout,Cin,KS,KS] = dL/dW given the layer input x[B,H,W,Cin] and gy[B,Ho,Wo,Cout].  Pixel-split
 * MFMA GEMM + deterministic reduce; `workspace`: ds_conv_wgrad_workspace_floats(s) floats.  Cin = 1
 * selects the conv1 kernel.  fc_F > 0: `s` is the fc layer as a 1x1 convolution over [1,B,1,K] and
 * the result is written in the reference's [N, C*F] feature order (model.py:164,208). */
long long ds_conv_wgrad_workspace_floats(const ds_conv_shape *s);
int ds_conv_wgrad_f32(const ds_conv_shape *s, const float *x, const float *gy, float *workspace,
                      float *gw_oihw, int fc_F, void *stream);
/* the same filter gradient on the bf16 matrix cores with split operands (bf16x3, f32-class accuracy):
 * 3x3 stride 1 and 5x5 stride 2 layers with Cin, Cout multiples of 64.  `workspace`:
 * ds_conv_wgrad_bf16_workspace_floats(s) floats.  Deterministic (fixed-order reduction). */
long long ds_conv_wgrad_bf16_workspace_floats(const ds_conv_shape *s);
int ds_conv_wgrad_bf16(const ds_conv_shape *s, const float *x, const float *gy, float *workspace,
                       float *gw_oihw, void *stream);
/* BatchNorm (train mode) backward in one call: gy = (g1 [+ g2]) masked by the clipped-ReLU of `act`
 * (NULL: unmasked); reductions sum gy, sum gy*xhat; ggamma, gbeta; gz = dL/d(conv output).
 * partial: ds_bn_bwd_partial_rows(n_pix, C) * C * 2 floats; coef: 3*C floats; gy is written (it is the
 * masked gradient the residual branch re-uses).  This is the G = 1 case of ds_bn_bwd_group_f32 below (the same kernels,
 * three launches, no member_sums); the package's own Python calls the grouped form. */
int ds_bn_bwd_partial_rows(long long n_pix, int C);
int ds_bn_bwd_f32(const float *g1, const float *g2, const float *act, const float *z,
                  const float *mean, const float *invstd, const float *gamma, float *gy,
                  float *partial, float *coef, float *ggamma, float *gbeta, float *gz,
                  long long n_pix, int C, void *stream);
/* the same for a batch made of G members with their own batch statistics (the three forwards of a triplet step run as
 * one batch, train_triplet.py:215), in four launches: tensors [G * n_pix, C]; mean, invstd [G][C]; partial
 * G * ds_bn_bwd_partial_rows(n_pix, C) * C * 2 floats; coef [G][3C]; member_sums [2][G][C] scratch; ggamma / gbeta [C] =
 * the members' gradients added in member order (what three backward passes accumulate into .grad).  G = 1: three
 * launches, dgamma / dbeta are written in place and member_sums is not touched. */
int ds_bn_bwd_group_f32(const float *g1, const float *g2, const float *act, const float *z, const float *mean,
                        const float *invstd, const float *gamma, float *gy, float *partial, float *coef,
                        float *member_sums, float *ggamma, float *gbeta, float *gz, long long n_pix, int C, int G,
                        void *stream);
/* ds_bn_bwd_group_f32 split where data-parallel training exchanges the sums (new capability, the
 * reference is single-GPU: train_triplet.py:97): local reductions of all G members -> sums [G][2C+1] float64
 * ({sum gy, sum gy*xhat} per channel, then the member's pixel count) ... the caller all-reduces `sums` over RCCL ...
 * -> coefficients, dgamma / dbeta (members added in order) and gz of all members.  2 + 3 launches per layer. */
int ds_bn_bwd_group_reduce_f32(const float *g1, const float *g2, const float *act, const float *z,
                               const float *mean, const float *invstd, float *gy, float *partial, double *sums,
                               long long n_pix, int C, int G, void *stream);
int ds_bn_bwd_group_apply_f32(const double *sums, const float *gy, const float *z, const float *mean,
                              const float *invstd, const float *gamma, float *coef, float *member_sums,
                              float *ggamma, float *gbeta, float *gz, long long n_pix, int C, int G, void *stream);
/* The 3x3 stride-1 data gradient FUSED with the first half of the BatchNorm backward of the layer it feeds (autograd of
 * y = clip(bn1(conv1(r))) / r = clip(bn(conv(x))) under loss.backward(), train_triplet.py:223 over model.py:69-75,187-189):
 *   gy = (dgrad(gz_up) [+ g2]) * [0 < z * mask_scale + mask_shift < 20],  partial[row] = { sum gy, sum gy * xhat }
 * i.e. ds_conv_dgrad_bf16 followed by the reduce kernel of ds_bn_bwd_group_f32, without the gradient's round trip
 * through HBM and without reading the activation (the clipped-ReLU mask is re-derived from the layer's own
 * pre-activation z with the very fma of ds_bn_apply_f32).  `s`: the FORWARD shape of the convolution whose data gradient
 * this is; z / g2 / gy [B,H,W,Cin]; the batch = G members of B/G utterances with their own statistics, tables
 * mean / invstd / mask_scale / mask_shift [G][Cin].  ds_conv_dgrad_bnbwd_bf16_rows: partial rows PER MEMBER (partial =
 * G * rows * Cin * 2 floats), or DS_ERR_UNSUPPORTED when a tile of the launch would straddle two members (fall back to
 * ds_conv_dgrad_bf16 + ds_bn_bwd_group_f32).  ds_bn_bwd_group_finish_f32 is the second half (coefficients, dgamma /
 * dbeta added in member order, gz); data-parallel training puts ds_partial_sum_f64_group -> all-reduce ->
 * ds_bn_bwd_group_apply_f32 in its place. */
int ds_conv_dgrad_bnbwd_bf16_rows(const ds_conv_shape *s, int G);
int ds_conv_dgrad_bnbwd_bf16(const ds_conv_shape *s, const float *gz_up, const void *w_hi, const void *w_lo,
                             const float *g2, const float *z, const float *mean, const float *invstd,
                             const float *mask_scale, const float *mask_shift, int G, float *gy, float *partial,
                             void *stream);
/* the 5x5 stride-2 data gradient with the same fusion; it feeds a BasicBlock's OUTPUT out = clip(bn2(conv2(y)) + r)
 * (model.py:76-80), whose mask needs the stored activation `act` (= the 5x5 layer's input, [B,H,W,Cin]); nothing is
 * added.  Four parity-class launches write interleaved pixels of gy and consecutive blocks of the members' partial rows
 * (ds_conv_dgrad_s2_bnbwd_bf16_rows: rows per member over all four). */
int ds_conv_dgrad_s2_bnbwd_bf16_rows(const ds_conv_shape *s, int G);
int ds_conv_dgrad_s2_bnbwd_bf16(const ds_conv_shape *s, const float *gz_up, const void *w_hi, const void *w_lo,
                                const float *act, const float *z, const float *mean, const float *invstd, int G,
                                float *gy, float *partial, void *stream);
int ds_bn_bwd_group_finish_f32(const float *partial, int n_partial, const float *gy, const float *z, const float *mean,
                               const float *invstd, const float *gamma, float *coef, float *member_sums, float *ggamma,
                               float *gbeta, float *gz, long long n_pix, int C, int G, void *stream);
/* forward counterpart: per-tile partial statistics of G members (n_partial rows of [C][2] each, consecutive)
 * -> sums [G][2C+1] float64 (count in the last slot of each row) in one launch */
int ds_partial_sum_f64_group(const float *partial, int n_partial, double *sums, long long count, int C, int G,
                             void *stream);
int ds_colsum_f32(const float *x, float *out, int R, int C, void *stream);

/* ---- split forms for data-parallel training (one process per GPU): the caller all-reduces the
 *      [C][2] float64 sums over RCCL between the two halves, so that N ranks normalise with the
 *      statistics of the GLOBAL batch exactly like one process would.  count == 0:
 *      the (all-reduced) pixel count is read from sums[2*C] on the device -- no host sync.
 *      ds_partial_sum_f64, ds_bn_bwd_reduce_f32 and ds_bn_bwd_apply_f32 are the G = 1 cases of
 *      ds_partial_sum_f64_group, ds_bn_bwd_group_reduce_f32 (without its fold) and ds_bn_bwd_group_apply_f32
 *      (with an explicit count); ds_partial_sum_f64 writes [C][2] only, never the count slot. ------- */
int ds_partial_sum_f64(const float *partial, int n_partial, double *sums, int C, void *stream);
int ds_bn_stats_from_sums_f32(const double *sums, long long count, const float *gamma,
                              const float *beta, float eps, float momentum, float *running_mean,
                              float *running_var, float *batch_mean, float *batch_invstd,
                              float *scale, float *shift, int C, void *stream);
int ds_bn_bwd_reduce_f32(const float *g1, const float *g2, const float *act, const float *z,
                         const float *mean, const float *invstd, float *gy, float *partial,
                         long long n_pix, int C, void *stream);
int ds_bn_bwd_apply_f32(const double *sums, long long count, const float *gy, const float *z,
                        const float *mean, const float *invstd, const float *gamma, float *coef,
                        float *ggamma, float *gbeta, float *gz, long long n_pix, int C, void *stream);

/* row gather and its adjoint (selection of mined candidates and the gradient back to them) */
int ds_gather_rows_f32(const float *src, const long long *idx, float *dst, int N, int D, void *stream);
/* dst [3][N][D] = the rows idx[0..N) of three sources in one launch (the utterances of the near-tie triplets; a negative
 * index gathers zeros); D % 4 == 0, pointers 16-byte aligned */
int ds_gather_rows3_f32(const float *src_a, const float *src_p, const float *src_n, const long long *idx, float *dst,
                        int N, int D, void *stream);
int ds_scatter_add_rows_f32(const float *g, const long long *idx, float *dst, int N, int M, int D,
                            int accumulate, void *stream);

/* ---- cross-GPU semi-hard negative search over an all-gathered candidate set (north_star; no
 *      reference counterpart).  out_index[i] in [0,M) or -1; out_dist may be NULL.
 *      For anchor i: among the candidates of another label, the closest one with distance > d_p[i]; without such a one the
 *      closest of another label; the lowest index among bit-equal distances; -1 (out_dist 0) when every candidate shares
 *      the label.  The distances are the search's own f32 sums (eps = 1e-4 / D inside the root), so a candidate whose
 *      distance equals d_p[i] to rounding may fall on either side of the strict comparison.
 *      D % 4 == 0 and D <= DS_MINE_MAX_D: a workgroup keeps at least two anchor rows (2 * D floats) next to its 36 KiB
 *      candidate tile in 64 KiB of LDS; a longer row is DS_ERR_BAD_SHAPE and nothing is launched. ---- */
#define DS_MINE_MAX_D 3584
long long ds_mine_workspace_floats(int N, int M);
int ds_mine_semihard_f32(const float *anchor, const float *d_p, const long long *anchor_label,
                         const float *cand, const long long *cand_label, float *workspace,
                         long long *out_index, float *out_dist, int N, int M, int D, void *stream);

/* ---- backward of the loss side and the tail (torch autograd of the lines cited above; the
 *      reference obtains them from loss.backward(), train_triplet.py:223,290) ------------------- */
int ds_pairwise_distance_bwd_f32(const float *x1, const float *x2, const float *d, const float *gd,
                                 float *g1, float *g2, int N, int D, void *stream);
/* grad_loss points at ONE device float (dL/dloss); clamp(min=0) passes gradient at exactly 0. */
int ds_triplet_margin_bwd_f32(const float *a, const float *p, const float *n, const float *d_p,
                              const float *d_n, float margin, const float *grad_loss, float *ga,
                              float *gp, float *gn, int N, int D, void *stream);
int ds_l2norm_scale_bwd_f32(const float *f, const float *ge, float *gf, int B, int D, float alpha,
                            float eps, void *stream);
/* backward of [clip(0,20) -> mean over time]: gx = (0 < out < 20) ? gpooled / Hr : 0 */
int ds_avgpool_time_bwd_f32(const float *gpooled, const float *out, float *gx, int B, int Hr, int Wc,
                            int C, void *stream);


/* Softmax pre-training head in one call (model.py:220-223 + train_triplet.py:281-285): logits = x W^T + b on the
 * f32 matrix cores with row max / log-sum-exp / per-row loss taken in the split-K reduction's epilogue, then the
 * mean.  N = n_cls padded to a multiple of 128 (zero filter rows); logits is [M, N]. */
int ds_fc_ce_fwd_f32(const float *x, const float *w_packed, const float *bias, float *workspace, float *logits,
                     const long long *labels, float *row_loss, float *lse, float *loss, int M, int K, int N,
                     int n_cls, void *stream);

/* ---- softmax cross-entropy of the classifier logits (nn.CrossEntropyLoss, mean reduction;
 *      train_triplet.py:281-287).  logits [M, ld] with n_cls valid columns; lse[M] and row_loss[M] are
 *      outputs of the forward that the backward re-uses; dlogits [M, ld_out], columns >= n_cls zeroed. -- */
int ds_cross_entropy_fwd_f32(const float *logits, const long long *labels, float *row_loss, float *lse,
                             float *loss, int M, int n_cls, int ld, void *stream);
int ds_cross_entropy_bwd_f32(const float *logits, const long long *labels, const float *lse,
                             const float *grad_loss, float *dlogits, int M, int n_cls, int ld, int ld_out,
                             void *stream);

/* ---- angular-margin softmax head (margin_head.hip): AAM-softmax / ArcFace and AM-softmax / CosFace on the
 *      classifier's weight, f32.  With x^, w^ the L2-normalised rows (an all-zero row stays zero):
 *        c[i,j] = clamp(x^_i . w^_j, -1, 1);   z[i,j] = scale c[i,j] for j != y_i,   z[i,y_i] = scale phi(c[i,y_i])
 *        DS_MARGIN_AM:   phi = c - m                                                      dphi/dc = 1
 *        DS_MARGIN_AAM:  phi = c cos m - sn sin m,  sn = sqrt(max(1 - c^2, DS_MARGIN_SIN2_FLOOR))   where c > -cos m
 *                                                                                         dphi/dc = cos m + c sin m / sn
 *                        phi = c - m sin m  otherwise (ArcFace's monotone fallback)        dphi/dc = 1
 *        loss = mean_i (logsumexp_{j < n_cls} z[i,j] - z[i,y_i])
 *      scale > 0, 0 <= margin < pi/2 (else DS_ERR_BAD_SHAPE); another kind is DS_ERR_UNSUPPORTED.  Labels in [0, n_cls)
 *      are the caller's promise: no entry point reads device memory back, and none indexes memory by a label.
 * ds_row_normalize_f32: x [R, K] -> xhat [R_out, K] = rows / norm and inv [R_out] = 1 / norm (both 0 for an all-zero
 *   row); rows R .. R_out-1 are written as zeros (class rows padded to a multiple of 128 for the two weight packers).
 * ds_fc_margin_ce_fwd_f32: xhat [M, K]; w_packed = ds_pack_fc_weight_f32(what [N, K], N, K, 1), N = n_cls padded to a
 *   multiple of 128; K % 32 == 0.  The split-K GEMM's reduction epilogue folds the K-slices, clamps, stores c [M, N]
 *   (pad columns 0), applies the margin and takes lse [M] and row_loss [M] over the n_cls real columns in one pass;
 *   loss = their mean.  workspace: ds_fc_margin_workspace_floats(M, K, N) floats, 16-byte aligned.
 * ds_fc_cosine_fwd_f32: the same GEMM and c; cos_out [M, n_cls] = scale c, no margin and no loss.
 * ds_margin_ce_bwd_f32: gc [M, N] = scale (grad_loss[0] / M) (exp(z - lse) - [j == y_i]), the label column times
 *   dphi/dc, pad columns 0 (the clamp passes gradient everywhere); r [M] = sum_j gc c; q [N] = sum_i gc c, summed in one
 *   fixed order without atomics.  ds_cosine_bwd_f32: the same outputs for gc = scale grad_out [M, n_cls].
 * ds_margin_grad_fixup_f32: out [R, K] = inv[row] (g - coef[row] u), rows of K % 4 == 0 floats: with A = gc what
 *   (ds_fc_l2norm_fwd_f32 on ds_pack_fc_weight_dgrad_f32's layout) and Bm = gc^T xhat (ds_conv_wgrad_f32, a 1x1
 *   convolution over the M rows),  dL/dx = fixup(A, xhat, r, inv_x)  and  dL/dW = fixup(Bm, what, q, inv_w).
 * Every sum has one order that depends on its row (q: its column and M) alone: two calls agree bit for bit, and a
 * row's c, loss and gradient do not depend on the other rows of the batch. ---- */
#define DS_MARGIN_AAM 0
#define DS_MARGIN_AM  1
#define DS_MARGIN_SIN2_FLOOR 1e-6f
int ds_row_normalize_f32(const float *x, float *xhat, float *inv, int R, int R_out, int K, void *stream);
long long ds_fc_margin_workspace_floats(int M, int K, int N);
int ds_fc_margin_ce_fwd_f32(const float *xhat, const float *w_packed, float *workspace, float *c,
                            const long long *labels, float *row_loss, float *lse, float *loss, int M, int K, int N,
                            int n_cls, float scale, float margin, int kind, void *stream);
int ds_fc_cosine_fwd_f32(const float *xhat, const float *w_packed, float *workspace, float *c, float *cos_out, int M,
                         int K, int N, int n_cls, float scale, void *stream);
int ds_margin_ce_bwd_f32(const float *c, const long long *labels, const float *lse, const float *grad_loss, float *gc,
                         float *r, float *q, int M, int N, int n_cls, float scale, float margin, int kind,
                         void *stream);
int ds_cosine_bwd_f32(const float *c, const float *grad_out, float *gc, float *r, float *q, int M, int N, int n_cls,
                      float scale, void *stream);
int ds_margin_grad_fixup_f32(const float *g, const float *u, const float *coef, const float *inv, float *out, int R,
                             int K, void *stream);

/* ---- variable-length batches (BASELINE configs[4]; the temporal mean pool of model.py:207 accepts any T) --------
 * Utterances of different lengths share one zero-padded batch [B,1,Tmax,64].  ds_mask_rows re-zeroes, after every
 * layer, the rows past each utterance's own extent (lens[b] rows of the [H][row_bytes] slab of image b are kept):
 * those zeros then act exactly like the utterance's own zero padding, so every kept row is bit-identical to the
 * forward of the utterance alone.  ds_avgpool_time_masked_f32 averages over the utterance's own rows.
 * lens[b] is clamped to [0, H] by both: lens[b] <= 0 zeroes the whole image / pools to 0 (no row is read), lens[b] > H
 * keeps / averages all H rows. */
int ds_mask_rows(void *x, const int *lens, int B, int H, long long row_bytes, void *stream);
int ds_avgpool_time_masked_f32(const float *x, const int *lens, float *pooled, int B, int Hr, int Wc, int C,
                               void *stream);
/* out[i] = mean of x[offsets[i] .. offsets[i+1]): enrolment sets of different sizes (train_triplet.py:350 takes the
 * mean of a trial's distances) */
int ds_segment_mean_f32(const float *x, const long long *offsets, float *out, int n_seg, void *stream);

/* ---- speaker identification (csrc/identify.hip): enrolled speaker models and a fused top-k search ----
 * ds_nearest_topk_f32: for each of queries[N,D] the k gallery[M,D] rows (row-major f32, 16-byte aligned) with the
 *   smallest SCREENING distance s = (|q|^2 + |g|^2) - 2 q.g, q.g from the f32 MFMA; the N x M matrix is never written.
 *   Rows are ordered by (s, gallery index): ties go to the lowest index, and the bits of s for a pair depend on the pair
 *   alone -- not on its tile, on `splits` or on the other rows.  out_dist / out_index [N,k] (s and int64 row numbers,
 *   ascending); ranks that cannot be filled (fewer than k eligible rows) are (+inf, -1).
 *   mode 0: every gallery row is eligible (the labels may be NULL); 1: rows whose label equals the query's are skipped
 *   (hardest negatives); 2: only those rows.  query_label[N], gallery_label[M] int64.
 *   splits: gallery ranges searched by separate workgroups and folded afterwards; 0 = chosen from the CU count.
 *   1 <= k <= DS_NEAREST_MAX_K, D % 4 == 0 and D <= DS_NEAREST_MAX_D, else DS_ERR_BAD_SHAPE.
 *   workspace: ds_nearest_workspace_bytes(N, M, D, k, splits) bytes (row norms + the splits' lists), 16-byte aligned.
 * ds_nearest_rescore_f32: the distance of every (query, index[n,r]) pair again, bit-identical to
 *   ds_pairwise_distance_f32 of the two rows (direct differences, eps = 1e-4 / D inside the root), and each query's k
 *   entries in ascending (distance, index) order; (-1) entries stay last as (+inf, -1).  Not in place.
 * ds_segment_mean_rows_f32: models[s,:] = mean of emb[offsets[s] .. offsets[s+1]) (rows added in order, f32);
 *   renorm != 0: then (m / sqrt(sum m^2 + eps)) * alpha, the arithmetic of ds_l2norm_scale_f32.
 * ds_rank_hits_i32: hits[r] = number of queries n whose query_label[n] equals gallery_label[index[n,r']] for some
 *   r' <= r (index < 0 never matches): rank-(r+1) identification counts, reduced in a fixed order. */
#define DS_NEAREST_MAX_K 64
#define DS_NEAREST_MAX_D 2048
long long ds_nearest_workspace_bytes(int N, int M, int D, int k, int splits);
int ds_nearest_topk_f32(const float *queries, const float *gallery, const long long *query_label,
                        const long long *gallery_label, int mode, void *workspace, float *out_dist,
                        long long *out_index, int N, int M, int D, int k, int splits, void *stream);
int ds_nearest_rescore_f32(const float *queries, const float *gallery, const long long *index, float *out_dist,
                           long long *out_index, int N, int M, int D, int k, void *stream);
int ds_segment_mean_rows_f32(const float *emb, const long long *offsets, float *models, int S, int D, int renorm,
                             float alpha, float eps, void *stream);
int ds_rank_hits_i32(const long long *index, const long long *gallery_label, const long long *query_label, int *hits,
                     int N, int k, void *stream);

/* ---- score normalisation (csrc/score_norm.hip): Z / T / S / AS-norm ----
 * ds_cohort_stats_f32: for each row of emb[N,D] the min(K, eligible) rows of cohort[M,D] (row-major f32, 16-byte
 *   aligned) with the smallest SCREENING value s -- the value of ds_nearest_topk_f32, bit for bit: both run one function
 *   (csrc/screen_tile.h) -- ordered by (s, cohort index), ties at the K-th value to the lowest indices; then
 *   mean[n] / std[n] = mean and population standard deviation (ddof 0) of the DISTANCES to those rows, recomputed by
 *   direct differences in the arithmetic of ds_pairwise_distance_f32 (eps = 1e-4 / D inside the root) and reduced in two
 *   passes (mean, then sum (d - mean)^2) in a fixed order over the index-ordered selection; count[n] = how many rows.
 *   K == M: every eligible row (Z / T / S-norm); K < M: the adaptive forms.  The selection is an exact radix select
 *   over the row's M values held in LDS as order-preserving keys (negative s included), which sets DS_COHORT_MAX_M.
 *   mode / labels as ds_nearest_topk_f32 (0: all rows; 1: skip rows with the row's own label; 2: only those); a row
 *   with fewer than K eligible cohort rows takes them all, with none: count 0, mean +inf, std 0.
 *   selected: NULL, or int32 [N, ceil(M / 32)]: bit (j % 32) of word j / 32 is set iff cohort row j was selected.
 *   row_block: rows whose screening values are alive at once, [row_block x M] in the workspace (never N x M); 0 = chosen
 *   by the library.  mean, std and selected are bit-identical whatever N, row_block or the position in the batch.
 *   1 <= K <= M <= DS_COHORT_MAX_M, D % 4 == 0, D <= DS_NEAREST_MAX_D, else DS_ERR_BAD_SHAPE (workspace query: -1).
 *   workspace: ds_cohort_workspace_bytes(N, M, D, K, row_block) bytes, 16-byte aligned.
 * ds_score_norm_apply_f32: out[t] = ((raw[t] - mean_a[ia]) / max(std_a[ia], min_std)
 *   + (raw[t] - mean_b[ib]) / max(std_b[ib], min_std)) / 2 with ia = a_index[t], ib = b_index[t] (int64 rows of the
 *   statistics tables; NULL: t itself); mean_b and std_b both NULL: the first term alone, without the 1/2. */
#define DS_COHORT_MAX_M 32768
long long ds_cohort_workspace_bytes(int N, int M, int D, int K, int row_block);
int ds_cohort_stats_f32(const float *emb, const float *cohort, const long long *emb_label, const long long *cohort_label,
                        int mode, void *workspace, float *mean, float *std, int *count, int *selected, int N, int M,
                        int D, int K, int row_block, void *stream);
int ds_score_norm_apply_f32(const float *raw, const long long *a_index, const long long *b_index, const float *mean_a,
                            const float *std_a, const float *mean_b, const float *std_b, float min_std, float *out, int T,
                            void *stream);

/* ---- verification scoring on the device --------------------------------------
 * ds_group_mean_f32: score of a trial = mean over G crop-pair distances (train_triplet.py:347-350).
 * ds_roc_sweep_f32: the threshold sweep of eval_metrics.py:5-50 (predict = dist < thr; tp/fp per
 * threshold thr0 + i*dthr) plus a summary {best-accuracy threshold index (first argmax), tpr, fpr,
 * accuracy there, EER, EER threshold}; the reference computes no EER. -------------------- */
int ds_group_mean_f32(const float *x, float *out, int n_groups, int G, void *stream);
int ds_roc_sweep_f32(const float *dist, const int *issame, int N, float thr0, float dthr, int n_thr,
                     int n_same, int n_diff, int *tp, int *fp, float *summary6, void *stream);

/* ---- small-batch tail (serving latency, round 4): temporal mean + 2048 -> 512 projection in one launch for
 *      B <= DS_TAIL_SMALL_MAX_B utterances, then the norm (model.py:207-213).  w_rows = the fc filter as [N][K'] rows in
 *      the pooled vector's f*C + c order (ds_pack_fc_weight_rows_f32).  Agrees with ds_avgpool_time_f32 +
 *      ds_fc_l2norm_fwd_f32 to f32 rounding (another summation order), 8 us instead of 30 at B = 1. ---- */
#define DS_TAIL_SMALL_MAX_B 4
int ds_pack_fc_weight_rows_f32(const float *w, float *w_rows, int N, int C, int F, void *stream);
int ds_tail_small_f32(const float *a, const float *w_rows, const float *bias, float *f, float *e, int B, int Hr, int K,
                      int N, float alpha, float eps, void *stream);

/* ---- OPT-IN fp16 training step (round 4; DeepSpeakerModel(train_precision="f16")): the triplet-regime step of
 *      train_triplet.py:215-224 with every activation, pre-activation and gradient tensor fp16 in HBM, the convolutions
 *      (forward AND data gradients) on ds_conv_fwd_f16 -- one fp16 MFMA per product, f32 accumulate -- and f32
 *      statistics / parameter gradients.  Gradient tensors hold S * g for a constant loss scale S (a power of two);
 *      what leaves in f32 (dgamma, dbeta, filter gradients) is un-scaled by `inv_scale` / `out_scale` = 1 / S.
 *      Tolerances (tests/test_gpu_train_f16.py, measured at 768 rows in brackets): loss 1e-3 (3.5e-4), train-mode
 *      embeddings 2e-3 (1.15e-3), gradients 8e-3 of the masked oracle (4.0e-3 worst, 1.4e-3 median; the reference's own fp32
 *      run is 4e-3 from its fp64 run on unmasked gradients). ---- */
/* data-gradient filter banks for ds_conv_fwd_f16.  stride 1: Cout*Cin*KS*KS halfs, [Cout/16][tap][Cin][16] with taps
 * flipped -- run with shape {B, Ho, Wo, Cin' = Cout, Cout' = Cin, KS, 1} over dL/d(conv output).  stride 2 (KS = 5):
 * 36*Cout*Cin halfs, [Cout/16][9][4 Cin][16] -- the four parity classes of dX as the output-channel blocks of ONE 3x3
 * stride-1 convolution {B, Ho, Wo, Cout, 4 Cin, 3, 1}; its output [B][Ho][Wo][2][2][Cin] is read in place by
 * ds_bn_bwd_group_f16(g1_parity = 1). */
int ds_pack_conv_weight_dgrad_f16(const float *w_oihw, void *w_f16, int Cout, int Cin, int KS, int stride, void *stream);
/* train-mode BatchNorm statistics of G members (rows [m*n_pix, (m+1)*n_pix) of z) -> [G][C] tables; running statistics
 * updated member after member (the reference's three forward calls); partial: G * ds_bn_f16_partial_rows(n_pix, C) * C * 2
 * floats of scratch.  Replaces nn.BatchNorm2d.train() forward bookkeeping (model.py:59,62,94,99,103,107). */
int ds_bn_f16_partial_rows(long long n_pix, int C);
int ds_bn_stats_group_f16(const void *z_f16, float *partial, long long n_pix, const float *gamma, const float *beta,
                          float eps, float momentum, float *running_mean, float *running_var, float *mean_t,
                          float *invstd_t, float *scale_t, float *shift_t, int C, int G, void *stream);
/* y = clip(z * scale[m] + shift[m] (+ residual)); flags: DS_EPI_RESIDUAL | DS_EPI_CLIP | DS_EPI_OUT_F32 (y f32: the last
 * stage, whose consumer is the f32 pooling / projection tail).  model.py:70-71,74-80,188-189 in train mode. */
int ds_bn_apply_group_f16(const void *z_f16, const float *scale_t, const float *shift_t, const void *res_f16, void *y,
                          long long n_pix, int C, int G, int flags, void *stream);
/* backward of BatchNorm(train) + clipped ReLU for G members: gy = (g1 [+ g2]) * mask, gz = dL/d(conv output); ggamma /
 * gbeta [C] summed over the members and un-scaled.  mask = 0 < act < 20 (act fp16, or f32 with act_is_f32), or -- act NULL,
 * mask_scale_t / mask_shift_t = the forward's [G][C] scale / shift tables -- 0 < fp16(clip(z * scale + shift)) < 20 taken
 * from the layer's own pre-activation (no third tensor read), or none (all NULL: g1 is already masked).  gy may be NULL
 * with the z-derived mask (no g2, no parity layout): the masked gradient is then never stored.
 * partial as above; coef [G][3 C] scratch.  H, W: the layer's map (used when g1_parity). */
int ds_bn_bwd_group_f16(const void *g1, int g1_parity, const void *g2, const void *act, int act_is_f32,
                        const float *mask_scale_t, const float *mask_shift_t, const void *z, const float *mean_t,
                        const float *invstd_t, const float *gamma, void *gy, float *partial, float *coef, float *ggamma,
                        float *gbeta, void *gz, long long n_pix, int H, int W, int C, int G, float inv_scale, void *stream);
/* data-parallel split forms (one process per GPU): partial sums only / the reduction only, then -- after
 * ds_partial_sum_f64_group(partial, ds_bn_f16_partial_rows(n_pix, C), sums, n_pix, C, G) and an all-reduce of the
 * [G][2C+1] float64 sums over RCCL -- ds_bn_stats_from_sums_f32 per member (forward) / ds_bn_bwd_group_apply_f16 (backward:
 * coefficients, dgamma / dbeta, gz from the GLOBAL sums; regen: gy was not stored, gy_or_g1 is g1 and the mask tables
 * are given).  An N-rank step then equals the single-process step on the global batch. */
int ds_bn_stats_partial_f16(const void *z_f16, float *partial, long long n_pix, int C, int G, void *stream);
int ds_bn_stats_from_sums_group_f32(const double *sums, const float *gamma, const float *beta, float eps, float momentum,
                                    float *running_mean, float *running_var, float *mean_t, float *invstd_t,
                                    float *scale_t, float *shift_t, int C, int G, void *stream);   /* all G members, one launch */
int ds_bn_bwd_group_reduce_f16(const void *g1, int g1_parity, const void *g2, const void *act, int act_is_f32,
                               const float *mask_scale_t, const float *mask_shift_t, const void *z, const float *mean_t,
                               const float *invstd_t, void *gy, float *partial, long long n_pix, int H, int W, int C, int G,
                               void *stream);
int ds_bn_bwd_group_apply_f16(const double *sums, const void *gy_or_g1, int regen, const float *mask_scale_t,
                              const float *mask_shift_t, const void *z, const float *mean_t, const float *invstd_t,
                              const float *gamma, float *coef, float *ggamma, float *gbeta, void *gz, long long n_pix, int C,
                              int G, float inv_scale, void *stream);
int ds_scale_cast_f32_to_f16(const float *x, void *y_f16, long long n, float scale, void *stream);
/* filter gradients from fp16 activations x and fp16 loss-scaled output gradients gy (cuDNN wgrad under
 * loss.backward(), train_triplet.py:223): 3x3 / 5x5, stride 1 / 2, Cin and Cout multiples of 64. */
long long ds_conv_wgrad_f16_workspace_floats(const ds_conv_shape *s);
int ds_conv_wgrad_f16(const ds_conv_shape *s, const void *x_f16, const void *gy_f16, float *workspace, float *gw_oihw,
                      float out_scale, void *stream);
/* conv1 (Cin = 1): f32 network input, fp16 output gradient; workspace ds_conv_wgrad_workspace_floats(s) floats */
int ds_conv_wgrad_c1_f16(const ds_conv_shape *s, const float *x, const void *gy_f16, float *workspace, float *gw_oihw,
                         float out_scale, void *stream);

/* ---- batch assembly on the device: out[b, t, :] = features[row_start[b] + t, :]
 *      for t < T, zero past row_end[b]; features = the corpus' [frames, F] fbank matrices concatenated
 *      and resident in HBM.  Replaces the host-side np.load + crop + transpose + H2D of
 *      audio_processing.py:38-74,185 / DeepSpeakerDataset_dynamic.py:82-103 per batch. ---------------- */
int ds_assemble_crops_f32(const float *features, const long long *row_start, const long long *row_end,
                          float *out, int B, int T, int F, void *stream);

/* ---- fused multi-tensor optimizer steps: one launch updates every parameter
 *      tensor; replaces torch.optim.{Adagrad,SGD,Adam}.step() of train_triplet.py:369-383,224,291 with
 *      the same arithmetic.  `params`, `grads`, `state1`, `state2` are DEVICE arrays of device pointers
 *      (one per tensor), `numel` a device int64 array; workgroup b updates elements
 *      [chunk_index[b]*ds_optim_chunk_elems(), +ds_optim_chunk_elems()) of tensor chunk_tensor[b]. ---- */
/* Steps that are captured into a HIP graph and replayed: the step count lives on the device (`step_count`, int32 [1],
 * bumped by ds_optim_step_inc once per optimizer step unless the skip flag is set) and Adagrad's decayed learning rate /
 * Adam's bias corrections are computed from it inside the kernel, in double precision as the host computes them. */
int ds_optim_step_inc(int *step_count, const int *skip_flag, void *stream);
int ds_adagrad_step_dev_f32(const void *params, const void *grads, const void *state1, const void *state2,
                            const long long *numel, const int *chunk_tensor, const int *chunk_index, int n_chunks,
                            double lr, double lr_decay, float weight_decay, float eps, const int *step_count,
                            const int *skip_flag, void *stream);
int ds_sgd_step_dev_f32(const void *params, const void *grads, const void *state1, const void *state2,
                        const long long *numel, const int *chunk_tensor, const int *chunk_index, int n_chunks, float lr,
                        float momentum, float dampening, float weight_decay, const int *step_count, const int *skip_flag,
                        void *stream);      /* the momentum buffers start at the step that counts 1 */
int ds_adam_step_dev_f32(const void *params, const void *grads, const void *state1, const void *state2,
                         const long long *numel, const int *chunk_tensor, const int *chunk_index, int n_chunks, float lr,
                         double beta1, double beta2, float eps, float weight_decay, const int *step_count,
                         const int *skip_flag, void *stream);
/* `bytes` (<= 2048, a multiple of 4) of a HOST table -> device memory as kernel arguments: no staging buffer, legal inside a
 * stream capture (a replayed graph writes the same values again).  The fused optimizers' pointer tables travel this way. */
int ds_fill_bytes(void *dst, const void *host_src, int bytes, void *stream);
int ds_optim_chunk_elems(void);
int ds_adagrad_step_f32(const void *params, const void *grads, const void *state1, const void *state2,
                        const long long *numel, const int *chunk_tensor, const int *chunk_index,
                        int n_chunks, float clr, float weight_decay, float eps, const int *skip_flag,
                        void *stream);
int ds_sgd_step_f32(const void *params, const void *grads, const void *state1, const void *state2,
                    const long long *numel, const int *chunk_tensor, const int *chunk_index, int n_chunks,
                    float lr, float momentum, float dampening, float weight_decay, int first_step,
                    const int *skip_flag, void *stream);
int ds_adam_step_f32(const void *params, const void *grads, const void *state1, const void *state2,
                     const long long *numel, const int *chunk_tensor, const int *chunk_index, int n_chunks,
                     float lr, float beta1, float beta2, float eps, float weight_decay,
                     float bias_correction1, float bias_correction2_sqrt, const int *skip_flag, void *stream);
/* `skip_flag` (nullable, device): non-zero = the launch leaves parameters and state untouched -- the overflow flag of a
 * loss-scaled fp16 training step, read on the device (no host round trip; torch.amp.GradScaler's found_inf).
 * ds_nonfinite_flag_f32: *flag = 1 if any of x[0..n) is inf or NaN (never cleared here: the tensors of one step
 * accumulate into one flag the caller zeroed). */
int ds_nonfinite_flag_f32(const float *x, long long n, int *flag, void *stream);

/* ---- log-mel filterbank front end (fbank.hip): waveforms -> [T_u, nfilt] f32 features, the reference's mk_MFB
 * (python_speech_features.fbank with a rectangular window, pre-emphasis 0.97, then 20*log10(max(fb, 1e-5)) and
 * normalize_frames).  Utterances are packed end to end; every buffer is the caller's.
 * ds_fbank_plan (HOST): from the host sample counts `lengths[n_utt]`, the frame counts and the tile table.  With
 *   table == NULL only counts[3] = {total frames, tiles, frames per tile} is written; otherwise also the int64 table
 *   samp_off[n_utt+1] | frame_off[n_utt+1] | tile_off[n_utt+1] | tile_utt[tiles] (3 * (n_utt + 1) + tiles entries),
 *   which the caller copies to the device.  An empty signal is DS_ERR_BAD_SHAPE; frame_len > nfft, nfft not a power of
 *   two in 64..1024, nfilt not a multiple of 4 in 4..128, or a tile that does not fit the LDS is DS_ERR_UNSUPPORTED.
 * ds_fbank_workspace_bytes: the f64 workspace: per-tile partial sums [tiles][2][nfilt], then per-utterance statistics
 *   [n_utt][2][nfilt].
 * ds_fbank_logmel_f32: samples f32 (in_int16 = 0) or int16 PCM scaled by 1/32768 (in_int16 = 1); table (device) from
 *   ds_fbank_plan; basis [frame_len rounded up to even][nfft] f32 with column 64p + j = cos(2 pi n k / nfft) and
 *   64p + 32 + j = sin(...) for bin k = 32p + j (column 32 holds cos of the Nyquist bin instead of sin_0); band
 *   [nfilt][2] int32 = {first bin, count} and mel_w [nfilt][wstride] f32 the filters' nonzero weights.  out
 *   [frames][nfilt] f32: 20*log10(max(fb, 1e-5)) (log_scale != 0) or fb; the workspace receives the tiles' partials.
 * ds_fbank_normalize_f32: after ds_fbank_logmel_f32 on the same stream and workspace: per utterance and filter, the mean
 *   over its frames is subtracted (use_scale: and the result divided by std + 2e-12, population std), in place.
 *   Deterministic: partials are reduced in a fixed order, so an utterance's features do not depend on its batch. */
int ds_fbank_plan(const long long *lengths, int n_utt, int frame_len, int frame_step, int nfft, int nfilt, long long *table,
                  long long *counts);
long long ds_fbank_workspace_bytes(int n_utt, int n_tiles, int nfilt);
int ds_fbank_logmel_f32(const void *samples, int in_int16, const long long *table, int n_utt, int n_tiles,
                        const float *basis, const int *band, const float *mel_w, int wstride, int frame_len,
                        int frame_step, int nfft, int nfilt, int log_scale, float *out, double *workspace, void *stream);
/* the kernels' pre-emphasis of one signal of n samples alone (y[0] = x[0], y[i] = x[i] - 0.97 x[i-1] in f32 with two
 * roundings): a test hook for the staging arithmetic */
int ds_fbank_preemphasis_f32(const void *samples, int in_int16, long long n, float *out, void *stream);
int ds_fbank_normalize_f32(float *feat, const long long *table, int n_utt, int n_tiles, int nfilt, int tile_rows,
                           int use_scale, double *workspace, void *stream);

/* ---- rational polyphase resampler (resample.hip): packed waveforms at one rate -> packed mono f32 at another, the
 * resampling and down-mix of the reference's librosa.load(filename, sr=16000, mono=True).  With up = new_rate / g and
 * down = orig_rate / g (g their gcd) and a windowed-sinc table h of 2 * half_width + 1 taps,
 *   y[m] = sum_k x[k] * h[half_width + m * down - k * up]   (0 <= k < n, taps outside the table are zero),
 *   n_out = ceil(n * up / down).
 * Every output is one fmaf chain over ascending k: deterministic, independent of tile, batch and call.  Every buffer is
 * the caller's.
 * ds_resample_plan (HOST): from the host frame counts `lengths[n_utt]`.  With table == NULL only counts[3] = {total
 *   outputs, tiles, outputs per tile} is written; otherwise also the int64 table in_off[n_utt+1] | out_off[n_utt+1] |
 *   tile_off[n_utt+1] | tile_utt[tiles] (3 * (n_utt + 1) + tiles entries), which the caller copies to the device.  An
 *   empty utterance is DS_ERR_BAD_SHAPE.  DS_ERR_UNSUPPORTED: with T = ceil((2 * half_width + 1) / up) taps per output,
 *   a polyphase table of more than 16384 entries (up * (T | 1)), or a tile whose input span does not fit the LDS next to
 *   the table (down / up in the hundreds).
 * ds_resample_poly_f32: samples f32 (in_int16 = 0) or int16 PCM scaled by 1/32768 (in_int16 = 1), interleaved
 *   [frames][channels] with 1 <= channels <= 8 (else DS_ERR_UNSUPPORTED): the channels of a frame are summed in order in
 *   f32 and the sum divided by `channels` in f32 before filtering.  table (device) from ds_resample_plan.  taps (device):
 *   the table in polyphase form [up][T | 1] f32, row p = the taps of outputs with (half_width + m * down) % up == p in the
 *   order of ascending input index: entry [p][j] = h[p + (T - 1 - j) * up], zero where that index exceeds 2 * half_width
 *   and in the padding column.  out [total outputs] f32. */
int ds_resample_plan(const long long *lengths, int n_utt, int up, int down, int half_width, long long *table,
                     long long *counts);
int ds_resample_poly_f32(const void *samples, int in_int16, int channels, const long long *table, int n_utt, int n_tiles,
                         const float *taps, int up, int down, int half_width, float *out, void *stream);

/* ---- energy voice-activity decision and selection of the voiced frames (csrc/vad.hip), on the filterbank's framing ----
 * The rule (Kaldi's compute-vad-energy / select-voiced-frames, not bit-compatible with it), for an utterance of T frames:
 *   e[t]   = ln(max(sum_i (32768 x[t * frame_step + i])^2, energy_floor)), 0 <= i < frame_len: raw samples (no
 *            pre-emphasis, window or DC removal), zero past the utterance's end; int16 enters as its integer value
 *   thr    = energy_threshold + energy_mean_scale * mean_t e[t]      (f64, accumulated in a fixed order, no atomics)
 *   voiced = count(e[lo..hi] > thr) >= proportion_threshold * (hi - lo + 1), lo = max(0, t - frames_context),
 *            hi = min(T - 1, t + frames_context): the window is clipped to the utterance
 * Every frame is summed in one fixed order: deterministic, independent of tile, batch and call.  Every buffer is the
 * caller's; nothing is allocated or synchronised.
 * ds_vad_log_energy_f32: samples as for ds_fbank_logmel_f32, table (device) and tile_rows (counts[2]) from ds_fbank_plan;
 *   out [total frames] f32.  The frames at the floor hold (float)log(energy_floor) exactly.  energy_floor not a positive
 *   finite float, frame_len or frame_step < 1: DS_ERR_BAD_SHAPE; a tile whose samples do not fit the LDS:
 *   DS_ERR_UNSUPPORTED.
 * ds_vad_tile_frames: frames per workgroup of the decision kernels.
 * ds_vad_plan (HOST): from the host frame offsets frame_off[n_utt + 1] (an utterance may have no frame).  With
 *   table == NULL only counts[3] = {total frames, decision tiles, frames per tile} is written; otherwise also the int64
 *   table frame_off[n_utt+1] | dtile_off[n_utt+1] | dtile_utt[tiles] (2 * (n_utt + 1) + tiles entries), which the caller
 *   copies to the device.  Tiles never straddle utterances.  Offsets that decrease, or 2^31 frames in one utterance:
 *   DS_ERR_BAD_SHAPE.
 * ds_vad_workspace_bytes: the workspace of ds_vad_decide / ds_vad_scan: thresholds f64 [n_utt], tile counts int64 [tiles].
 * ds_vad_decide: energy [frames] f32 -> mask [frames] uint8 (1 = voiced), scan [frames] int32 (the exclusive scan of the
 *   mask INSIDE each utterance) and kept [n_utt] int64.  Four launches: thresholds, vote + tile counts, scan of the
 *   tile counts per utterance, scan inside the tiles -- an utterance may span any number of workgroups and none waits
 *   for another.  frames_context < 0, proportion_threshold outside (0, 1] or a non-finite parameter: DS_ERR_BAD_SHAPE;
 *   frames_context > 64: DS_ERR_UNSUPPORTED.
 * ds_vad_scan: scan and kept of a caller's own mask (non-zero = kept).
 * ds_vad_select_f32: the kept rows of feat [frames][nfilt] f32, in order, packed into out [sum kept][nfilt].  ktable
 *   (device): the ds_fbank_plan layout over the KEPT frames -- samp_off (not read) | frame_off | tile_off | tile_utt with
 *   tile_rows rows per tile, an utterance without kept frames without tiles -- built by the caller from `kept`.
 *   workspace: ds_fbank_workspace_bytes(n_utt, n_ktiles, nfilt); its per-tile {sum, sum of squares} [n_ktiles][2][nfilt]
 *   f64 over the kept rows are written in ds_fbank_logmel_f32's layout and order, so ds_fbank_normalize_f32 with ktable
 *   normalises over the kept rows. */
int ds_vad_tile_frames(void);
int ds_vad_plan(const long long *frame_off, int n_utt, long long *table, long long *counts);
long long ds_vad_workspace_bytes(int n_utt, int n_dtiles);
int ds_vad_log_energy_f32(const void *samples, int in_int16, const long long *table, int n_utt, int n_tiles, int tile_rows,
                          int frame_len, int frame_step, double energy_floor, float *out, void *stream);
int ds_vad_decide(const float *energy, const long long *vtable, int n_utt, int n_dtiles, double energy_threshold,
                  double energy_mean_scale, int frames_context, double proportion_threshold, unsigned char *mask, int *scan,
                  long long *kept, void *workspace, void *stream);
int ds_vad_scan(const unsigned char *mask, const long long *vtable, int n_utt, int n_dtiles, int *scan, long long *kept,
                void *workspace, void *stream);
int ds_vad_select_f32(const float *feat, const unsigned char *mask, const int *scan, const long long *vtable,
                      const long long *ktable, int n_utt, int n_ktiles, int nfilt, int tile_rows, float *out,
                      double *workspace, void *stream);

/* ---- waveform augmentation (csrc/augment.hip): reverberation, additive noise at an SNR and the output level, on packed
 * waveforms.  For utterance u of n samples x (int16 PCM scaled by 1/32768), an impulse response h of K taps with delay
 * p (0 <= p < K) and up to 8 noise clips v_j with starts s_j:
 *   r[m] = sum_k h[k] * x[m + p - k]   (0 <= m < n, 0 <= k < K, x zero outside [0, n): np.convolve(x, h)[p : p + n]);
 *          r = x for an utterance without an impulse response
 *   s[m] = r[m] + sum_j g_j * v_j[(s_j + m) mod len_j],  g_j = sqrt(P_r / (P_vj * 10^(snr_j / 10))), 0 when a power is 0
 *   y    = s * sqrt(P_x / P_s)   (y = s when P_s = 0)
 * P_x, P_r, P_s: mean squares over the utterance, accumulated in f64 in one fixed order; P_vj: the mean square of the
 * whole clip, from the caller.  r is an f32 MFMA product of 32 x 32 Toeplitz blocks of h against the samples folded
 * into columns of 32; every output is one fmaf chain fixed by its position in its utterance: deterministic, independent
 * of tile, batch and call.  Every buffer is the caller's; nothing is allocated, read back or synchronised.
 * ds_augment_plan (HOST): from the host sample counts `lengths[n_utt]`.  With table == NULL only counts[4] = {total
 *   samples, tiles, outputs per tile, taps the reverberation kernel takes per pass} is written; otherwise also the int64
 *   table off[n_utt+1] | tile_off[n_utt+1] | tile_utt[tiles] (2 * (n_utt + 1) + tiles entries), which the caller copies
 *   to the device.  Tiles never straddle utterances.  An empty utterance is DS_ERR_BAD_SHAPE.
 * ds_augment_workspace_bytes: the f64 workspace [tiles][3] = per-tile sums of x^2, r^2, s^2.
 * ds_augment_reverb_f32: samples f32 (in_int16 = 0) or int16 (in_int16 = 1) -> out [total samples] f32 = r, and the
 *   tiles' sums of x^2 and r^2 in the workspace.  rir_bank (device): the impulse responses, packed f32; rir_tab
 *   (device): int64 [n_utt][3] = {offset of the utterance's h in rir_bank, or -1 for none; K; p}.  Both NULL: every
 *   utterance is copied.  max_taps: the largest K of the call; above 65536 DS_ERR_UNSUPPORTED.
 * ds_augment_mix_f32: data = r -> s in place, and the tiles' sums of s^2.  noise_tab (device): int64
 *   [n_utt][n_noises][5] = {offset of the clip in noise_bank, or -1 for none; its length (< 2^31); s_j (0 <= s_j <
 *   length); the bits of P_vj as f64; the bits of 10^(snr_j / 10) as f64}.  g_j is rounded to f32 once and s is one
 *   fmaf chain over j.  n_noises > 8: DS_ERR_UNSUPPORTED.
 * ds_augment_level_f32: data = s -> y in place; mixed = 1 after ds_augment_mix_f32, 0 straight after
 *   ds_augment_reverb_f32 (s = r). */
int ds_augment_plan(const long long *lengths, int n_utt, long long *table, long long *counts);
long long ds_augment_workspace_bytes(int n_tiles);
int ds_augment_reverb_f32(const void *samples, int in_int16, const long long *table, int n_utt, int n_tiles,
                          const float *rir_bank, const long long *rir_tab, int max_taps, float *out, double *workspace,
                          void *stream);
int ds_augment_mix_f32(float *data, const long long *table, int n_utt, int n_tiles, const float *noise_bank,
                       const long long *noise_tab, int n_noises, double *workspace, void *stream);
int ds_augment_level_f32(float *data, const long long *table, int n_utt, int n_tiles, int mixed, const double *workspace,
                         void *stream);

/* ---- speaker diarisation (csrc/ahc.hip): within-recording distance matrices of a packed batch of recordings and their
 * agglomerative hierarchical clustering, one recording per workgroup.  Recording r owns rows row_off[r] .. row_off[r+1]
 * of emb[N,D] (n_r of them, 0 <= n_r <= DS_AHC_MAX_N); its n_r x n_r f32 matrix lies at entry sum_{q<r} n_q^2 of the
 * packed matrices, its n_r - 1 merge steps at sum_{q<r} max(n_q - 1, 0) of the step arrays, its leaves at row_off[r].
 * Every buffer is the caller's; nothing is allocated, read back or synchronised, and no kernel uses an atomic or waits
 * for another workgroup.  A recording's results are bit-identical whatever else is in the batch.
 * ds_ahc_plan (HOST): from the host offsets row_off[n_rec + 1] (row_off[0] == 0).  With table == NULL only counts[6] =
 *   {total rows, distance tiles, rows per tile, matrix entries, merge steps, largest n_r} is written; otherwise also
 *   the int64 table row_off | mat_off | step_off | tile_off (n_rec + 1 entries each) | tile_rec[tiles], which the caller
 *   copies to the device.  A tile is a (rows per tile)^2 block of one recording's upper triangle.  Offsets that
 *   decrease, n_r above DS_AHC_MAX_N, D < 1 or D > DS_NEAREST_MAX_D: DS_ERR_BAD_SHAPE.
 * ds_ahc_workspace_bytes (HOST): the bytes of the packed matrices, the work area that the linkage consumes; -1 for
 *   offsets that ds_ahc_plan refuses.
 * ds_ahc_distances_f32: entry (i, j), i != j, is ds_pairwise_distance_f32 of rows i and j bit for bit (direct
 *   differences, eps = 1e-4 / D inside the root); computed once for i < j and stored on both sides; +inf on the
 *   diagonal.  n_tiles, tile_rows: counts[1], counts[2] of the plan for the same D.
 * ds_ahc_linkage_f32: the n_r - 1 merges of every recording, IN PLACE over its matrix (symmetric, NaN-free; consumed).
 *   Step s merges the active pair (a, b), a < b, with the smallest current distance, ties to the smallest a, then the
 *   smallest b.  The cluster lives on in slot a (a cluster's slot is its lowest member).  For every other active k:
 *     DS_AHC_SINGLE min(d_ak, d_bk); DS_AHC_COMPLETE max(d_ak, d_bk);
 *     DS_AHC_AVERAGE ((float)n_a * d_ak + (float)n_b * d_bk) / (float)(n_a + n_b): both products, the sum and the
 *     division each rounded to f32 (no fused multiply-add),
 *   written to row and column a.  pair [steps][2] int32 = (a, b); height [steps] f32 = the merged distance; size
 *   [steps] int32 = n_a + n_b; into / step [rows] int32 = the slot that absorbed slot i and at which step (-1, -1 for
 *   the survivor).  n_max: the largest n_r (counts[5]); above DS_AHC_MAX_N: DS_ERR_BAD_SHAPE; another method:
 *   DS_ERR_UNSUPPORTED.
 * ds_ahc_cut: labels [rows] int32 and n_found [n_rec] int32 from a linkage.  M = the number of leading steps with
 *   height <= threshold (it stops at the FIRST step above: f32 average linkage may invert by an ulp), at most
 *   n_r - n_clusters where that is given; leaf i follows `into` while step < M, to its cluster's lowest member; the label
 *   is the rank of that root among the roots: 0, 1, ... in order of first appearance.  threshold_mode / n_clusters_mode:
 *   0 not given, 1 the scalar, 2 one value per recording (device vectors); both 0: DS_ERR_UNSUPPORTED. */
#define DS_AHC_MAX_N 4096
#define DS_AHC_AVERAGE 0
#define DS_AHC_COMPLETE 1
#define DS_AHC_SINGLE 2
int ds_ahc_plan(const long long *row_off, int n_rec, int D, long long *table, long long *counts);
long long ds_ahc_workspace_bytes(const long long *row_off, int n_rec);
int ds_ahc_distances_f32(const float *emb, const long long *table, int n_rec, int n_tiles, int tile_rows, int D,
                         float *dist, void *stream);
int ds_ahc_linkage_f32(float *dist, const long long *table, int n_rec, int n_max, int method, int *pair, float *height,
                       int *size, int *into, int *step, void *stream);
int ds_ahc_cut(const long long *table, int n_rec, int n_max, const float *height, const int *into, const int *step,
               const float *threshold_vec, float threshold, int threshold_mode, const int *n_clusters_vec, int n_clusters,
               int n_clusters_mode, int *labels, int *n_found, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPSPEAKER_HIP_H */
