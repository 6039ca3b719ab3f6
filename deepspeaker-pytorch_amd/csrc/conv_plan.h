// conv_plan.h -- what the f32, bf16 and fp16 convolution planners (plan_tiles in conv_mfma_f32.hip, plan_bf16 in
// conv_mfma_bf16.hip, plan_f16 in conv_mfma_f16.hip) must agree on, each piece written once.  Plain host C++; the
// planners run on every launch, so everything here is a template or an inline function that takes the planner's own
// predicate by type (no std::function).  What differs stays with the planner: its tile table, its feasibility limits
// (staging items / LDS), its extra score factors and tie-break table, and everything after the search (pitch, LDS
// bytes, staging slots).
#pragma once
#include "ds_common.h"

// The chip the planners size their grids for: the MI355X's 256 CUs of 4 SIMDs.  Deliberately NOT ds_cu_count(): the
// recorded plans (tests/golden/conv_plans_f32_bf16.json, f16_conv_plans.json) and the host emulator, which reports 2
// CUs, depend on the constant; planning for the device actually present would be a change of behaviour, not a fold.
constexpr int kPlanCUs = 256;
constexpr int kPlanSIMDs = 4 * kPlanCUs;

// The checks every planner makes, in this order (the recorded bad-shape rows pin order and codes), and the output
// grid.  cin_multiple: input channels per chunk (8 f32, 16 bf16, 32 fp16); allow_1x1: the f32 kernel only.  grid_H /
// grid_W > 0 replace the forward convolution's output grid (the parity classes of a stride-2 data gradient).  The
// bounds that only some planners have -- B * Ho < 2^24, and the 2^30 / 2^31 output sizes -- stay with them.
static inline int ds_plan_check_shape(const ds_conv_shape *s, int cin_multiple, bool allow_1x1, int &Ho, int &Wo,
                                      int grid_H = 0, int grid_W = 0) {
    DS_REQUIRE(s != nullptr, DS_ERR_NULL);
    DS_REQUIRE(s->B > 0 && s->H > 0 && s->W > 0 && s->Cin > 0 && s->Cout > 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE((allow_1x1 && s->KS == 1) || s->KS == 3 || s->KS == 5, DS_ERR_UNSUPPORTED);
    DS_REQUIRE(s->stride == 1 || s->stride == 2, DS_ERR_UNSUPPORTED);
    DS_REQUIRE(s->Cin % cin_multiple == 0 && s->Cout % 64 == 0, DS_ERR_BAD_SHAPE);
    const int pad = s->KS / 2;
    Ho = grid_H > 0 ? grid_H : (s->H + 2 * pad - s->KS) / s->stride + 1;
    Wo = grid_W > 0 ? grid_W : (s->W + 2 * pad - s->KS) / s->stride + 1;
    DS_REQUIRE(Ho > 0 && Wo > 0 && Wo <= 128, DS_ERR_BAD_SHAPE);
    DS_REQUIRE((long long)s->B * s->H * s->W * s->Cin < (1ll << 31), DS_ERR_BAD_SHAPE);
    return DS_OK;
}

// The segmentations of a Ho x Wo output grid for an M tile of MT pixels: a segment is `rt` full-width output rows of
// one image, a tile holds `ni` segments -- as many as MT allows, at most all there are, shrunk until fits(ni, rows_in,
// cols_in) holds (the planner's limit: staging items, LDS); a height of which not even one segment fits is skipped.
// rows_in x cols_in is the input tile of one segment (input stride IS, ext_h x ext_w taps).  Calls
// visit(rt, ni, n_mt) with n_mt = M tiles of the launch.
template <class Fits, class Visit>
static inline void ds_plan_segmentations(int B, int Ho, int Wo, int MT, int IS, int ext_h, int ext_w, Fits &&fits,
                                         Visit &&visit) {
    for (int rt = 1; rt <= Ho; ++rt) {
        if ((long long)rt * Wo > MT) break;
        const int segs_per_img = ds_ceil_div(Ho, rt);
        const long long n_segs = (long long)B * segs_per_img;
        int ni = MT / (rt * Wo);
        if (ni > n_segs) ni = (int)n_segs;
        const int rows_in = IS * (rt - 1) + ext_h, cols_in = IS * (Wo - 1) + ext_w;
        while (ni > 1 && !fits(ni, rows_in, cols_in)) --ni;
        if (!fits(ni, rows_in, cols_in)) continue;
        visit(rt, ni, ds_ceil_div_ll(n_segs, ni));
    }
}

// The objective: (fraction of the tiles' MFMA rows that are real pixels) x (occupancy of the last round of
// workgroups).  The grid runs in rounds of (CUs x resident workgroups); a half-empty last round idles matrix cores
// just like masked rows do (measured: 768 workgroups at 2 per CU run at 0.84 of the rate of 256 or 512).  A grid that
// fits in one round is spread evenly over the CUs by the dispatcher.
// The planners add tie-breaks of 1e-6 and 1e-9 to this value: the operations and their order are part of the result.
static inline double ds_plan_fill_occupancy(int B, int Ho, int Wo, long long n_mt, int MT, long long blocks,
                                            int wg_per_cu) {
    double eff = (double)B * Ho * Wo / ((double)n_mt * MT);
    const long long slots = (long long)kPlanCUs * wg_per_cu;
    if (blocks <= slots) eff *= (double)blocks / (double)(ds_ceil_div_ll(blocks, kPlanCUs) * kPlanCUs);
    else eff *= (double)blocks / (double)(ds_ceil_div_ll(blocks, slots) * slots);
    return eff;
}

// The winner's geometry: the fields of ConvK / ConvKB / ConvKH (in `pl.k`) and of the plan that follow from
// (rt, ni) alone.  Same arguments as ds_plan_segmentations; NTILE = output channels per tile.
template <class Plan>
static inline void ds_plan_fill_geometry(Plan &pl, int B, int Ho, int Wo, int IS, int ext_h, int ext_w, int Cout,
                                         int NTILE, int rt, int ni) {
    auto &k = pl.k;
    k.RT = rt;
    k.NI = ni;
    k.segs_per_img = ds_ceil_div(Ho, rt);
    k.n_segs = B * k.segs_per_img;
    k.rows_in = IS * (rt - 1) + ext_h;
    k.cols_in = IS * (Wo - 1) + ext_w;
    k.n_ntiles = Cout / NTILE;
    pl.n_mtiles = ds_ceil_div(k.n_segs, ni);
    pl.grid = pl.n_mtiles * k.n_ntiles;
}

// The 5x5 stride-2 data gradient: pixel (2r + ph, 2c + pw) of dX only receives the taps kh = ph, kw = pw (mod 2), so
// dX splits into four parity classes cls = 2 ph + pw, each a dense stride-1 convolution over the dY grid that writes
// Hr x Wc pixels of dX.  A class of a one-row (one-column) map can be empty: it is skipped, but still owns its bank.
struct ds_s2_class {
    int ph, pw;
    int Hr, Wc;
    bool empty() const { return Hr <= 0 || Wc <= 0; }
};
static inline ds_s2_class ds_s2_class_of(int H, int W, int cls) {
    const int ph = cls >> 1, pw = cls & 1;
    return {ph, pw, (H - ph + 1) / 2, (W - pw + 1) / 2};
}
// the dY grid of an H x W input: the 5x5 stride-2 pad-2 forward's output
static inline int ds_s2_dy_rows(int H) { return (H - 1) / 2 + 1; }
static inline int ds_s2_dy_cols(int W) { return (W - 1) / 2 + 1; }
