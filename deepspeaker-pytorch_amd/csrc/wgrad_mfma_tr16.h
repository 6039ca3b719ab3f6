// wgrad_mfma_tr16.h -- filter gradients of the 3x3 / 5x5 convolution layers on the 16-bit matrix cores with
// transposing LDS reads: kernel, plan and launch, shared by the split-operand bf16 path (wgrad_mfma_bf16.hip, f32
// tensors) and the fp16 path (wgrad_mfma_f16.hip, fp16 tensors).  Each of the two supplies an `Ops` policy (the operand
// format) and its C entry points.
//
// dW[co][ci][kh][kw] = sum over (b, h, w) of dY[b,h,w,co] * X[b, s*h+kh-p, s*w+kw-p, ci]
// (autograd of nn.Conv2d under loss.backward(), reference train_triplet.py:223; layers model.py:47-50,
// 98-106).  As a GEMM: M = Cout, N = Cin, K = every output pixel of the batch.  Same decomposition as the
// f32 kernel (wgrad_mfma_f32.hip): workgroup = (tap group, 64 co, 64 ci, pixel split); per pixel tile the
// dY rows and the X halo tile are staged in LDS once and reused by every tap of the group; partial sums go
// to [split][tap][Cout][Cin] and wgrad_reduce_kernel folds them in a fixed order (deterministic).
//
// What is different: v_mfma_f32_32x32x16_{bf16,f16} contracts 16 pixels per instruction and wants, per lane, 8
// CONSECUTIVE pixels of ONE channel -- the transposed view of the channels-last activations.  The tiles
// stay pixel-major in LDS (one record of Ops::REC bytes per pixel, written with coalesced stores) and the
// operands are fetched with ds_read_b64_tr_b16: within a 16-lane group lane i supplies the
// 8-byte piece (row i>>2, column quad i&3) of a 4-pixel x 16-channel block and receives column i, i.e. 4
// pixels of its own channel.  Two such reads make one 8-element fragment; because every lane supplies its own
// pixel address, any tap offset or stride works without alignment constraints.
//
// Ops, a struct of constants and three inline functions:
//   ELEM                bytes per tensor element in HBM
//   QV                  16-byte staged items per pixel (64 / QV channels each): a staging slot is 256 / QV pixels
//   REC                 bytes per pixel record in LDS (data + pad: conflict-free transposing reads)
//   PARTS, PART_BYTES   fragment parts per operand and the byte distance between them inside a record
//   GSL3 / XSL3, GSL3_BIG / XSL3_BIG, GSL5 / XSL5      staging slots of the instantiations (see the kernel)
//   vec                 one fragment part (8 x 16 bit)
//   put(rec, q, v)      stage item q of a pixel: 16 bytes as loaded -> the record
//   join(a, b)          two transposing reads -> one fragment part
//   mma(a, b, c)        one tap's product of two fragments (PARTS parts each) added to c
#pragma once
#include <ds_device.h>
#include "ds_common.h"
#include "wgrad_reduce.h"

namespace {

constexpr int WB_C = 64;                     // channels per tile on both sides

struct WgradK {
    const void *x, *gz;
    float *partial;
    int H, W, Cin, Ho, Wo, Cout;
    int KS, IS, pad;
    int RT, NI, segs_per_img, n_segs, n_tiles;
    int rows_in, cols_in, seg_pix;
    int P;                       // output-pixel slots per tile (multiple of 16, >= NI*RT*Wo)
    int S, n_co_tiles, n_ci_tiles;
    unsigned x_bytes, gz_bytes;  // extents of x / gz (32-bit buffer offsets)
    int k0;                      // first kernel row of the group (5x5)
};

// one MFMA operand: pixels q0 .. q0+7 of this lane's channel, in Ops::PARTS parts
template <class Ops>
struct WgradFrag {
    typename Ops::vec part[Ops::PARTS];
};

// rec0 / rec1 are the byte addresses this lane supplies for the two 4-pixel blocks (its piece: pixel
// q0 + 4r + ((lane&15)>>2), quad lane&3)
template <class Ops>
__device__ __forceinline__ WgradFrag<Ops> frag_tr(const char *rec0, const char *rec1) {
    WgradFrag<Ops> f;
#pragma unroll
    for (int k = 0; k < Ops::PARTS; ++k)
        f.part[k] = Ops::join(ds_read_tr16_b64(rec0 + k * Ops::PART_BYTES), ds_read_tr16_b64(rec1 + k * Ops::PART_BYTES));
    return f;
}

// TG taps per workgroup, KW taps per kernel row.  <9, 3>: all of a 3x3.  A 5x5 runs as two launches over kernel-row
// GROUPS: rows k0, k0 + stride, ... (k0 = 0: three rows = <15, 5>; the other two = <10, 5>).  With the stride between
// a group's rows equal to the convolution stride, kernel row m of the group reads, for output row r, tile row r + m:
// the staged tile holds only the input rows of that residue (RT + rows - 1 of them), and each dY tile staged is
// contracted against 15 (10) taps instead of the 5 of a single kernel row.
// Four waves as 2 (co) x 2 (ci), each owning a 32 x 32 block of every tap of the group; the accumulators take most
// of the register file (one wave per SIMD).
// GSL / XSL: staging slots per thread (16 bytes each) for the dY rows and the X halo tile -- the tile's size in registers:
// (256 / QV) * GSL output pixels, (256 / QV) * XSL halo pixels.  A 3x3 (9 accumulators) has room for 8 + 14: tiles of
// that size halve the barriers, pipeline fills and halo rows per contracted pixel of the 4-slot ones; a 5x5 group
// (15 accumulators) keeps 4 + 12.
template <class Ops, int TG, int KW, int GSL, int XSL>
__global__ void __launch_bounds__(256) DS_ONE_WAVE_PER_SIMD wgrad_mfma_tr16_kernel(const WgradK p) {
    constexpr bool GROUP = KW == 5;                     // kernel-row group of a 5x5 (see above)
    constexpr int WB_REC = Ops::REC;
    char *lds = (char *)ds_dynamic_lds();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lhi = lane >> 5;
    const int co_sub = wave & 1, ci_sub = wave >> 1;

    int bid = blockIdx.x;
    const int sp = bid % p.S;
    bid /= p.S;
    const int cit = bid % p.n_ci_tiles;
    bid /= p.n_ci_tiles;
    const int cot = bid % p.n_co_tiles;

    const int tile_in_pix = p.NI * p.seg_pix;
    char *gzt = lds;                                    // [P] records
    char *xt = gzt + (size_t)p.P * WB_REC;              // [tile_in_pix] records
    int *pixtab = (int *)(xt + (size_t)tile_in_pix * WB_REC);   // [P] byte offset of each pixel's (0,0)-tap input record
    int *segtab = pixtab + p.P;                         // [2][NI][4] per-tile segment origins, double-buffered

    f32x16 acc[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    const int pix_per_seg = p.RT * p.Wo;
    constexpr int QV = Ops::QV, QC = WB_C / QV;         // 16-byte items per staged pixel, channels per item

    // ---- tile-invariant staging descriptors: per slot the element offset RELATIVE to the segment's origin and
    //      (segment << 16 | row); per tile only four numbers per segment change (segtab) ----
    int g_rel[GSL], g_sr[GSL], x_rel[XSL], x_sr[XSL];   // *_sr = -1: unused slot, -2: always-zero slot
    const int n_g = p.P * QV, n_x = tile_in_pix * QV;
#pragma unroll
    for (int it = 0; it < GSL; ++it) {
        const int i = tid + it * 256;
        g_sr[it] = -1;
        g_rel[it] = 0;
        if (i < n_g) {
            const int pp = i / QV, q = i - pp * QV;
            const int seg = pp / pix_per_seg, rem = pp - seg * pix_per_seg;
            const int r = rem / p.Wo, c = rem - r * p.Wo;
            g_sr[it] = (seg < p.NI) ? ((seg << 16) | r) : -2;
            g_rel[it] = (r * p.Wo + c) * p.Cout + cot * WB_C + q * QC;
        }
    }
#pragma unroll
    for (int it = 0; it < XSL; ++it) {
        const int i = tid + it * 256;
        x_sr[it] = -1;
        x_rel[it] = 0;
        if (i < n_x) {
            const int pix = i / QV, q = i - pix * QV;
            const int seg = pix / p.seg_pix, pr = pix - seg * p.seg_pix;
            const int rr = pr / p.cols_in, cc = pr - rr * p.cols_in;
            const int hrel = GROUP ? p.IS * rr + p.k0 : rr;            // image row = IS*r0 - pad + hrel
            const int w = cc - p.pad;
            x_sr[it] = (w >= 0 && w < p.W) ? ((seg << 16) | hrel) : -2;
            x_rel[it] = (hrel * p.W + cc) * p.Cin + cit * WB_C + q * QC;
        }
    }
    for (int pp = tid; pp < p.P; pp += 256) {
        const int seg = pp / pix_per_seg, rem = pp - seg * pix_per_seg;
        const int r = rem / p.Wo, c = rem - r * p.Wo;
        // GROUP: tile row j is image row IS*(r0 + j) - pad + k0, output row r's first tap sits in tile row r
        pixtab[pp] = (seg < p.NI) ? (seg * p.seg_pix + (GROUP ? r : p.IS * r) * p.cols_in + p.IS * c) * WB_REC : 0;
    }

    // software pipeline over tiles: the next tile's global loads are issued into registers before this
    // tile's matrix work and written to LDS (Ops::put) after it
    f32x4 gv[GSL], xv[XSL];
    auto fill_segtab = [&](int tile, int buf) {          // {dY origin, output rows left, X origin, first image row}
        if (tid < p.NI) {
            const int gseg = tile * p.NI + tid;
            int gbase = 0, rows_left = 0, xbase = 0, h0 = -(1 << 20);
            if (gseg < p.n_segs) {
                const int b = gseg / p.segs_per_img;
                const int r0 = (gseg - b * p.segs_per_img) * p.RT;
                gbase = (b * p.Ho + r0) * p.Wo * p.Cout;
                rows_left = p.Ho - r0;
                h0 = p.IS * r0 - p.pad;
                xbase = ((b * p.H + h0) * p.W - p.pad) * p.Cin;
            }
            int *e = segtab + (buf * p.NI + tid) * 4;
            e[0] = gbase; e[1] = rows_left; e[2] = xbase; e[3] = h0;
        }
    };
    // Branch-free: a slot's segment entry is read from LDS, its validity folded into the offset (out-of-range
    // offsets of a raw buffer load return 0) -- GSL + XSL independent loads per thread instead of as many
    // read -> compare -> branch -> load chains.
    const ds_buffer gbuf = ds_make_buffer(p.gz, p.gz_bytes), xbuf = ds_make_buffer(p.x, p.x_bytes);
    auto issue_loads = [&](int buf) {
        const int *st = segtab + buf * p.NI * 4;
        int g_org[GSL], g_rows[GSL], x_org[XSL], x_h0[XSL];
#pragma unroll
        for (int it = 0; it < GSL; ++it) {                 // every slot's segment entry, requested unconditionally
            const int *e = st + (g_sr[it] >= 0 ? (g_sr[it] >> 16) : 0) * 4;
            g_org[it] = e[0];
            g_rows[it] = e[1];
        }
#pragma unroll
        for (int it = 0; it < XSL; ++it) {
            const int *e = st + (x_sr[it] >= 0 ? (x_sr[it] >> 16) : 0) * 4;
            x_org[it] = e[2];
            x_h0[it] = e[3];
        }
#pragma unroll
        for (int it = 0; it < GSL; ++it) {                 // (the reads above must not sink into per-slot branches)
            DS_OPAQUE_VGPR(g_org[it]);
            DS_OPAQUE_VGPR(g_rows[it]);
        }
#pragma unroll
        for (int it = 0; it < XSL; ++it) {
            DS_OPAQUE_VGPR(x_org[it]);
            DS_OPAQUE_VGPR(x_h0[it]);
        }
#pragma unroll
        for (int it = 0; it < GSL; ++it) {
            const bool ok = (g_sr[it] >= 0) & ((g_sr[it] & 0xFFFF) < g_rows[it]);
            gv[it] = ds_buffer_load_f32x4(gbuf, ok ? (unsigned)(g_org[it] + g_rel[it]) * (unsigned)Ops::ELEM : DS_BUFFER_OOB);
        }
#pragma unroll
        for (int it = 0; it < XSL; ++it) {
            const int h = x_h0[it] + (x_sr[it] & 0xFFFF);
            const bool ok = (x_sr[it] >= 0) & (h >= 0) & (h < p.H);
            xv[it] = ds_buffer_load_f32x4(xbuf, ok ? (unsigned)(x_org[it] + x_rel[it]) * (unsigned)Ops::ELEM : DS_BUFFER_OOB);
        }
    };

    // this lane's piece of every transposing read: pixel (lane&15)>>2 of the 4-pixel block, channel quad
    // lane&3 of the 16-channel block (lane>>4)&1 of the wave's 32 channels
    const int piece_pix = (lane & 15) >> 2;
    const int a_col = (co_sub * 32 + ((lane >> 4) & 1) * 16 + (lane & 3) * 4) * 2;     // byte offset inside a fragment part
    const int b_col = (ci_sub * 32 + ((lane >> 4) & 1) * 16 + (lane & 3) * 4) * 2;

    fill_segtab(sp, 0);
    __syncthreads();
    if (sp < p.n_tiles) issue_loads(0);
    int buf = 0;
    for (int tile = sp; tile < p.n_tiles; tile += p.S, buf ^= 1) {
        __syncthreads();                                // previous tile's fragment reads are done
#pragma unroll
        for (int it = 0; it < GSL; ++it)
            if (g_sr[it] != -1) {
                const int i = tid + it * 256;
                Ops::put(gzt + (size_t)(i / QV) * WB_REC, i % QV, gv[it]);
            }
#pragma unroll
        for (int it = 0; it < XSL; ++it)
            if (x_sr[it] != -1) {
                const int i = tid + it * 256;
                Ops::put(xt + (size_t)(i / QV) * WB_REC, i % QV, xv[it]);
            }
        fill_segtab(tile + p.S, buf ^ 1);
        __syncthreads();
        if (tile + p.S < p.n_tiles) issue_loads(buf ^ 1);   // in flight during this tile's matrix work
        // ---- contract: 16 pixels per MFMA, one accumulator per tap.  Nothing but this wave hides its own LDS latency:
        //      fragments travel AH taps ahead of their MFMAs through NS register slots (TG is a multiple of NS, so the
        //      slot pattern repeats every step); the next step's dY fragments are requested with its first tap ----
        constexpr int NS = (TG % 3 == 0) ? 3 : 2, AH = NS - 1;
        static_assert(TG % NS == 0, "slot pattern must repeat per step");
        auto tap_off = [&](int t) { return ((t / KW) * p.cols_in + (t % KW)) * WB_REC; };
        auto step_ptrs = [&](int s, const char *&g0, const char *&g1, const char *&x0, const char *&x1) {
            const int pp0 = s + 8 * lhi + piece_pix, pp1 = pp0 + 4;
            g0 = gzt + (size_t)pp0 * WB_REC + a_col;
            g1 = gzt + (size_t)pp1 * WB_REC + a_col;
            x0 = xt + pixtab[pp0] + b_col;
            x1 = xt + pixtab[pp1] + b_col;
        };
        const char *g0, *g1, *x0, *x1;
        step_ptrs(0, g0, g1, x0, x1);
        WgradFrag<Ops> a = frag_tr<Ops>(g0, g1);
        WgradFrag<Ops> bf[NS];
#pragma unroll
        for (int t = 0; t < AH; ++t) bf[t] = frag_tr<Ops>(x0 + tap_off(t), x1 + tap_off(t));
        for (int s = 0; s < p.P; s += 16) {
            const char *ng0, *ng1, *nx0, *nx1;
            step_ptrs(s + 16 < p.P ? s + 16 : s, ng0, ng1, nx0, nx1);      // last step: harmless re-reads of this one
            WgradFrag<Ops> na = a;
#pragma unroll
            for (int t = 0; t < TG; ++t) {
                const int ahead = t + AH, slot = ahead % NS;
                if (ahead < TG) {
                    bf[slot] = frag_tr<Ops>(x0 + tap_off(ahead), x1 + tap_off(ahead));
                } else {
                    if (ahead == TG) na = frag_tr<Ops>(ng0, ng1);
                    bf[slot] = frag_tr<Ops>(nx0 + tap_off(ahead - TG), nx1 + tap_off(ahead - TG));
                }
                __builtin_amdgcn_sched_barrier(0);
                acc[t] = Ops::mma(a.part, bf[t % NS].part, acc[t]);
                __builtin_amdgcn_sched_barrier(0);
            }
            a = na;
            x0 = nx0;
            x1 = nx1;
        }
    }

    // ---- partial[sp][tap][co][ci] ----
    const int co0 = cot * WB_C + co_sub * 32, ci0 = cit * WB_C + ci_sub * 32;
#pragma unroll
    for (int t = 0; t < TG; ++t) {
        const int tap = GROUP ? (p.k0 + p.IS * (t / KW)) * p.KS + (t % KW) : t;
        float *dst = p.partial + (((size_t)sp * p.KS * p.KS + tap) * p.Cout) * p.Cin;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
            dst[(size_t)co * p.Cin + ci0 + l31] = acc[t][r];
        }
    }
}

struct WgradPlan {
    WgradK k;                    // 5x5: the geometry of the three-row group; launch_wgrad() derives the other
    bool big;                    // 3x3: the GSL3_BIG / XSL3_BIG instantiation
    int grid;
    size_t lds_bytes;
    long long partial_floats;
};

template <class Ops>
static int plan_wgrad(WgradPlan &pl, const ds_conv_shape *s) {
    DS_REQUIRE(s != nullptr, DS_ERR_NULL);
    DS_REQUIRE(s->B > 0 && s->H > 0 && s->W > 0, DS_ERR_BAD_SHAPE);
    DS_REQUIRE(s->KS == 3 || s->KS == 5, DS_ERR_UNSUPPORTED);
    DS_REQUIRE(s->stride == 1 || s->stride == 2, DS_ERR_UNSUPPORTED);
    DS_REQUIRE(s->Cin % WB_C == 0 && s->Cout % WB_C == 0, DS_ERR_BAD_SHAPE);
    WgradK &k = pl.k;
    const int pad = s->KS / 2;
    k.H = s->H; k.W = s->W; k.Cin = s->Cin; k.Cout = s->Cout;
    k.Ho = (s->H + 2 * pad - s->KS) / s->stride + 1;
    k.Wo = (s->W + 2 * pad - s->KS) / s->stride + 1;
    DS_REQUIRE(k.Ho > 0 && k.Wo > 0 && k.Wo <= 64, DS_ERR_BAD_SHAPE);
    DS_REQUIRE((long long)s->B * s->H * s->W * s->Cin < (1ll << 30), DS_ERR_BAD_SHAPE);      // 32-bit byte offsets
    DS_REQUIRE((long long)s->B * k.Ho * k.Wo * s->Cout < (1ll << 30), DS_ERR_BAD_SHAPE);
    k.x_bytes = (unsigned)((long long)s->B * s->H * s->W * s->Cin * Ops::ELEM);
    k.gz_bytes = (unsigned)((long long)s->B * k.Ho * k.Wo * s->Cout * Ops::ELEM);
    k.KS = s->KS; k.IS = s->stride; k.pad = pad;
    k.k0 = 0;
    const int group_rows = 3;                             // kernel rows of the (larger) 5x5 group
    // segment height / segments per tile: the kernel's staging slots bound the tile (256 / QV pixels per slot): at most
    // GSL slots of output pixels and XSL slots, less two pixels, of halo pixels
    constexpr int SLOT_PIX = 256 / Ops::QV;
    int max_out_pix = 0, max_in_pix = 0, best_rt = 0, best_ni = 1;
    // rows per segment: the most pixels per tile among the heights that waste the fewest rows in an image's last segment
    auto search = [&](int gsl, int xsl) {
        max_out_pix = gsl * SLOT_PIX; max_in_pix = xsl * SLOT_PIX - 2;
        best_rt = 0; best_ni = 1;
        double best_fill = -1.0;
        for (int rt = 1; rt <= k.Ho; ++rt) {
            if (rt * k.Wo > max_out_pix) break;
            const int rows_in = s->KS == 5 ? rt + group_rows - 1 : s->stride * (rt - 1) + s->KS;
            const int cols_in = s->stride * (k.Wo - 1) + s->KS;
            if (rows_in * cols_in > max_in_pix) break;
            const int segs = ds_ceil_div(k.Ho, rt);
            const int padded = (rt * k.Wo + 15) & ~15;
            const double fill = (double)k.Ho * k.Wo / ((double)segs * padded) + 1e-6 * rt;
            if (s->KS == 5 || fill > best_fill) { best_fill = fill; best_rt = rt; }
        }
        if (best_rt == 0) return 0;
        const int segs_per_img = ds_ceil_div(k.Ho, best_rt);
        const int rows_in = s->KS == 5 ? best_rt + group_rows - 1 : s->stride * (best_rt - 1) + s->KS;
        const int seg_pix = rows_in * (s->stride * (k.Wo - 1) + s->KS);
        while ((best_ni + 1) * best_rt * k.Wo <= max_out_pix && (best_ni + 1) * seg_pix <= max_in_pix &&
               best_ni + 1 <= s->B * segs_per_img)
            ++best_ni;
        return best_ni * best_rt * k.Wo;                  // output pixels per tile
    };
    pl.big = false;
    if (s->KS == 3) {
        const int px_big = search(Ops::GSL3_BIG, Ops::XSL3_BIG);
        const int px = search(Ops::GSL3, Ops::XSL3);
        if (Ops::GSL3 < Ops::GSL3_BIG && 2 * px_big >= 3 * px) {       // worth the larger tile only if it is much larger
            search(Ops::GSL3_BIG, Ops::XSL3_BIG);
            pl.big = true;
        }
    } else {
        search(Ops::GSL5, Ops::XSL5);
    }
    DS_REQUIRE(best_rt > 0, DS_ERR_UNSUPPORTED);
    k.RT = best_rt;
    k.segs_per_img = ds_ceil_div(k.Ho, best_rt);
    k.n_segs = s->B * k.segs_per_img;
    k.rows_in = s->KS == 5 ? best_rt + group_rows - 1 : s->stride * (best_rt - 1) + s->KS;   // 5x5: the rows of one residue
    k.cols_in = s->stride * (k.Wo - 1) + s->KS;
    k.seg_pix = k.rows_in * k.cols_in;
    k.NI = best_ni;
    k.P = (best_ni * best_rt * k.Wo + 15) & ~15;
    k.n_tiles = ds_ceil_div(k.n_segs, best_ni);
    k.n_co_tiles = s->Cout / WB_C;
    k.n_ci_tiles = s->Cin / WB_C;
    const int base_blocks = k.n_co_tiles * k.n_ci_tiles;
    int S = ds_ceil_div(ds_cu_count(), base_blocks);      // one workgroup per CU, every one with the same share of the tiles
    if (S > k.n_tiles) S = k.n_tiles;
    if (S < 1) S = 1;
    k.S = S;
    pl.grid = base_blocks * S;
    pl.lds_bytes = ((size_t)k.P + (size_t)k.NI * k.seg_pix) * Ops::REC + ((size_t)k.P + 8 * k.NI) * 4;
    DS_REQUIRE(k.P <= max_out_pix && k.NI * k.seg_pix <= max_in_pix + 2 && k.NI <= 255 &&
                   s->stride * k.rows_in + s->KS < 4096 && pl.lds_bytes <= 150 * 1024, DS_ERR_UNSUPPORTED);
    pl.partial_floats = (long long)S * s->KS * s->KS * s->Cout * s->Cin;
    return DS_OK;
}

// gw_oihw = out_scale * sum over pixels of gy (x) x; workspace: plan_wgrad()'s partial_floats floats
template <class Ops>
static int launch_wgrad(const ds_conv_shape *s, const void *x, const void *gy, float *workspace, float *gw_oihw,
                        float out_scale, void *stream) {
    WgradPlan pl;
    int rc = plan_wgrad<Ops>(pl, s);
    if (rc != DS_OK) return rc;
    pl.k.x = x; pl.k.gz = gy; pl.k.partial = workspace;
    if (s->KS == 3) {
        if (pl.big)
            DS_LAUNCH_BIG_LDS((wgrad_mfma_tr16_kernel<Ops, 9, 3, Ops::GSL3_BIG, Ops::XSL3_BIG>), pl.grid, 256, pl.lds_bytes, stream, pl.k);
        else
            DS_LAUNCH_BIG_LDS((wgrad_mfma_tr16_kernel<Ops, 9, 3, Ops::GSL3, Ops::XSL3>), pl.grid, 256, pl.lds_bytes, stream, pl.k);
    } else {
        // kernel rows 0, s, 2s (15 taps), then the remaining two (10 taps): same tiles, same splits, disjoint taps
        DS_LAUNCH_BIG_LDS((wgrad_mfma_tr16_kernel<Ops, 15, 5, Ops::GSL5, Ops::XSL5>), pl.grid, 256, pl.lds_bytes, stream, pl.k);
        rc = ds_last_launch_error();
        if (rc) return rc;
        WgradK k2 = pl.k;
        k2.k0 = s->stride == 2 ? 1 : 3;
        k2.rows_in = pl.k.RT + 1;
        k2.seg_pix = k2.rows_in * k2.cols_in;
        DS_LAUNCH_BIG_LDS((wgrad_mfma_tr16_kernel<Ops, 10, 5, Ops::GSL5, Ops::XSL5>), pl.grid, 256, pl.lds_bytes, stream, k2);
    }
    rc = ds_last_launch_error();
    if (rc) return rc;
    const long long n = (long long)s->KS * s->KS * s->Cout * s->Cin;
    int lg, rgrid;
    wgrad_reduce_shape(n, pl.k.S, lg, rgrid);
    DS_LAUNCH(wgrad_reduce_kernel, rgrid, 256, 1024, stream, (const float *)workspace, gw_oihw,
              pl.k.S, s->KS * s->KS, s->Cout, s->Cin, 0, out_scale, lg);
    return ds_last_launch_error();
}

}  // namespace
