// conv_mfma_f16_parts.h -- the tile-invariant parts the three hand-scheduled fp16 convolution kernels have in common:
// conv_mfma_f16_kernel.h (one tile per workgroup), conv_mfma_f16_pkernel.h (persistent) and conv_block_f16.hip (a whole
// BasicBlock).  The tests assert persistent = one-tile = 64-wide and block = two calls BITWISE; that rests on these
// pieces -- which pixel a lane owns, where its fragment lies, which filter slab a unit reads, how an accumulator tile is
// turned around -- being the same in all of them.  The split-operand bf16 kernel takes the lane permutation.
//
// A piece is called from a kernel only where the kernel's gfx950 instruction text stays what it was with the piece
// written out (compared kernel by kernel when this header was made: DESIGN_LOG.md, "One plan resolution ...").  These
// are schedules tuned against a full register file, and a forced-inline call is inlined before the optimiser has seen
// the caller: in some kernels that alone reorders the prologue's address arithmetic, moves the register allocation of
// the whole stream and, in the 5x5 persistent kernels with 16 items, grows the scratch frame.  So:
//   ds_mfma_lpix       one-tile, block, bf16 kernels; WRITTEN OUT in the persistent kernel
//   ds_f16_frag_pixel  one-tile kernel and the planner (frag_read_cost); WRITTEN OUT in the persistent kernel
//   ds_f16_lane_w, ds_f16_w_unit, ds_f16_epi, clip bounds   all three kernels
//   ds_f16_put_tile    persistent and block kernels; WRITTEN OUT in the one-tile kernel
// A written-out copy carries a comment that names the function it restates.  What is NOT here is what differs on
// purpose -- the run_chunk unit loops, the epilogue arithmetic, the persistent loops, the staging descriptors (with the
// stride-2 column slots and the tap offsets, which moved the instruction text of both kernels) -- and what the block
// kernel does its own way (compile-time pitch, no stride 2).
#pragma once
#include <ds_device.h>
#include "ds_common.h"

// Which pixel of its 32-pixel sub-tile a lane owns is free (the epilogue un-permutes): it is chosen so that the two
// 16-lane SERVICE GROUPS of a ds_read_b128 -- lanes {0-3,12-15,20-27} and {4-11,16-19,28-31} -- each read 16 CONSECUTIVE
// pixels, i.e. consecutive 80- (48-) byte records that walk all 64 banks.
__device__ __forceinline__ int ds_mfma_lpix(int l31) {
    return (l31 < 4 || l31 >= 28) ? l31 : (l31 < 12) ? l31 + 12 : (l31 < 16) ? l31 - 8 : (l31 < 20) ? l31 + 8 : l31 - 12;
}

// ---- pixel fragments ----
// A pixel m past the tile's last segment reads what the first pixel of its 16-pixel service group reads -- the same
// address is served in the same LDS cycle -- or record 0 if that one is past the end as well.  ONE definition for the
// kernels' a_off and for the planner's bank-conflict model (frag_read_cost in conv_mfma_f16.hip).
__host__ __device__ __forceinline__ int ds_f16_frag_pixel(int m, int tile_pixels) { return m >= tile_pixels ? (m & ~15) : m; }

// ---- filter fragments: bank [K/16][tap][Cout][16] ----
// this lane's offset (in halfs) inside a [Cout][16] slab: output channel n_base + l31, k-slots 8 lhi ..
__device__ __forceinline__ size_t ds_f16_lane_w(int n_base, int l31, int lhi) { return (size_t)(n_base + l31) * 16 + 8 * lhi; }
// Unit u of a chunk of KPT k-steps = (k-step u / NT, tap u % NT): filter slab KPT * chunk + u / NT, tap u % NT.
// K-step-major, so that a pixel's products are accumulated in the same order with 16- and 32-channel chunks (results do
// not depend on which the planner picks for a batch size).  kc_stride = NT * Cout * 16 (one 16-channel slab),
// tap_stride = Cout * 16.
template <int NT, int KPT>
__device__ __forceinline__ const _Float16 *ds_f16_w_unit(const _Float16 *w, size_t lane_w, size_t kc_stride, size_t tap_stride,
                                                         int chunk, int u) {
    return w + lane_w + (size_t)(KPT * chunk + (u / NT)) * kc_stride + (size_t)(u % NT) * tap_stride;
}

// ---- epilogue ----
// The filters were the A operand of every MFMA, so the accumulators hold the TRANSPOSED product: a lane owns one output
// pixel (lpix of the 32-pixel sub-tile) and, per register quad g, four consecutive output channels 8g + 4*lhi .. +3.  A
// step of NS sub-tiles (32 pixels x NS*32 channels) is turned around through a wave-private LDS buffer so that residual
// loads and stores move whole pixel rows: the NS*32 channels of a pixel are contiguous across NS*4 lanes, 8 channels =
// 16 bytes of fp16 per lane.
template <int NS>
struct ds_f16_epi {
    static constexpr int TP = NS * 32 + 4;      // buffer row pitch in floats (conflict-free 16-byte writes)
    static constexpr int LPP = NS * 4;          // lanes per pixel row
    static constexpr int PPI = 64 / LPP;        // pixel rows per instruction
    static constexpr int NRI = 32 / PPI;        // instructions per sub-tile
};
// accumulators acc[0 .. NS) of one sub-tile row -> the turn-around buffer dst
template <int NS>
__device__ __forceinline__ void ds_f16_put_tile(float *dst, const f32x16 *acc, int lpix, int lhi) {
#pragma unroll
    for (int ns = 0; ns < NS; ++ns)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = acc[ns][4 * g + j];
            *(f32x4 *)(dst + lpix * ds_f16_epi<NS>::TP + ns * 32 + 8 * g + 4 * lhi) = v;
        }
}
// the clipped ReLU of the reference (model.py:70-80); (-inf, +inf) without DS_EPI_CLIP: one v_med3 either way
constexpr float DS_F16_CLIP_LO = 0.0f, DS_F16_CLIP_HI = 20.0f;
__device__ __forceinline__ float ds_f16_clip_lo(int flags) { return (flags & DS_EPI_CLIP) ? DS_F16_CLIP_LO : -__builtin_inff(); }
__device__ __forceinline__ float ds_f16_clip_hi(int flags) { return (flags & DS_EPI_CLIP) ? DS_F16_CLIP_HI : __builtin_inff(); }
