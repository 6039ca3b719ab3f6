// wgrad_mfma_f16.hip -- filter gradients of the 3x3 / 5x5 convolution layers for the OPT-IN fp16 training step
// (train_f16.hip): fp16 activations and fp16 (loss-scaled) output gradients in HBM, ONE v_mfma_f32_32x32x16_f16 per
// product, f32 accumulation, f32 result un-scaled in the fixed-order fold.  Kernel, plan and launch: wgrad_mfma_tr16.h;
// here the operand format and the C entry points.
//
// What fp16 tensors change against the split-operand bf16 path (wgrad_mfma_bf16.hip): staging is a 16-byte copy (8
// channels, no conversion, no hi / lo halves), a pixel record is 128 B of data + 64 B of pad instead of 320 B, so tiles are
// twice as many pixels (256 for a 3x3) at the same LDS footprint, and a tap is one MFMA instead of three.
#include "wgrad_mfma_tr16.h"

namespace {

struct WgradOps_f16 {
    static constexpr int ELEM = 2;                       // fp16 tensors
    static constexpr int QV = WB_C / 8;                  // 16-byte items (8 halfs) per staged pixel
    static constexpr int REC = 2 * WB_C + 64;            // 64 halfs | pad -> 48 dwords: four consecutive records (and their second
                                                         // 16-channel block, 8 dwords on) start in eight different 8-dword bank groups
    static constexpr int PARTS = 1, PART_BYTES = 0;
    // 32 pixels per slot: a 3x3 tile is up to 256 output / 446 halo pixels (no big variant), a 5x5 kernel-row group 128 / 382
    static constexpr int GSL3 = 8, XSL3 = 14, GSL3_BIG = GSL3, XSL3_BIG = XSL3, GSL5 = 4, XSL5 = 12;
    typedef f16x8 vec;

    static __device__ __forceinline__ void put(char *rec, int q, const f32x4 v) { *(f32x4 *)(rec + q * 16) = v; }      // 8 channels, as they are
    static __device__ __forceinline__ vec join(const bf16x4 a, const bf16x4 b) {
        return __builtin_shufflevector(__builtin_bit_cast(f16x4, a), __builtin_bit_cast(f16x4, b), 0, 1, 2, 3, 4, 5, 6, 7);
    }
    static __device__ __forceinline__ f32x16 mma(const vec *a, const vec *b, f32x16 c) { return ds_mfma_32x32x16_f16(a[0], b[0], c); }
};

}  // namespace

extern "C" long long ds_conv_wgrad_f16_workspace_floats(const ds_conv_shape *s) {
    WgradPlan pl;
    int rc = plan_wgrad<WgradOps_f16>(pl, s);
    return rc == DS_OK ? pl.partial_floats : rc;
}

// gw_oihw = out_scale * sum over pixels of gy (x) x: x [B,H,W,Cin] fp16 activations, gy [B,Ho,Wo,Cout] fp16 output
// gradients in loss-scaled units (out_scale = 1 / S), workspace ds_conv_wgrad_f16_workspace_floats(s) floats.
extern "C" int ds_conv_wgrad_f16(const ds_conv_shape *s, const void *x_f16, const void *gy_f16, float *workspace,
                                 float *gw_oihw, float out_scale, void *stream) {
    DS_REQUIRE(s && x_f16 && gy_f16 && workspace && gw_oihw, DS_ERR_NULL);
    DS_REQUIRE(DS_ALIGNED16(x_f16) && DS_ALIGNED16(gy_f16), DS_ERR_ALIGNMENT);
    return launch_wgrad<WgradOps_f16>(s, x_f16, gy_f16, workspace, gw_oihw, out_scale, stream);
}
