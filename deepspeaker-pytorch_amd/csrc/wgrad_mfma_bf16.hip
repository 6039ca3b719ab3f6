// wgrad_mfma_bf16.hip -- filter gradients of the 3x3 / 5x5 convolution layers on the bf16 matrix cores
// with split operands (bf16x3: x = hi + lo, product = hi*hi + hi*lo + lo*hi, f32 accumulate): f32 activations and f32
// output gradients in HBM.  Kernel, plan and launch: wgrad_mfma_tr16.h; here the operand format and the C entry points.
#include "wgrad_mfma_tr16.h"

// staging slots (16 pixels each) of the two 3x3 instantiations: 128-pixel tiles, and 160-pixel ones for geometries
// whose image (or a much larger part of it) then fits one tile -- measured per layer at 768 utterances
// (tools/wgrad_ab.py): 64-pixel tiles 610 / 506 / 463 / 587 us, 128: 540 / 431 / 461 / 422, 160: 564 / 446 / 410 / 442
#ifndef DS_WGRAD_GSL3
#define DS_WGRAD_GSL3 8
#define DS_WGRAD_XSL3 14
#endif

namespace {

struct WgradOps_bf16x3 {
    static constexpr int ELEM = 4;                       // f32 tensors
    static constexpr int QV = WB_C / 4;                  // float4 per staged pixel
    static constexpr int REC = 4 * WB_C + 64;            // hi (128) | lo (128) | pad -> 80 dwords = 16 mod 64
    static constexpr int PARTS = 2, PART_BYTES = 2 * WB_C;      // hi at +0, lo behind it
    // a 3x3 tile is up to 128 output / 222 halo pixels (110 KiB of records, one workgroup per CU), the big one 160 / 270,
    // a 5x5 kernel-row group 64 / 190
    static constexpr int GSL3 = DS_WGRAD_GSL3, XSL3 = DS_WGRAD_XSL3, GSL3_BIG = 10, XSL3_BIG = 17, GSL5 = 4, XSL5 = 12;
    typedef bf16x8 vec;

    static __device__ __forceinline__ void put(char *rec, int q, const f32x4 v) {      // 4 channels -> hi / lo halves of the record
        bf16x4 h, l;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            h[j] = (__bf16)v[j];
            l[j] = (__bf16)(v[j] - (float)h[j]);
        }
        *(bf16x4 *)(rec + q * 8) = h;
        *(bf16x4 *)(rec + PART_BYTES + q * 8) = l;
    }
    static __device__ __forceinline__ vec join(const bf16x4 a, const bf16x4 b) {
        return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    }
    static __device__ __forceinline__ f32x16 mma(const vec *a, const vec *b, f32x16 c) {      // part 0: hi, part 1: lo
        c = ds_mfma_32x32x16_bf16(a[1], b[0], c);
        c = ds_mfma_32x32x16_bf16(a[0], b[1], c);
        return ds_mfma_32x32x16_bf16(a[0], b[0], c);
    }
};

}  // namespace

extern "C" long long ds_conv_wgrad_bf16_workspace_floats(const ds_conv_shape *s) {
    WgradPlan pl;
    int rc = plan_wgrad<WgradOps_bf16x3>(pl, s);
    return rc == DS_OK ? pl.partial_floats : rc;
}

extern "C" int ds_conv_wgrad_bf16(const ds_conv_shape *s, const float *x, const float *gy, float *workspace,
                                  float *gw_oihw, void *stream) {
    DS_REQUIRE(s && x && gy && workspace && gw_oihw, DS_ERR_NULL);
    DS_REQUIRE(DS_ALIGNED16(x) && DS_ALIGNED16(gy), DS_ERR_ALIGNMENT);
    return launch_wgrad<WgradOps_bf16x3>(s, x, gy, workspace, gw_oihw, 1.0f, stream);
}
