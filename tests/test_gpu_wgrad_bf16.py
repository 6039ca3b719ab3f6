"""The split-operand bf16 filter-gradient kernel (wgrad_mfma_bf16.hip, the default training path) on the device, through
the C ABI on device tensors, against the float64 reference of the same operation (train_f16_cases.wgrad_ref): every
instantiation -- the base and the big 3x3 tiles, both kernel-row-group launches of a 5x5 -- with one tile per image, several
images per tile, a part-empty last tile and an uneven share of the tiles per split.

Bar: max-norm relative error 3e-5 (16 mantissa bits per operand), the bar test_gpu_parity.py and test_emul_kernels.py hold
this kernel to.  Every call writes into a NaN-filled workspace and a NaN-filled output; two calls must agree bit for bit
(fixed-order fold).

The plan of every case on a 256-CU device (staging slots of 16 pixels: base 3x3 tiles up to 128 output / 222 halo pixels, big
160 / 270, a 5x5 group 64 / 190), derived from the plan arithmetic; the splits are those the host emulator plans when told
256 CUs and are asserted exactly on such a device."""
import ctypes

import pytest
import torch

import train_f16_cases as TC
from conftest import rel_err
from test_gpu_train_f16_kernels import dev, eng, full, host     # noqa: F401  (eng: the module-scoped engine fixture)

pytestmark = pytest.mark.gpu

# (b, ci, co, h, w, ks, stride, split class, S on a 256-CU device); the classes are train_f16_cases.check_split_class's
CASES = [
    # <9,3,8,14>: 3-row segments of 96 pixels, one per tile (two would pass 128), 6 tiles: S = 6, one tile per split
    (2, 64, 64, 9, 32, 3, 1, "tiles", 6),
    # <9,3,10,17>: a whole 160-pixel image per tile (base tiles would hold half an image: 80 pixels), 3 tiles: S = 3
    (3, 128, 64, 20, 8, 3, 1, "tiles", 3),
    # <9,3,10,17>, 16 co/ci tile pairs: S = 256 / 16 = 16 over 40 tiles -- eight splits own three tiles, eight own two
    (40, 256, 256, 20, 8, 3, 1, "cus", 16),
    # <9,3,8,14>: three 40-pixel images per tile (120 of 128 slots; the big tile holds no more), 5 images in 2 tiles -- the
    # last tile a third empty: S = 2
    (5, 64, 128, 10, 4, 3, 1, "tiles", 2),
    # <15,5,4,12> + <10,5,4,12>: output 7 x 8 (odd height), one image per tile (56 of 64 slots), 3 tiles: S = 3
    (3, 64, 128, 13, 16, 5, 2, "tiles", 3),
    # <15,5,4,12> + <10,5,4,12>: output 5 x 2, three images per tile (the 190 halo pixels bound it), 4 images in 2 tiles: S = 2
    (4, 128, 128, 10, 4, 5, 2, "tiles", 2),
]


@pytest.mark.parametrize("b,ci,co,h,w,ks,st,split_cls,s256", CASES)
def test_conv_wgrad_bf16(eng, b, ci, co, h, w, ks, st, split_cls, s256):
    from deepspeaker_pytorch_amd._native import ConvShape
    shp = ConvShape(b, h, w, ci, co, ks, st)
    n_ws = eng.lib.raw("ds_conv_wgrad_bf16_workspace_floats")(ctypes.byref(shp))
    assert n_ws > 0 and n_ws % (ks * ks * co * ci) == 0
    n_split = n_ws // (ks * ks * co * ci)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    TC.check_split_class(n_split, cus, ci, co, split_cls, s256)
    ho, wo = (h - 1) // st + 1, (w - 1) // st + 1
    gen = torch.Generator().manual_seed(b + ci + co + h + ks)
    x = torch.randn((b, h, w, ci), generator=gen)
    gy = torch.randn((b, ho, wo, co), generator=gen)
    x_d, g_d = dev(x), dev(gy)
    p = eng._p
    gws = []
    for _ in range(2):
        ws, gw = full((n_ws,), torch.float32), full((co, ci, ks, ks), torch.float32)
        eng.lib.call("ds_conv_wgrad_bf16", ctypes.byref(shp), p(x_d), p(g_d), p(ws), p(gw), eng._stream(x_d))
        gws.append(gw)
    torch.cuda.synchronize()
    ref = TC.wgrad_ref(x.permute(0, 3, 1, 2).numpy(), gy.permute(0, 3, 1, 2).numpy(), ks, st)
    err = rel_err(host(gws[0]), ref)                        # NaN anywhere: nan < 3e-5 is False
    print(f"wgrad bf16x3 b={b} {ci}->{co} {h}x{w} k{ks}s{st}: S={n_split} ({split_cls}, {cus} CUs), {b * ho * wo} pixels, "
          f"kernel {err:.2e} (bar 3e-5)")
    assert torch.equal(gws[0], gws[1])                      # fixed-order fold
    assert err < 3e-5, err
