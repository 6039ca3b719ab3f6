"""The convolution cases of the f32 and bf16 kernel tests, (B, Cin, Cout, H, W, KS, stride): the emulator tests
(test_emul_kernels.py), the device tests of the data gradients (test_gpu_conv_plans.py) and the recorded plans
(conv_plan_cases.py) read the same lists."""

CASES = [
    # (B, Cin, Cout, H, W, KS, stride)       what it exercises
    (2, 8, 64, 9, 32, 3, 1),                 # stage-1 geometry, partial last row block (9 = 2*4+1)
    (1, 16, 64, 8, 16, 3, 1),                # two channel chunks, 8-row segments
    (3, 8, 128, 20, 8, 3, 1),                # stage-3 geometry: whole image = 160 rows, 160x128 tile
    (5, 8, 128, 10, 4, 3, 1),                # stage-4 geometry: 4 images per tile, ragged last tile
    (2, 8, 64, 16, 32, 5, 2),                # 5x5 stride 2, even sizes
    (2, 8, 128, 13, 16, 5, 2),               # 5x5 stride 2, odd height (variable-length utterances)
    (3, 16, 128, 7, 8, 5, 2),                # 5x5 s2 into a 4x4 map, multi-image tiles
    (70, 24, 64, 1, 1, 1, 1),                # 1x1 on [B,1,1,C]: the fc GEMM shape class
]

BF16_CASES = [
    (2, 16, 64, 9, 32, 3, 1), (3, 32, 128, 20, 8, 3, 1), (5, 16, 128, 10, 4, 3, 1),
    (2, 16, 64, 16, 32, 5, 2), (2, 32, 128, 13, 16, 5, 2), (3, 16, 128, 7, 8, 5, 2),
]

# data gradients: stride 1 (flipped bank) and the four parity classes of stride 2 -- odd heights, and a one-row map
# whose odd-row classes are empty
DGRAD_CASES = [
    (2, 64, 8, 9, 32, 3, 1), (3, 128, 16, 20, 8, 3, 1),
    (2, 64, 8, 16, 32, 5, 2), (2, 64, 16, 13, 16, 5, 2), (3, 128, 8, 7, 8, 5, 2), (1, 64, 8, 1, 4, 5, 2),
]

DGRAD_BF16_CASES = [(2, 64, 64, 9, 32, 3, 1), (2, 64, 64, 16, 32, 5, 2), (2, 64, 16, 13, 16, 5, 2),
                    (3, 128, 64, 7, 8, 5, 2), (1, 64, 32, 1, 4, 5, 2)]
