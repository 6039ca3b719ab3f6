"""Shapes of the fp16 convolution tests, shared by the emulator files (test_emul_f16.py) and the device file
(test_gpu_f16_plans.py): (B, Cin, Cout, H, W, KS, stride)."""

CASES = [
    (2, 64, 64, 11, 32, 3, 1),               # stage-1 geometry, two chunks, ragged last row block
    (3, 32, 128, 20, 8, 3, 1),               # stage-3 geometry, one chunk, 160-pixel tile = one image
    (5, 96, 128, 10, 4, 3, 1),               # stage-4 geometry: several images per tile, three chunks, ragged tile
    (2, 64, 128, 21, 16, 5, 2),              # 5x5 stride 2, odd height, two chunks
    (3, 32, 256, 9, 8, 5, 2),                # 5x5 s2 into a 5x4 map, multi-image tiles
    (1, 64, 64, 3, 5, 3, 1),                 # tiny map: every tile row ragged
    (1, 64, 128, 21, 64, 5, 2),              # wide stride-2 input: too many staging items -> single-buffered tile
    (1, 32, 64, 12, 100, 3, 1),              # wide 3x3 map (variable-length / wide inputs), single chunk
    (2, 32, 128, 100, 4, 3, 1),              # several row blocks of one image per tile: mixed halo windows (table walk)
]

# Larger batches of the bench geometries: on the emulated device (2 "compute units" = 2-4 resident workgroups) every
# persistent workgroup walks many tiles -- top / middle / bottom row blocks, ragged last tiles, several n tiles.
PERSIST_CASES = [
    (3, 64, 64, 27, 32, 3, 1),               # row blocks of one image (linear item offsets), ragged last block
    (9, 32, 128, 20, 8, 3, 1),               # one image per tile
    (11, 64, 128, 10, 4, 3, 1),              # several whole images per tile (item tables), ragged last tile
    (3, 64, 128, 43, 16, 5, 2),              # 5x5 stride 2 row blocks, odd height
    (7, 32, 256, 9, 8, 5, 2),                # 5x5 stride 2, multi-image tiles, two n tiles
    (2, 32, 128, 100, 4, 3, 1),              # a tall narrow map: 32-row blocks
    (7, 64, 256, 10, 4, 3, 1),               # Cout % 256 == 0 on 10x4 maps: the 128 x 256 plan (cfg 7, NSUB = 4), ragged tile
    (8, 32, 512, 10, 4, 3, 1),               # ... two n tiles of 256, one chunk
]
