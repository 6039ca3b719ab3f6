"""What the f32 and the bf16 convolution planners give for a table of shapes, member counts and forced tile
configurations: the rows of tests/golden/conv_plans_f32_bf16.json.  The file was recorded ONCE, on the host emulator, with
the library of the commit before the three planners' shared parts moved to csrc/conv_plan.h
(`python tests/conv_plan_cases.py LIBRARY OUT`); the tests replay the rows (test_emul_conv_plans.py on the emulator,
test_gpu_conv_plans.py on the device library) and never regenerate them.  Neither planner reads the number of compute
units, so one file serves both.

A row is one call, integers only; "s" = [B, Cin, Cout, H, W, KS, stride] or null (a null shape pointer):
  {"k": "f32",  "s", "rc": ds_conv_plan_describe, "o8": its out8 (rc == 0), "rows": ds_conv_stats_rows}
  {"k": "bf16", "s", "x3", "cfg": forced configuration or -1, "rc": ds_conv_bf16_plan_describe, "o8",
                "rows": ds_conv_bf16_stats_rows}
  {"k": "g3",   "s", "G", "rows": ds_conv_dgrad_bnbwd_bf16_rows}        (negative: an error code)
  {"k": "g5",   "s", "G", "rows": ds_conv_dgrad_s2_bnbwd_bf16_rows}"""
import ctypes
import json
import os

from conv_cases import BF16_CASES, CASES, DGRAD_BF16_CASES, DGRAD_CASES
from f16_plan_cases import BATCHES, LAYERS

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plans_f32_bf16.json")

N_BF16_CFG = 9
# odd-sized maps whose four stride-2 parity classes differ in size; one with H = 1 (the odd-row classes are empty)
# (the first two of each kind are accepted with three members, the others have tiles that straddle them)
ODD_MAPS = [(3, 64, 64, 9, 31, 5, 2), (24, 64, 64, 1, 32, 5, 2), (3, 64, 64, 13, 7, 5, 2), (6, 64, 128, 1, 4, 5, 2),
            (3, 128, 64, 9, 15, 5, 2), (6, 64, 64, 5, 3, 5, 2),
            (3, 64, 64, 9, 31, 3, 1), (24, 64, 64, 1, 32, 3, 1), (3, 64, 64, 13, 7, 3, 1), (6, 128, 64, 1, 4, 3, 1),
            (3, 64, 128, 9, 15, 3, 1)]
# one shape per check of the two planners, in the order the checks are made (None: the null shape pointer)
BAD = [
    None,
    (0, 16, 64, 8, 8, 3, 1),                # B <= 0
    (1, 16, 64, 8, 8, 7, 1),                # KS = 7
    (1, 16, 64, 8, 8, 1, 1),                # 1x1: the f32 kernel only
    (1, 16, 64, 8, 8, 3, 3),                # stride 3
    (1, 12, 64, 8, 8, 3, 1),                # Cin % 8
    (1, 8, 64, 8, 8, 3, 1),                 # Cin % 16: bf16 only
    (1, 16, 96, 8, 8, 3, 1),                # Cout % 64
    (1, 16, 64, 4, 129, 3, 1),              # Wo > 128
    (4096, 64, 64, 128, 64, 3, 1),          # B * H * W * Cin = 2^31
    (1 << 24, 16, 64, 1, 1, 3, 1),          # B * Ho = 2^24 (bf16: reciprocal index arithmetic)
    (4096, 8, 512, 32, 32, 3, 1),           # B * Ho * Wo * Cout = 2^31 (the f32 forward's own bound)
    (4096, 64, 64, 128, 32, 3, 1),          # B * Ho * Wo * Cout = 2^30 (32-bit byte offsets)
    (1, 16, 64, 8, 256, 5, 2),              # no tile configuration holds one 259-column row block
]
# member counts the fused entry points refuse: none, not a divisor of B; and the wrong kind of layer for each
BAD_G = [("g3", (6, 64, 64, 8, 8, 3, 1), 0), ("g3", (6, 64, 64, 8, 8, 3, 1), 4), ("g3", (6, 64, 64, 8, 8, 5, 2), 3),
         ("g5", (6, 64, 64, 8, 8, 5, 2), 0), ("g5", (6, 64, 64, 8, 8, 5, 2), 4), ("g5", (6, 64, 64, 8, 8, 3, 1), 3),
         ("g3", None, 1), ("g5", None, 1)]


def layer_shapes(batch):
    """the seven layers and, for each 5x5 stride-2 layer, the shape one parity class of its data gradient plans:
    a 3x3 stride-1 convolution over the output-gradient grid with the channels exchanged"""
    out = [(batch, ci, co, h, w, ks, st) for h, w, ci, co, ks, st in LAYERS]
    out += [(batch, co, ci, h // 2, w // 2, 3, 1) for h, w, ci, co, ks, st in LAYERS if ks == 5]
    return out


def keys():
    """(kind, shape, x3 or G, forced cfg) of every row, in file order"""
    shapes = [s for b in BATCHES for s in layer_shapes(b)]
    shapes += list(dict.fromkeys(CASES + BF16_CASES + DGRAD_CASES + DGRAD_BF16_CASES + ODD_MAPS))
    ks = []
    for s in shapes:
        ks.append(("f32", s, 0, -1))
        ks.append(("bf16", s, 0, -1))
        ks.append(("bf16", s, 1, -1))
        if s[5:] in ((3, 1), (5, 2)):
            for g in (1, 3):
                ks.append(("g3" if s[5] == 3 else "g5", s, g, -1))
    for s in layer_shapes(768):
        for cfg in range(N_BF16_CFG):
            for x3 in (0, 1):
                ks.append(("bf16", s, x3, cfg))
    for s in BAD:
        ks.append(("f32", s, 0, -1))
        ks.append(("bf16", s, 0, -1))
        ks.append(("bf16", s, 1, -1))
    for kind, s, g in BAD_G:
        ks.append((kind, s, g, -1))
    return ks


def resolve_rows(lib, only=None):
    """the rows the library `lib` (a NativeLib) gives now; the forced-configuration hook is back at its default afterwards"""
    from deepspeaker_pytorch_amd._native import ConvShape
    force = lib.raw("ds_conv_bf16_set_forced_cfg")
    rows = []
    try:
        for kind, s, a, cfg in (keys() if only is None else only):
            force(cfg)
            shp = None
            if s is not None:
                b, ci, co, h, w, k, st = s
                shp = ctypes.byref(ConvShape(b, h, w, ci, co, k, st))
            row = {"k": kind, "s": None if s is None else list(s)}
            out8 = (ctypes.c_int * 8)()
            if kind == "f32":
                rc = lib.raw("ds_conv_plan_describe")(shp, out8)
                row.update(rc=rc, o8=list(out8) if rc == 0 else [], rows=lib.raw("ds_conv_stats_rows")(shp))
            elif kind == "bf16":
                rc = lib.raw("ds_conv_bf16_plan_describe")(shp, a, out8)
                row.update(x3=a, cfg=cfg, rc=rc, o8=list(out8) if rc == 0 else [],
                           rows=lib.raw("ds_conv_bf16_stats_rows")(shp, a))
            else:
                name = "ds_conv_dgrad_bnbwd_bf16_rows" if kind == "g3" else "ds_conv_dgrad_s2_bnbwd_bf16_rows"
                row.update(G=a, rows=lib.raw(name)(shp, a))
            rows.append(row)
    finally:
        force(-1)
    return rows


def row_key(r):
    s = None if r["s"] is None else tuple(r["s"])
    return (r["k"], s, r.get("x3", r.get("G", 0)), r.get("cfg", -1))


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def dump_fixture(rows, path=FIXTURE):
    """one row per line: a changed plan reads as a one-line diff"""
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from deepspeaker_pytorch_amd._native import NativeLib
    dump_fixture(resolve_rows(NativeLib(sys.argv[1], host_memory=True)), sys.argv[2])
