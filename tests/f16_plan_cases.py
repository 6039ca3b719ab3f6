"""What the fp16 convolution's planner resolves for a table of shapes, flag sets and tuning hooks: the rows of
tests/golden/f16_conv_plans.json.  The file was recorded ONCE, on the host emulator, with the library of the commit before
the plan resolution was folded into one function (`python tests/f16_plan_cases.py LIBRARY OUT`); the tests replay the
rows (test_emul_f16_plans.py on the emulator, test_gpu_f16_plans.py on the device library) and never regenerate them.
None of the recorded values depends on the number of compute units, so one file serves both.

A row: {"s": [B, Cin, Cout, H, W, KS, stride], "f": flags, "cfg": forced configuration or -1, "pad": layout padding,
        "rc": return code of ds_conv_f16_plan_describe_hinted, "o8": its out8 (rc == 0),
        "lrc": return code of ds_conv_f16_plan_lds_layout, "o4": its out4 (lrc == 0),
        "ws": ds_conv_f16_splitk_workspace_bytes (negative: an error code)}"""
import ctypes
import json
import os

from f16_conv_cases import CASES, PERSIST_CASES

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f16_conv_plans.json")

# DS_CONV_HINT_SINGLE_BUFFER, _CHUNK16, _NO_PERSIST, _NO_WIDE, DS_CONV_IN_PLANES16 (include/deepspeaker_hip.h)
FLAG_SETS = (0, 64, 128, 1024, 2048, 512)
BATCHES = (1, 2, 7, 48, 96, 256, 768)
# the 3x3 and 5x5 layers of the 4-stage network at T = 160 (as tools/conv_probe.LAYERS): H, W, Cin, Cout, KS, stride
LAYERS = [
    (80, 32, 64, 64, 3, 1),
    (80, 32, 64, 128, 5, 2),
    (40, 16, 128, 128, 3, 1),
    (40, 16, 128, 256, 5, 2),
    (20, 8, 256, 256, 3, 1),
    (20, 8, 256, 512, 5, 2),
    (10, 4, 512, 512, 3, 1),
]
# shapes that must fail: Cin % 32, Wo > 128, KS = 7, B * Ho * Wo * Cout >= 2^30
BAD = [(1, 48, 64, 8, 8, 3, 1), (1, 32, 64, 4, 129, 3, 1), (1, 32, 64, 8, 8, 7, 1), (4096, 64, 64, 128, 32, 3, 1),
       (1, 32, 96, 8, 8, 3, 1), (1, 32, 64, 8, 8, 3, 3)]


def _layer_shapes(batch):
    out = []
    for h, w, ci, co, ks, st in LAYERS:
        out.append((batch, ci, co, h, w, ks, st))
    for h, w, ci, co, ks, st in LAYERS:
        if ks == 5:     # the data gradient of a 5x5 stride-2 layer: ONE 3x3 stride-1 convolution over the output-gradient
            out.append((batch, co, 4 * ci, h // 2, w // 2, 3, 1))      # grid, Cin' = Cout, Cout' = 4 Cin
    return out


def keys():
    """(shape, flags, forced cfg, layout padding) of every row, in file order"""
    ks = []
    shapes = list(CASES) + list(PERSIST_CASES) + [s for b in BATCHES for s in _layer_shapes(b)]
    for s in shapes:
        for f in FLAG_SETS:
            ks.append((s, f, -1, 0))
    for s in _layer_shapes(768):
        for pad in (0, 1):
            for cfg in range(-1, 7):
                if (cfg, pad) != (-1, 0):
                    ks.append((s, 0, cfg, pad))
    for s in BAD:
        ks.append((s, 0, -1, 0))
    return ks


def resolve_rows(lib, only=None):
    """the rows the library `lib` (a NativeLib) gives now; both tuning hooks are back at their defaults afterwards"""
    from deepspeaker_pytorch_amd._native import ConvShape
    describe, layout = lib.raw("ds_conv_f16_plan_describe_hinted"), lib.raw("ds_conv_f16_plan_lds_layout")
    ws_bytes = lib.raw("ds_conv_f16_splitk_workspace_bytes")
    rows = []
    try:
        for s, f, cfg, pad in (keys() if only is None else only):
            lib.raw("ds_conv_f16_set_forced_cfg")(cfg)
            lib.raw("ds_conv_f16_set_layout_padding")(pad)
            b, ci, co, h, w, k, st = s
            shp = ConvShape(b, h, w, ci, co, k, st)
            out8, out4 = (ctypes.c_int * 8)(), (ctypes.c_int * 4)()
            rc = describe(ctypes.byref(shp), f, out8)
            lrc = layout(ctypes.byref(shp), f, out4)
            rows.append({"s": list(s), "f": f, "cfg": cfg, "pad": pad, "rc": rc, "o8": list(out8) if rc == 0 else [],
                         "lrc": lrc, "o4": list(out4) if lrc == 0 else [], "ws": int(ws_bytes(ctypes.byref(shp)))})
    finally:
        lib.raw("ds_conv_f16_set_forced_cfg")(-1)
        lib.raw("ds_conv_f16_set_layout_padding")(0)
    return rows


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
