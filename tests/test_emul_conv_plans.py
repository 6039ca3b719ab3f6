"""The f32 and bf16 convolution planners on the host emulator against the committed record
(tests/golden/conv_plans_f32_bf16.json; see conv_plan_cases.py for what a row holds and how the file was made)."""
import ctypes

import pytest

from conv_plan_cases import BAD, BAD_G, keys, load_fixture, resolve_rows, row_key
from emul_util import emul_lib

# (pixels, channels, threads) of a tile -> resident workgroups per CU: the rows of kCfgB (conv_mfma_bf16_kernel.h) and
# (pixels, channels) -> the same of kCfg (conv_mfma_f32.hip)
BF16_TILES = {(128, 64, 256): 3, (160, 128, 256): 2, (256, 64, 256): 2, (160, 128, 128): 2, (160, 256, 256): 1,
              (320, 128, 256): 1, (320, 64, 128): 2, (128, 128, 128): 2, (128, 256, 256): 1}
F32_TILES = {(128, 64): 4, (160, 128): 2, (256, 64): 2}
CUS, SIMDS = 256, 1024


@pytest.fixture(scope="module")
def fixture_rows():
    return load_fixture()


def test_fixture_has_exactly_the_listed_rows(fixture_rows):
    assert [row_key(r) for r in fixture_rows] == keys()
    assert len(set(keys())) == len(keys()) > 700


def test_plans_are_the_recorded_ones(fixture_rows):
    got = resolve_rows(emul_lib())
    for g, want in zip(got, fixture_rows):
        assert g == want
    assert len(got) == len(fixture_rows)


def test_fixture_covers_what_it_is_for(fixture_rows):
    """every bf16 and f32 tile configuration (the bf16 ones forced, and all but one by the planner's own choice), both
    branches of the last-round occupancy for each planner, the bf16 wave penalty, a launch the fused entry point refuses because its tiles
    straddle members, and every error code"""
    f32 = [r for r in fixture_rows if r["k"] == "f32" and r["rc"] == 0]
    bf16 = [r for r in fixture_rows if r["k"] == "bf16" and r["rc"] == 0]
    assert {(r["o8"][0], r["o8"][1]) for r in f32} == set(F32_TILES)
    assert {(r["o8"][0], r["o8"][1], r["o8"][6]) for r in bf16 if r["cfg"] >= 0} == set(BF16_TILES)
    # the planner's own choices: every tile but 320 x 128, which wins no recorded shape (as tools/conv_bf16_ab.py found)
    assert {(r["o8"][0], r["o8"][1], r["o8"][6]) for r in bf16 if r["cfg"] < 0} == set(BF16_TILES) - {(320, 128, 256)}
    assert {r["x3"] for r in bf16} == {0, 1}
    # a grid inside one round of resident workgroups, and one that needs several
    one_round = {r["o8"][4] <= CUS * F32_TILES[(r["o8"][0], r["o8"][1])] for r in f32}
    assert one_round == {True, False}
    one_round = {r["o8"][4] <= CUS * BF16_TILES[(r["o8"][0], r["o8"][1], r["o8"][6])] for r in bf16}
    assert one_round == {True, False}
    # fewer waves than the chip has SIMDs: at a bench-size batch too, where another tile would have filled them
    assert any(r["o8"][4] * (r["o8"][6] // 64) < SIMDS and r["s"][0] >= 256 for r in bf16)
    assert any(r["o8"][4] * (r["o8"][6] // 64) >= SIMDS for r in bf16)
    # every recorded stats-row count is the plan's number of M tiles: grid / (Cout / channels per tile)
    for r in f32 + bf16:
        assert r["rows"] * (r["s"][2] // r["o8"][1]) == r["o8"][4]
    fused = {(r["k"], tuple(r["s"]), r["G"]): r["rows"] for r in fixture_rows if r["k"] in ("g3", "g5") and r["s"]}
    straddle = ("g3", (768, 512, 512, 10, 4, 3, 1))
    assert fused[straddle + (3,)] == -4 and fused[straddle + (1,)] > 0
    assert any(k[0] == "g5" and k[2] == 3 and v > 0 for k, v in fused.items())
    # four parity classes of different sizes; and a one-row map, whose empty classes leave the rows of the other two
    assert fused[("g5", (3, 64, 64, 9, 31, 5, 2), 3)] > 0 and fused[("g5", (24, 64, 64, 1, 32, 5, 2), 3)] > 0
    assert fused[("g5", (6, 64, 128, 1, 4, 5, 2), 3)] == -4 and fused[("g5", (6, 64, 128, 1, 4, 5, 2), 1)] > 0
    bad = [r for r in fixture_rows if r["k"] in ("f32", "bf16") and (r["s"] is None or tuple(r["s"]) in BAD)]
    assert len(bad) == 3 * len(BAD)
    assert all(r["rows"] == r["rc"] for r in bad if r["rc"] < 0)
    assert {r["rc"] for r in bad if r["k"] == "f32"} == {0, -1, -3, -4}      # OK (1x1, Cin = 8), BAD_SHAPE, NULL, UNSUPPORTED
    assert {r["rc"] for r in bad if r["k"] == "bf16"} == {-1, -3, -4}
    assert all(fused[(k, tuple(s), g)] == -4 for k, s, g in BAD_G if s is not None)
    assert [r["rows"] for r in fixture_rows if r["k"] in ("g3", "g5") and r["s"] is None] == [-3, -3]
    # bf16 without split operands has the three small tiles only: forcing another one leaves nothing to plan with
    assert all(r["rc"] == -4 for r in fixture_rows if r["k"] == "bf16" and r["x3"] == 0 and r["cfg"] >= 3)


def test_the_hook_is_restored_after_a_failure():
    lib = emul_lib()
    first = keys()[1]
    assert first[0] == "bf16"
    with pytest.raises(ctypes.ArgumentError):
        resolve_rows(lib, only=[("bf16", first[1], 1, 5), ("bf16", first[1], "not an int", -1)])
    assert resolve_rows(lib, only=[first]) == [load_fixture()[1]]
