"""The fp16 convolution's plan resolution on the host emulator against the committed record
(tests/golden/f16_conv_plans.json; see f16_plan_cases.py for what a row holds and how the file was made)."""
import ctypes

import pytest

from emul_util import emul_lib
from f16_plan_cases import BAD, FLAG_SETS, keys, load_fixture, resolve_rows


@pytest.fixture(scope="module")
def fixture_rows():
    return load_fixture()


def test_fixture_has_exactly_the_listed_rows(fixture_rows):
    assert [(tuple(r["s"]), r["f"], r["cfg"], r["pad"]) for r in fixture_rows] == keys()
    assert len({(tuple(r["s"]), r["f"], r["cfg"], r["pad"]) for r in fixture_rows}) > 600


def test_plans_are_the_recorded_ones(fixture_rows):
    got = resolve_rows(emul_lib())
    for g, want in zip(got, fixture_rows):
        assert g == want
    assert len(got) == len(fixture_rows)


def test_fixture_covers_what_it_is_for(fixture_rows):
    """every tile configuration, both chunk widths, both buffering modes, the persistent and the one-tile kernel, a
    split-K workspace, padded strides and every error the bad shapes are there for"""
    ok = [r for r in fixture_rows if r["rc"] == 0]
    assert {(r["o8"][0], r["o8"][1], r["o8"][6]) for r in ok} >= {(160, 128, 128), (160, 256, 256), (320, 128, 256),
                                                                 (320, 64, 128), (128, 128, 128), (128, 256, 256),
                                                                 (640, 64, 256), (128, 256, 128)}
    flavours = {r["o8"][7] // 100 for r in ok}          # persistent, double-buffered, 16-channel chunks
    assert flavours >= {110, 111, 10, 11, 0}
    assert any(r["ws"] > 0 for r in ok) and any(r["ws"] == 0 for r in ok)
    assert any(r["pad"] == 1 and r["o4"][1] % 16 == 0 and r["o4"][1] != r["o4"][0] * 80 for r in ok)
    assert sorted({r["f"] for r in fixture_rows}) == sorted(FLAG_SETS)
    bad = [r for r in fixture_rows if tuple(r["s"]) in BAD]
    assert len(bad) == len(BAD) and all(r["rc"] < 0 and r["lrc"] == r["rc"] and r["ws"] == r["rc"] for r in bad)
    assert {r["rc"] for r in bad} == {-1, -4}           # DS_ERR_BAD_SHAPE, DS_ERR_UNSUPPORTED


def test_the_hooks_are_restored_after_a_failure():
    lib = emul_lib()
    first = keys()[0]
    with pytest.raises(ctypes.ArgumentError):
        resolve_rows(lib, only=[(keys()[-1][0], 0, 3, 1), (first[0], "not an int", -1, 0)])
    assert resolve_rows(lib, only=[first]) == [load_fixture()[0]]
