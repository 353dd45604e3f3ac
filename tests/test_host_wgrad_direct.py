"""The planner of the direct small-kernel weight gradient (``fc_wgrad_direct_geometry``, csrc/host_wgrad.cpp) on the table
tests/test_gpu_wgrad_direct.py runs: covered or refused as listed, and the words the launch is sized by.  No GPU."""
import math

import pytest

from fft_conv_pytorch_amd import _native
from tests import accuracy_util as au
from tests.route_util import Case

CUS = 256
KNOBS = ("FFTCONV_WGRAD_DIRECT", "FFTCONV_WGRAD_DIRECT_SLICES")
FIRST = Case(2, 8, 8, (9, 10, 19), (3, 3, 3), p=1)
# (case, fc_dtype code of x and dY)
COVERED = [
    (FIRST, 0),
    (Case(3, 6, 10, (21, 37), (3, 5), s=(2, 1), d=(1, 2), p=(2, 3), g=2), 0),
    (Case(2, 5, 5, (23, 17), (7, 7), p=3, g=5, note="depthwise"), 0),
    (Case(2, 3, 20, (12, 13), (3, 3), p=1, note="two-out-blocks"), 0),
    (Case(1, 2, 2, (7, 8, 9), (5, 5, 5), p=2, note="125-taps"), 0),
    (Case(1, 2, 2, (4, 10, 11), (2, 8, 8), p=(1, 3, 3), note="128-taps"), 0),
    (Case(2, 3, 4, (11, 13), (3, 3), p=2, mode="reflect"), 0),
    (Case(2, 3, 4, (11, 13), (3, 3), p=2, mode="replicate"), 0),
    (Case(2, 3, 4, (11, 13), (3, 3), p=2, mode="circular"), 0),
    (FIRST, 3),
    (FIRST, 2),
]
TAPS_147 = Case(1, 2, 2, (4, 10, 11), (3, 7, 7), p=(1, 3, 3), note="147-taps")
REFUSED = [(TAPS_147, 0, "128 taps"), (FIRST, 1, "float64"), (Case(2, 2, 2, (9, 9), (3, 3), p=1), 4, "complex64"),
           (Case(2, 2, 2, (40,), (3,), p=1), 0, "1-D")]


def desc_of(c, dtype=0):
    return _native.conv_desc(c.nd, c.B, c.cin, c.cout, c.g, c.size, c.k, c.tup(c.s), c.tup(c.p), c.tup(c.d),
                             _native.PAD_MODES[c.mode], dtype)


def units_of(c, geom):
    return c.B * math.prod(-(-o // geom[f"tile{i}"]) for i, o in enumerate(au.out_spatial(c)))


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("c,dtype", COVERED, ids=lambda v: v.ident() if isinstance(v, Case) else f"dt{v}")
@pytest.mark.parametrize("forced", [None, 1, 3, 10 ** 6])
def test_geometry_of_a_covered_layer(c, dtype, forced, monkeypatch):
    if forced is not None:
        monkeypatch.setenv("FFTCONV_WGRAD_DIRECT_SLICES", str(forced))
    geom = _native.wgrad_direct_geometry(desc_of(c, dtype), CUS)
    units = units_of(c, geom)
    assert all(1 <= geom[f"tile{i}"] <= o for i, o in enumerate(au.out_spatial(c))) and (c.nd == 3 or geom["tile2"] == 0)
    assert 1 <= geom["out_block"] <= 16 and 1 <= geom["in_block"] <= c.cin // c.g
    assert geom["in_block"] * math.prod(c.k) <= 512
    assert 0 < geom["lds_bytes"] <= 160 * 1024
    assert 1 <= geom["slices"] <= units
    if forced is not None:
        assert geom["slices"] == min(forced, units)
    assert geom["workspace_bytes"] == geom["slices"] * c.cout * (c.cin // c.g) * math.prod(c.k) * 4


def test_slices_follow_the_cu_count():
    big = Case(8, 8, 8, (64, 64, 64), (3, 3, 3), p=1)
    few, many = (_native.wgrad_direct_geometry(desc_of(big), cus)["slices"] for cus in (8, 256))
    assert few < many


@pytest.mark.parametrize("c,dtype,words", REFUSED, ids=lambda v: v.ident() if isinstance(v, Case) else None)
def test_refused_layers_say_why(c, dtype, words):
    with pytest.raises(NotImplementedError, match=words):
        _native.wgrad_direct_geometry(desc_of(c, dtype), CUS)


def test_a_halo_past_the_lds_budget_is_refused():
    # one output position of one input channel reaches (4 * 120 + 1)^2 samples = 925 KB through a dilation of 120
    with pytest.raises(NotImplementedError, match="LDS"):
        _native.wgrad_direct_geometry(desc_of(Case(1, 1, 1, (600, 600), (5, 5), d=120)), CUS)
