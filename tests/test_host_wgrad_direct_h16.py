"""The planner of the 16-bit MFMA body of the direct weight gradient (FFTCONV_WGRAD_DIRECT_BODY=h16, csrc/host_wgrad.cpp):
which layers take it, and the geometry words of the table tests/test_gpu_wgrad_direct_h16.py runs.  No GPU."""
import math

import pytest

from fft_conv_pytorch_amd import _native
from tests import accuracy_util as au
from tests.route_util import Case
from tests.test_host_wgrad_direct import COVERED, CUS, FIRST, KNOBS, desc_of, units_of
from tests.test_host_wgrad_direct_dw import BODY, FIRST as DW_FIRST, ident

TRANSPOSED = Case(2, 4, 6, (7, 9), (3, 3), s=2, p=1, op=1, tr=True)
TWO_IN_BLOCKS = Case(1, 64, 4, (6, 9), (3, 3), p=1, note="two-in-blocks")      # 64 x 9 columns > the 512 of a workgroup
# each the smallest shape that reaches one way the kernel can go wrong
CASES = list({c.ident(): c for c, _ in COVERED if c.cin > c.g}.values()) + [
    Case(2, 4, 6, (9, 21), (3, 3), s=(1, 2), p=1, note="x-stride-2"),
    Case(2, 4, 4, (11, 29), (3, 3), s=(2, 3), d=(1, 2), p=2, note="x-stride-3-dilation-2"),
    Case(2, 3, 4, (8, 5), (3, 3), p=1, note="row-shorter-than-a-run"),
    TRANSPOSED, TWO_IN_BLOCKS]


def forward_of(c):
    """(the forward layer whose weight gradient a transposed layer's dW is: dY is its signal)"""
    return Case(c.B, c.cout, c.cin, au.out_spatial(c), c.k, s=c.s, p=c.p, d=c.d, g=c.g) if c.tr else c


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for k in KNOBS + (BODY,):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("c,dtype,knob,body", [(FIRST, 3, "h16", "h16"), (FIRST, 2, "h16", "h16"), (FIRST, 0, "h16", "mfma"),
                                               (DW_FIRST, 3, "h16", "valu"), (FIRST, 3, None, "mfma")], ids=ident)
def test_body_of_a_layer_under_the_knob(c, dtype, knob, body, monkeypatch):
    if knob:
        monkeypatch.setenv(BODY, knob)
    assert _native.wgrad_direct_body(desc_of(c, dtype), CUS) == body


@pytest.mark.parametrize("c", CASES, ids=ident)
@pytest.mark.parametrize("forced", [None, 1, 3, 10 ** 6])
def test_geometry_of_the_h16_body(c, forced, monkeypatch):
    monkeypatch.setenv(BODY, "h16")
    if forced is not None:
        monkeypatch.setenv("FFTCONV_WGRAD_DIRECT_SLICES", str(forced))
    c = forward_of(c)
    assert _native.wgrad_direct_body(desc_of(c, 3), CUS) == "h16"
    geom = _native.wgrad_direct_geometry(desc_of(c, 3), CUS)
    units = units_of(c, geom)
    assert all(1 <= geom[f"tile{i}"] <= o for i, o in enumerate(au.out_spatial(c))) and (c.nd == 3 or geom["tile2"] == 0)
    assert 1 <= geom["out_block"] <= 16 and 1 <= geom["in_block"] <= c.cin // c.g
    assert geom["in_block"] * math.prod(c.k) <= 512
    assert 0 < geom["lds_bytes"] <= 160 * 1024
    assert 1 <= geom["slices"] <= units
    if forced is not None:
        assert geom["slices"] == min(forced, units)
    assert geom["workspace_bytes"] == geom["slices"] * c.cout * (c.cin // c.g) * math.prod(c.k) * 4
