"""The planner of the depthwise body of the direct weight gradient (``fc_wgrad_direct_body``, FFTCONV_WGRAD_DIRECT_BODY and
the geometry words of that body, csrc/host_wgrad.cpp), on the table tests/test_gpu_wgrad_direct_dw.py runs.  No GPU."""
import math

import pytest

from fft_conv_pytorch_amd import _native
from tests import accuracy_util as au
from tests.route_util import Case
from tests.test_host_wgrad_direct import CUS, KNOBS, desc_of, units_of

BODY = "FFTCONV_WGRAD_DIRECT_BODY"
M = 8       # the largest channel multiplier the automatic rule gives to the depthwise body
FIRST = Case(2, 5, 5, (23, 17), (7, 7), p=3, g=5, note="kxb8-ragged-edge")
# (case, fc_dtype code of x and dY, forced slices): each the smallest shape that reaches one way the kernel can go wrong
DEPTHWISE = [
    (FIRST, 0, None),
    (Case(2, 3, 6, (12, 13), (3, 3), p=1, g=3, note="multiplier-2"), 0, None),
    (Case(3, 4, 4, (21, 37), (3, 5), s=(2, 1), d=(1, 2), p=(2, 3), g=4, note="general-build"), 0, None),
    (Case(1, 2, 2, (7, 8, 9), (5, 5, 5), p=2, g=2, note="125-taps"), 0, None),
    (Case(1, 2, 2, (4, 10, 11), (2, 8, 8), p=(1, 3, 3), g=2, note="128-taps"), 0, None),
    (Case(2, 2, 2, (20, 9), (9, 1), p=(4, 0), g=2, note="kxb1"), 0, None),
    (Case(1, 2, 2, (6, 40), (3, 11), p=(1, 5), g=2, note="two-blocks-per-row"), 0, None),
    (Case(1, 1, 1, (5, 3), (3, 3), note="one-column"), 0, None),
    (Case(2, 3, 3, (11, 13), (3, 3), p=2, g=3, mode="reflect"), 0, None),
    (Case(2, 3, 3, (11, 13), (3, 3), p=2, g=3, mode="replicate"), 0, None),
    (Case(2, 3, 3, (11, 13), (3, 3), p=2, g=3, mode="circular"), 0, None),
    (FIRST, 3, None),
    (FIRST, 2, None),
    (FIRST, 0, 3),
]
TRANSPOSED = Case(2, 4, 4, (7, 9), (3, 3), s=2, p=1, op=1, g=4, tr=True)
TWO_PER_GROUP = Case(2, 6, 3, (12, 13), (3, 3), p=1, g=3)


def ident(v):
    return v.ident() if isinstance(v, Case) else None if v is None else str(v)


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for k in KNOBS + (BODY,):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("c,knob,body", [
    (FIRST, None, "valu"), (TWO_PER_GROUP, None, "mfma"), (TWO_PER_GROUP, "valu", "mfma"), (FIRST, "mfma", "mfma"),
    (Case(2, 3, 3 * M, (12, 13), (3, 3), p=1, g=3), None, "valu"),
    (Case(2, 3, 3 * (M + 1), (12, 13), (3, 3), p=1, g=3), None, "mfma"),
    (Case(2, 3, 3 * (M + 1), (12, 13), (3, 3), p=1, g=3), "valu", "valu"),
], ids=ident)
def test_body_of_a_layer_under_the_knob(c, knob, body, monkeypatch):
    if knob:
        monkeypatch.setenv(BODY, knob)
    assert _native.wgrad_direct_body(desc_of(c), CUS) == body


@pytest.mark.parametrize("c,dtype,_", DEPTHWISE[:-1], ids=ident)
@pytest.mark.parametrize("forced", [None, 1, 3, 10 ** 6])
def test_geometry_of_the_depthwise_body(c, dtype, _, forced, monkeypatch):
    if forced is not None:
        monkeypatch.setenv("FFTCONV_WGRAD_DIRECT_SLICES", str(forced))
    assert _native.wgrad_direct_body(desc_of(c, dtype), CUS) == "valu"
    geom = _native.wgrad_direct_geometry(desc_of(c, dtype), CUS)
    units = units_of(c, geom)
    assert all(1 <= geom[f"tile{i}"] <= o for i, o in enumerate(au.out_spatial(c))) and (c.nd == 3 or geom["tile2"] == 0)
    assert geom["out_block"] == geom["in_block"] == 1
    assert 0 < geom["lds_bytes"] <= 160 * 1024
    assert 1 <= geom["slices"] <= units
    if forced is not None:
        assert geom["slices"] == min(forced, units)
    assert geom["workspace_bytes"] == geom["slices"] * c.cout * math.prod(c.k) * 4


def test_slices_fill_the_device_several_workgroups_deep():
    # B8 C256 56^2 k7: channels x slices reach 4 workgroups per CU, where two slices per channel left the MFMA body idle
    geom = _native.wgrad_direct_geometry(desc_of(Case(8, 256, 256, (56, 56), (7, 7), p=3, g=256), 3), CUS)
    assert 256 * geom["slices"] == 4 * CUS and geom["lds_bytes"] <= 160 * 1024 // 4
