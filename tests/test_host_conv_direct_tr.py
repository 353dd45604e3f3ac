"""The planner of the direct strided transposed convolution (``fc_conv_direct_tr_geometry``, csrc/host_direct.cpp) on the
table tests/test_gpu_conv_direct_tr.py runs: covered or refused as listed, and the words the launch is sized by.  No GPU."""
import math

import pytest

from fft_conv_pytorch_amd import _native
from tests.route_util import Case
from tests.test_host_conv_direct import CUS, GROUPS, desc_of

KNOB = "FFTCONV_DIRECT_TR"


def T(*a, **kw):
    return Case(*a, tr=True, **kw)


UNEVEN = T(2, 4, 6, (7, 9), (3, 3), s=2, p=1, note="uneven-phases")
NO_TAP = T(2, 4, 6, (7, 9), (3, 3), s=2, d=2, p=2, op=1, note="phases-without-a-tap")
MIXED = T(3, 10, 6, (11, 19), (3, 5), s=(2, 1), d=(1, 2), p=(2, 3), g=2, note="mixed")
PHASES_16 = T(1, 2, 3, (5, 6), (5, 5), s=4, p=1, note="16-phases")
# (case, fc_dtype code of x, weight, bias and y)
FORWARD = [
    (UNEVEN, 0), (UNEVEN, 3), (UNEVEN, 2),
    (T(2, 4, 6, (7, 9), (4, 4), s=2, p=1, note="even-phases"), 0),
    (T(2, 4, 6, (7, 9), (2, 2), s=2, note="no-halo"), 0),
    (T(2, 4, 6, (7, 9), (3, 3), s=2, p=1, op=1, note="output-padding"), 0),
    (NO_TAP, 0),
    (T(2, 4, 6, (6, 7), (1, 3), s=(3, 2), note="k<s"), 0),
    (MIXED, 0),
    (T(2, 3, 4, (7, 8), (5, 5), s=3, p=2, op=2, note="stride-3"), 0),
    (PHASES_16, 0),
    (T(1, 2, 2, (3, 3), (8, 8), s=8, note="64-phases"), 0),
    (T(2, 4, 6, (7, 9), (3, 3), s=2, p=3, note="padding-past-the-kernel"), 0),
    (T(2, 3, 20, (6, 7), (3, 3), s=2, p=1, note="two-out-blocks"), 0),
    (T(2, 20, 4, (4, 5, 6), (3, 3, 3), s=2, p=1, op=1, note="two-in-blocks"), 0),
    (T(1, 2, 2, (40, 70), (3, 3), s=2, p=1, note="tile-seams"), 0),
]
# strided layers whose dX is the strided transposed form
DX = [(GROUPS, 0), (Case(2, 8, 16, (12, 13), (3, 3), s=2, p=1), 0), (Case(2, 8, 16, (12, 13), (3, 3), s=2, p=1), 3),
      (Case(2, 4, 4, (7, 8, 9), (3, 3, 3), s=2, p=1), 0)]
REFUSED = [
    (Case(2, 4, 6, (7, 9), (3, 3), s=2, p=1), 0, "not transposed: fc_conv_direct covers it"),
    (T(2, 4, 6, (7, 9), (3, 3), p=1), 0, "at stride 1: fc_conv_direct covers it"),
    (T(2, 5, 5, (7, 9), (3, 3), s=2, p=1, g=5), 0, "depthwise"),
    (T(2, 2, 2, (40,), (3,), s=2), 0, "1-D"), (UNEVEN, 1, "float64"), (UNEVEN, 4, "complex64"),
    (T(1, 2, 2, (4, 10, 11), (3, 7, 7), s=2), 0, "128 taps"),
    (T(1, 2, 2, (3, 3), (3, 3), s=9), 0, "stride of at most 8"),
    (T(1, 2, 2, (3, 3, 3), (3, 3, 3), s=(8, 8, 2)), 0, "at most 64 phases"),
    (T(1, 2, 2, (600, 600), (5, 5), s=2, d=120, note="halo"), 0, "LDS"),
    (T(2 ** 31, 2, 2, (3, 3), (3, 3), s=2), 0, "units exceed 2.31"),
    (T(2 ** 28, 2, 256, (1, 1), (2, 2), s=2), 0, "workgroups exceed"),
]
ids = lambda v: v.ident() if isinstance(v, Case) else f"dt{v}" if isinstance(v, int) else None      # noqa: E731


@pytest.mark.parametrize("c,dtype", FORWARD, ids=ids)
def test_geometry_of_a_covered_layer(c, dtype):
    geom = _native.conv_direct_tr_geometry(desc_of(c, dtype), CUS)
    assert tuple(geom) == _native.CONV_DIRECT_TR_INFO_WORDS
    assert all(geom[f"tile{i}"] >= 1 for i in range(c.nd)) and (c.nd == 3 or geom["tile2"] == 0)
    assert math.prod(geom[f"tile{i}"] for i in range(c.nd)) <= 1024
    assert geom["phases"] == math.prod(c.tup(c.s)) and 1 <= geom["phases_per_pass"] <= geom["phases"]
    assert geom["phases_per_pass"] % c.tup(c.s)[-1] == 0      # whole rows of last-axis phases
    cig = c.cin // c.g
    assert 1 <= geom["in_block"] <= cig and geom["in_blocks"] == -(-cig // geom["in_block"])
    assert geom["in_block"] * math.prod(c.k) <= 512
    assert 0 < geom["lds_bytes"] <= 160 * 1024


def test_sixteen_phases_pass_in_whole_rows_and_a_long_reduction_in_blocks():
    geom = _native.conv_direct_tr_geometry(desc_of(PHASES_16), CUS)
    assert geom["phases"] == 16 and geom["phases_per_pass"] in (4, 8, 12, 16)
    two = next(c for c, _ in FORWARD if c.note == "two-in-blocks")
    assert _native.conv_direct_tr_geometry(desc_of(two), CUS)["in_blocks"] == 2      # 540 columns


@pytest.mark.parametrize("c,dtype,words", REFUSED, ids=ids)
def test_refused_layers_say_why(c, dtype, words):
    with pytest.raises(NotImplementedError, match=words):
        _native.conv_direct_tr_geometry(desc_of(c, dtype), CUS)


def test_the_stride_1_planner_still_refuses_a_strided_transposed_layer():
    with pytest.raises(NotImplementedError, match="stride 1"):
        _native.conv_direct_geometry(desc_of(UNEVEN), CUS)
