"""The planner of the direct small-kernel forward (``fc_conv_direct_geometry``, csrc/host_direct.cpp) on the table
tests/test_gpu_conv_direct.py runs: covered or refused as listed, and the words the launch is sized by.  No GPU."""
import math

import pytest

from fft_conv_pytorch_amd import _native
from tests import accuracy_util as au
from tests.route_util import Case
from tests.test_host_wgrad_direct import CUS, FIRST, TAPS_147

KNOB = "FFTCONV_DIRECT"
TWO_IN_BLOCKS = Case(2, 20, 4, (5, 6, 7), (3, 3, 3), p=1, note="two-in-blocks")
GROUPS = Case(3, 6, 10, (21, 37), (3, 5), s=(2, 1), d=(1, 2), p=(2, 3), g=2)
# (case, fc_dtype code of x, weight, bias and y)
FORWARD = [
    (FIRST, 0), (FIRST, 3), (FIRST, 2),
    (Case(2, 3, 20, (12, 13), (3, 3), p=1, note="two-out-blocks"), 0),
    (TWO_IN_BLOCKS, 0),
    (GROUPS, 0),
    (Case(1, 2, 2, (7, 8, 9), (5, 5, 5), p=2, note="125-taps"), 0),
    (Case(1, 2, 2, (4, 10, 11), (2, 8, 8), p=(1, 3, 3), note="128-taps"), 0),
    (Case(2, 3, 4, (11, 13), (3, 3), p=2, mode="reflect"), 0),
    (Case(2, 3, 4, (11, 13), (3, 3), p=2, mode="replicate"), 0),
    (Case(2, 3, 4, (11, 13), (3, 3), p=2, mode="circular"), 0),
    (Case(2, 4, 4, (11, 13), (3, 3), note="padding-0"), 0),
    (Case(2, 2, 32, (12, 13), (3, 3), p=1, g=2, note="multiplier-16"), 0),
]
# stride-1 layers whose dX is the transposed form
DX = [
    (FIRST, 0), (FIRST, 3),
    (TWO_IN_BLOCKS, 0),
    (Case(2, 4, 20, (5, 6, 7), (3, 3, 3), p=1, note="two-in-blocks-of-dx"), 0),
    (Case(3, 6, 10, (21, 37), (3, 5), d=(2, 1), p=(2, 2), g=2), 0),
    (Case(2, 4, 4, (11, 13), (3, 3), note="padding-0"), 0),
]
TRANSPOSED = Case(2, 2, 4, (7, 9), (3, 3), p=1, g=2, tr=True)
DEPTHWISE = Case(2, 5, 5, (23, 17), (7, 7), p=3, g=5, note="depthwise")
REFUSED = [
    (TAPS_147, 0, "128 taps"), (FIRST, 1, "float64"), (Case(2, 2, 2, (9, 9), (3, 3), p=1), 4, "complex64"),
    (Case(2, 2, 2, (40,), (3,), p=1), 0, "1-D"), (DEPTHWISE, 0, "depthwise"),
    (Case(1, 1, 1, (600, 600), (5, 5), d=120, note="halo"), 0, "LDS"),
    (Case(2, 4, 6, (7, 9), (3, 3), s=2, p=1, tr=True), 0, "stride 1"),
    (Case(2, 4, 6, (7, 9), (3, 3), p=1, op=1, tr=True), 0, "output padding"),
    (Case(2, 4, 6, (7, 9), (3, 3), p=3, tr=True), 0, "crop"),
]


def desc_of(c, dtype=0):
    return _native.conv_desc(c.nd, c.B, c.cin, c.cout, c.g, c.size, c.k, c.tup(c.s), c.tup(c.p), c.tup(c.d),
                             _native.PAD_MODES[c.mode], dtype, transposed=c.tr, output_padding=c.tup(c.op))


def dx_case(c):
    """The stride-1 transposed layer that is the dX of the stride-1 layer c: dY is its signal."""
    return Case(c.B, c.cout, c.cin, au.out_spatial(c), c.k, p=c.p, d=c.d, g=c.g, tr=True)


@pytest.mark.parametrize("c,dtype", FORWARD + [(dx_case(c), code) for c, code in DX] + [(TRANSPOSED, 0)],
                         ids=lambda v: v.ident() if isinstance(v, Case) else f"dt{v}")
def test_geometry_of_a_covered_layer(c, dtype):
    geom = _native.conv_direct_geometry(desc_of(c, dtype), CUS)
    out, cig, cog = au.out_spatial(c), c.cin // c.g, c.cout // c.g
    assert all(1 <= geom[f"tile{i}"] <= o for i, o in enumerate(out)) and (c.nd == 3 or geom["tile2"] == 0)
    assert math.prod(geom[f"tile{i}"] for i in range(c.nd)) <= 1024
    assert geom["out_block"] == min(cog, 16) and geom["out_blocks"] == -(-cog // 16)
    assert 1 <= geom["in_block"] <= cig and geom["in_blocks"] == -(-cig // geom["in_block"])
    assert geom["in_block"] * math.prod(c.k) <= 512
    assert 0 < geom["lds_bytes"] <= 160 * 1024


def test_a_long_reduction_runs_in_blocks():
    assert _native.conv_direct_geometry(desc_of(TWO_IN_BLOCKS), CUS)["in_blocks"] == 2      # 540 columns


@pytest.mark.parametrize("c,dtype,words", REFUSED, ids=lambda v: v.ident() if isinstance(v, Case) else None)
def test_refused_layers_say_why(c, dtype, words):
    with pytest.raises(NotImplementedError, match=words):
        _native.conv_direct_geometry(desc_of(c, dtype), CUS)
