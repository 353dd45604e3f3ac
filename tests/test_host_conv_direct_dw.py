"""The planner of the direct depthwise forward (``fc_conv_direct_dw_geometry``, csrc/host_direct.cpp) on the table
tests/test_gpu_conv_direct_dw.py runs: covered or refused as listed, and the words the launch is sized by.  No GPU."""
import pytest

from fft_conv_pytorch_amd import _native
from tests import accuracy_util as au
from tests.route_util import Case
from tests.test_host_conv_direct import DEPTHWISE, desc_of, dx_case
from tests.test_host_wgrad_direct import CUS, FIRST, TAPS_147

KNOB = "FFTCONV_DIRECT_DW"
MULT = {m: Case(2, 3, 3 * m, (12, 13), (3, 3), p=1, g=3, note=f"multiplier-{m}") for m in (2, 3, 8)}
MULT_9 = Case(2, 2, 18, (12, 13), (3, 3), p=1, g=2, note="multiplier-9")
VOLUME = Case(1, 4, 4, (5, 6, 7), (3, 3, 3), p=1, g=4)
TILES = Case(1, 2, 2, (40, 150), (3, 3), p=1, g=2, note="tiles")
STRIDED = Case(2, 4, 4, (21, 37), (3, 5), s=(2, 1), d=(1, 2), p=(2, 3), g=4)
# (case, fc_dtype code of x, weight, bias and y)
FORWARD = [
    (DEPTHWISE, 0), (DEPTHWISE, 3), (DEPTHWISE, 2),
    (MULT[2], 0), (MULT[3], 0), (MULT[8], 0),
    (VOLUME, 0),
    (Case(1, 2, 2, (14, 15), (11, 11), p=5, g=2, note="121-taps"), 0),
    (Case(1, 2, 2, (9, 20), (2, 8), p=(1, 3), g=2, note="kx-8"), 0),
    (Case(1, 2, 2, (11, 13), (1, 5), p=(0, 2), g=2), 0), (Case(1, 2, 2, (11, 13), (5, 1), p=(2, 0), g=2), 0),
    (STRIDED, 0),
    (Case(2, 4, 4, (21, 37), (3, 5), s=(1, 2), p=(1, 2), g=4, note="stride-2-last"), 0),
    (TILES, 0),
] + [(Case(2, 3, 3, (11, 13), (3, 3), p=2, g=3, mode=mode), 0) for mode in ("reflect", "replicate", "circular")] + [
    (Case(2, 3, 3, (11, 13), (3, 3), g=3, note="padding-0"), 0),
    (Case(2, 4, 4, (7, 9), (3, 3), p=1, g=4, tr=True), 0), (Case(2, 8, 4, (7, 9), (3, 3), p=1, g=4, tr=True), 0),
]
# stride-1 zero-padded layers whose dX is the transposed form
DX = [(DEPTHWISE, 0), (DEPTHWISE, 3), (MULT[3], 0), (MULT[8], 0), (MULT[8], 3), (VOLUME, 0)]
REFUSED = [
    (FIRST, 0, "depthwise layers only"), (MULT_9, 0, "multipliers of at most 8"), (Case(2, 2, 2, (40,), (3,), p=1, g=2), 0, "1-D"),
    (DEPTHWISE, 1, "float64"), (DEPTHWISE, 4, "complex64"),
    (TAPS_147, 0, "128 taps"),
    (Case(2, 4, 4, (7, 9), (3, 3), s=2, p=1, g=4, tr=True), 0, "stride 1"),
    (Case(2, 4, 4, (7, 9), (3, 3), p=1, op=1, g=4, tr=True), 0, "output padding"),
    (Case(2, 4, 4, (7, 9), (3, 3), p=3, g=4, tr=True), 0, "crop"),
]
ids = lambda v: v.ident() if isinstance(v, Case) else f"dt{v}" if isinstance(v, int) else None      # noqa: E731


@pytest.mark.parametrize("c,dtype", FORWARD + [(dx_case(c), code) for c, code in DX], ids=ids)
def test_geometry_of_a_covered_layer(c, dtype):
    geom = _native.conv_direct_dw_geometry(desc_of(c, dtype), CUS)
    out, m = au.out_spatial(c), max(c.cin, c.cout) // c.g
    assert all(1 <= geom[f"tile{i}"] <= o for i, o in enumerate(out)) and (c.nd == 3 or geom["tile2"] == 0)
    assert 0 < geom["lds_bytes"] <= 160 * 1024
    assert geom["slots"] == 1 if c.tr else m <= geom["slots"] <= 8
    general = c.tup(c.s)[-1] != 1 or c.tup(c.d)[-1] != 1
    assert (geom["taps_per_block"] == 1) == general and geom["taps_per_block"] in (1, 4, 8)
    assert geom["slots"] * geom["runs_per_thread"] == 8
    tiles = 1
    for i, o in enumerate(out):
        tiles *= -(-o // geom[f"tile{i}"])
    assert geom["workgroups"] == c.B * c.g * tiles


def test_the_two_direct_routes_partition_the_multipliers():
    assert _native.conv_direct_geometry(desc_of(MULT_9), CUS)["out_block"] == 9
    with pytest.raises(NotImplementedError, match="depthwise"):
        _native.conv_direct_geometry(desc_of(MULT[8]), CUS)


@pytest.mark.parametrize("c,dtype,words", REFUSED, ids=ids)
def test_refused_layers_say_why(c, dtype, words):
    with pytest.raises(NotImplementedError, match=words):
        _native.conv_direct_dw_geometry(desc_of(c, dtype), CUS)
