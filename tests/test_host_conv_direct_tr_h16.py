"""The planner of the direct strided transposed convolution on the 16-bit matrix instructions
(``fc_conv_direct_tr_h16_geometry``, csrc/host_direct.cpp) on the table tests/test_gpu_conv_direct_tr_h16.py runs: covered
or refused as listed, and the words the launch is sized by.  No GPU."""
import math

import pytest

from fft_conv_pytorch_amd import _native
from tests.route_util import Case
from tests.test_host_conv_direct import CUS, desc_of
from tests.test_host_conv_direct_tr import FORWARD, REFUSED, UNEVEN, T

# a group of two whole cells of 8 channels and a ragged one
RAGGED = T(2, 20, 6, (7, 9), (3, 3), s=2, p=1, note="ragged-cell")
# 10 cells: 68 MFMA steps over the 8 phases (8, 4, 4, 2, 4, 2, 2 and 1 taps), past the 64 of a block
TWO_IN_BLOCKS = T(2, 80, 4, (4, 5, 6), (3, 3, 3), s=2, p=1, op=1, note="two-in-blocks-h16")
CASES = list({c.ident(): c for c, _ in FORWARD}.values()) + [RAGGED, TWO_IN_BLOCKS]
ids = lambda v: v.ident() if isinstance(v, Case) else f"dt{v}" if isinstance(v, int) else None      # noqa: E731


@pytest.mark.parametrize("dtype", [3, 2], ids=ids)
@pytest.mark.parametrize("c", CASES, ids=ids)
def test_geometry_of_a_covered_layer(c, dtype):
    geom = _native.conv_direct_tr_h16_geometry(desc_of(c, dtype), CUS)
    assert tuple(geom) == _native.CONV_DIRECT_TR_INFO_WORDS
    assert all(geom[f"tile{i}"] >= 1 for i in range(c.nd)) and (c.nd == 3 or geom["tile2"] == 0)
    assert math.prod(geom[f"tile{i}"] for i in range(c.nd)) <= 1024
    assert geom["phases"] == math.prod(c.tup(c.s)) and 1 <= geom["phases_per_pass"] <= geom["phases"]
    assert geom["phases_per_pass"] % c.tup(c.s)[-1] == 0      # whole rows of last-axis phases
    cig = c.cin // c.g
    assert geom["in_block"] % 8 == 0 and 8 <= geom["in_block"] <= -(-cig // 8) * 8      # whole cells
    assert geom["in_blocks"] == -(-cig // geom["in_block"])
    assert 0 < geom["lds_bytes"] <= 160 * 1024
    assert c is not TWO_IN_BLOCKS or geom["in_blocks"] >= 2


@pytest.mark.parametrize("c,dtype,words", [(c, code or 3, words) for c, code, words in REFUSED] +
                         [(UNEVEN, 0, "float32: fc_conv_direct_tr covers it")], ids=ids)
def test_refused_layers_say_why(c, dtype, words):
    with pytest.raises(NotImplementedError, match=words):
        _native.conv_direct_tr_h16_geometry(desc_of(c, dtype), CUS)
