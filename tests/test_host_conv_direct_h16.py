"""The planner of the direct forward on the 16-bit matrix instructions (``fc_conv_direct_h16_geometry``,
csrc/host_direct.cpp) on the table tests/test_gpu_conv_direct_h16.py runs: covered or refused as listed, and the words the
launch is sized by.  No GPU."""
import math

import pytest

from fft_conv_pytorch_amd import _native
from tests import accuracy_util as au
from tests.route_util import Case
from tests.test_host_conv_direct import DX, FIRST, FORWARD, REFUSED, TRANSPOSED, desc_of, dx_case
from tests.test_host_wgrad_direct import CUS

# 5 cells of 8 channels x 27 taps = 1080 columns: the smallest group of whole cells past the cap of 1024
TWO_IN_BLOCKS_H16 = Case(2, 40, 4, (5, 6, 7), (3, 3, 3), p=1, note="two-in-blocks-h16")
COVERED = [c for c, _ in FORWARD] + [dx_case(c) for c, _ in DX] + [TRANSPOSED, TWO_IN_BLOCKS_H16]
ids = lambda v: v.ident() if isinstance(v, Case) else f"dt{v}"      # noqa: E731


@pytest.mark.parametrize("dtype", [2, 3], ids=ids)
@pytest.mark.parametrize("c", COVERED, ids=ids)
def test_geometry_of_a_covered_layer(c, dtype):
    geom = _native.conv_direct_h16_geometry(desc_of(c, dtype), CUS)
    out, cig, cog = au.out_spatial(c), c.cin // c.g, c.cout // c.g
    assert all(1 <= geom[f"tile{i}"] <= o for i, o in enumerate(out)) and (c.nd == 3 or geom["tile2"] == 0)
    assert math.prod(geom[f"tile{i}"] for i in range(c.nd)) <= 1024
    assert geom["out_block"] == min(cog, 16) and geom["out_blocks"] == -(-cog // 16)
    assert geom["in_block"] % 8 == 0 or geom["in_block"] == cig
    assert 1 <= geom["in_block"] <= cig and geom["in_blocks"] == -(-cig // geom["in_block"])
    assert -(-geom["in_block"] // 8) * 8 * math.prod(c.k) <= 1024
    assert 0 < geom["lds_bytes"] <= 160 * 1024
    assert c is not TWO_IN_BLOCKS_H16 or geom["in_blocks"] >= 2


@pytest.mark.parametrize("c,dtype,words", [(c, code if code in (1, 4) else 3, words) for c, code, words in REFUSED] +
                         [(FIRST, 0, "fc_conv_direct covers"), (TWO_IN_BLOCKS_H16, 0, "fc_conv_direct covers")],
                         ids=lambda v: v.ident() if isinstance(v, Case) else None)
def test_refused_layers_say_why(c, dtype, words):
    with pytest.raises(NotImplementedError, match=words):
        _native.conv_direct_h16_geometry(desc_of(c, dtype), CUS)
