"""The direct small-kernel weight gradient (``fc_wgrad_direct``, csrc/wgrad_direct.hpp) under FFTCONV_WGRAD_DIRECT=1.

Inputs are the integers of tests/accuracy_util.py.  With (terms per dW element) x max|x| x 8 < 2**24 every float32 partial
sum of the time-domain sum is a whole number below 2**24, so the route must return float64 autograd's dW itself, bit for
bit, whatever its order of summation; each test asserts the condition for its shape first.  The long reduction of the
last test is bounded by ``accuracy_util.check`` against the float32 rfftn baseline."""
import math

import pytest
import torch

from fft_conv_pytorch_amd import _native, autograd, fft_conv
from fft_conv_pytorch_amd.functional import fft_conv_transpose
from tests import accuracy_util as au
from tests.route_util import Case
from tests.test_host_wgrad_direct import COVERED, FIRST, KNOBS, TAPS_147, desc_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {0: torch.float32, 1: torch.float64, 2: torch.float16, 3: torch.bfloat16, 4: torch.complex64}
TRANSPOSED = Case(2, 4, 6, (7, 9), (3, 3), s=2, p=1, op=1, tr=True)
ACCURACY_MARGIN = au.RMS_MARGIN       # the default: the three-level sum needs no margin of its own


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    autograd._BWD_PLANS.clear()
    yield
    autograd._BWD_PLANS.clear()


def assert_whole_in_float32(c, cls):
    """(terms per dW element) x max|x| x 8 < 2**24: every partial sum is exact in float32."""
    out = c.size if c.tr else au.out_spatial(c)      # (a transposed layer's dW: dY is the signal, x the output gradient)
    xmax = au.HI + (au.OFFSET if cls == "offset" else 0)
    assert c.B * math.prod(out) * xmax * au.HI < 2 ** 24


def public_dw(c, x, w, gy):
    """(dW through the public call's backward, the route ``dw_route`` names for it)."""
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    if c.tr:
        y = fft_conv_transpose(xr, wr, None, stride=c.s, padding=c.p, output_padding=c.op, dilation=c.d, groups=c.g)
        signal, conf = gy, (c.tup(c.s), c.tup(c.p), c.tup(c.d), c.g, "constant")
    else:
        y = fft_conv(xr, wr, None, stride=c.s, padding=c.p, dilation=c.d, groups=c.g, padding_mode=c.mode)
        signal, conf = x, (c.tup(c.s), c.tup(c.p), c.tup(c.d), c.g, c.mode)
    assert y.shape == gy.shape
    y.backward(gy)
    return wr.grad, autograd.dw_route(signal, tuple(w.shape), *conf)


def operands(c, cls, dtype):
    x, w, b = au.inputs(c, cls)
    gy = au.grad_output((c.B, c.cout) + au.out_spatial(c), torch.float32)
    want = au.truth_grads(c, x, w, b, gy)[1]
    return x.to(DEV, dtype), w.to(DEV, dtype), gy.to(DEV, dtype), want


@pytest.mark.parametrize("cls", au.CLASSES)
@pytest.mark.parametrize("c,code,slices", [(c, code, None) for c, code in COVERED] + [(TRANSPOSED, 0, None), (FIRST, 0, 3)],
                         ids=lambda v: v.ident() if isinstance(v, Case) else None if v is None else str(v))
def test_direct_dw_is_the_truth_bit_for_bit(c, code, slices, cls, monkeypatch):
    assert_whole_in_float32(c, cls)
    monkeypatch.setenv("FFTCONV_WGRAD_DIRECT", "1")
    if slices:
        monkeypatch.setenv("FFTCONV_WGRAD_DIRECT_SLICES", str(slices))
    x, w, gy, want = operands(c, cls, DTYPES[code])
    got, route = public_dw(c, x, w, gy)
    assert route == "direct"
    # (a 16-bit weight receives the float32 dW rounded once: the truth, a whole number below 2**24, rounded the same way)
    assert got.dtype == w.dtype and torch.equal(got.cpu(), want.to(w.dtype))


@pytest.mark.parametrize("c,code", [(TAPS_147, 0), (FIRST, 1), (Case(2, 2, 2, (9, 9), (3, 3), p=1), 4)],
                         ids=["147-taps", "float64", "complex64"])
def test_a_refused_layer_keeps_its_route_and_its_bits(c, code, monkeypatch):
    x, w, _ = au.inputs(c, "centred", DEV, complex_=code == 4)
    x, w = x.to(DTYPES[code]), w.to(DTYPES[code])
    gy = au.grad_output((c.B, c.cout) + au.out_spatial(c), DTYPES[code], DEV)
    before, route_before = public_dw(c, x, w, gy)
    monkeypatch.setenv("FFTCONV_WGRAD_DIRECT", "1")
    autograd._BWD_PLANS.clear()
    after, route_after = public_dw(c, x, w, gy)
    assert route_after == route_before != "direct"
    assert torch.equal(after, before)


def test_unset_switch_names_todays_route():
    x, w, gy, _ = operands(FIRST, "centred", torch.float32)
    assert public_dw(FIRST, x, w, gy)[1] == "wgrad_nd"


def test_bits_do_not_depend_on_the_workspace():
    c = FIRST
    assert_whole_in_float32(c, "offset")
    x, w, gy, want = operands(c, "offset", torch.float32)
    desc = desc_of(c)
    geom = _native.wgrad_direct_geometry(desc, torch.cuda.get_device_properties(DEV).multi_processor_count)
    results = []
    for fill in (float("nan"), 0.0):
        ws = torch.full((geom["workspace_bytes"] // 4,), fill, device=DEV)
        dw = torch.full(tuple(w.shape), float("nan"), device=DEV)
        with torch.cuda.device(DEV):
            _native.wgrad_direct(desc, x.data_ptr(), gy.data_ptr(), dw.data_ptr(), ws.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        results.append(dw)
    assert torch.equal(results[0], results[1]) and torch.equal(results[0].double().cpu(), want)


def test_accuracy_of_a_long_reduction(monkeypatch):
    """B2 2 -> 2 64^3 k3 'same': 524,288 terms per element of dW in three levels (a unit of 512 positions, the units of a
    slice, the slices in blocks of 16), against float64 autograd and the float32 rfftn baseline."""
    c = Case(2, 2, 2, (64, 64, 64), (3, 3, 3), p=1)
    gen = torch.Generator().manual_seed(5)
    x, w, gy = (torch.randn(s, generator=gen).to(DEV) for s in ((2, 2, 64, 64, 64), (2, 2, 3, 3, 3), (2, 2, 64, 64, 64)))
    b = torch.zeros(2, device=DEV)
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    torch.nn.functional.conv3d(xr, wr, None, padding=1).backward(gy.double())
    base = au.baseline_grads(c, x, w, b, gy)[2]
    monkeypatch.setenv("FFTCONV_WGRAD_DIRECT", "1")
    got, route = public_dw(c, x, w, gy)
    assert route == "direct"
    au.check("direct dW", got, wr.grad, base, torch.float32, rms_margin=ACCURACY_MARGIN)
