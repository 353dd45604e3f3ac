"""The direct small-kernel forward and input gradient (``fc_conv_direct``, csrc/conv_direct.hpp) under FFTCONV_DIRECT=1.

Inputs are the integers of tests/accuracy_util.py.  With (Cin/g x taps) x max|x| x 8 + 8 < 2**24 every float32 partial sum
of the time-domain sum is a whole number below 2**24, so the route must return the float64 truth itself, bit for bit,
whatever its order of summation; each test asserts the condition for its shape first.  16-bit tensors: the truth rounded
once.  The long reduction of the last test is bounded by ``accuracy_util.check`` against the float32 rfftn baseline."""
import math

import pytest
import torch

from fft_conv_pytorch_amd import _native, autograd, fft_conv, functional
from fft_conv_pytorch_amd.functional import fft_conv_transpose
from tests import accuracy_util as au
from tests.route_util import Case
from tests.test_host_conv_direct import DEPTHWISE, DX, FIRST, FORWARD, GROUPS, KNOB, TAPS_147, TRANSPOSED, desc_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {0: torch.float32, 1: torch.float64, 2: torch.float16, 3: torch.bfloat16, 4: torch.complex64}
ids = lambda v: v.ident() if isinstance(v, Case) else str(v)      # noqa: E731


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    monkeypatch.delenv("FFTCONV_WGRAD_DIRECT", raising=False)


def assert_whole_in_float32(c, cls, reduce_channels):
    """(channels per group of the reduction x taps) x max|x| x 8 + 8 < 2**24: every partial sum is exact in float32."""
    xmax = au.HI + (au.OFFSET if cls == "offset" else 0)
    assert reduce_channels * math.prod(c.k) * xmax * au.HI + au.HI < 2 ** 24


def conf(c):
    return c.tup(c.s), c.tup(c.p), c.tup(c.d), c.g, c.mode


def call(c, x, w, b, **kw):
    if c.tr:
        return fft_conv_transpose(x, w, b, stride=c.s, padding=c.p, output_padding=c.op, dilation=c.d, groups=c.g, **kw)
    return fft_conv(x, w, b, stride=c.s, padding=c.p, dilation=c.d, groups=c.g, padding_mode=c.mode, **kw)


def route(c, x, w, **kw):
    return functional.conv_route(x, tuple(w.shape), c.s, c.p, c.d, c.g, c.mode, transposed=c.tr, output_padding=c.op, **kw)


# (float16: the centred class only, so that |y| stays below 65,504)
@pytest.mark.parametrize("c,code,cls", [(c, code, cls) for c, code in FORWARD + [(TRANSPOSED, 0)] for cls in au.CLASSES
                                        if code != 2 or cls == "centred"], ids=ids)
def test_direct_forward_is_the_truth_bit_for_bit(c, code, cls, monkeypatch):
    assert_whole_in_float32(c, cls, c.cin // c.g)
    dtype = DTYPES[code]
    x, w, b = au.inputs(c, cls)
    want = au.truth(c, x, w, b)
    assert code != 2 or want.abs().max() < 65504
    monkeypatch.setenv(KNOB, "1")
    x, w, b = (t.to(DEV, dtype) for t in (x, w, b))
    assert route(c, x, w) == "direct"
    got = call(c, x, w, b)
    assert got.dtype == dtype and torch.equal(got.cpu(), want.to(dtype))


@pytest.mark.parametrize("c,code", DX, ids=ids)
def test_direct_dx_is_the_truth_bit_for_bit(c, code, monkeypatch):
    assert_whole_in_float32(c, "centred", c.cout // c.g)
    dtype = DTYPES[code]
    x, w, b = au.inputs(c, "centred")
    gy = au.grad_output((c.B, c.cout) + au.out_spatial(c), torch.float32)
    want = au.truth_grads(c, x, w, b, gy, only_dx=True)[0]
    monkeypatch.setenv(KNOB, "1")
    xr, w, gy = x.to(DEV, dtype).requires_grad_(), w.to(DEV, dtype), gy.to(DEV, dtype)
    assert autograd.dx_route(xr, tuple(w.shape), *conf(c)) == "direct"
    call(c, xr, w, None).backward(gy)
    assert xr.grad.dtype == dtype and torch.equal(xr.grad.cpu(), want.to(dtype))


REFUSED = [(TAPS_147, 0, {}), (FIRST, 1, {}), (Case(2, 2, 2, (9, 9), (3, 3), p=1), 4, {}), (DEPTHWISE, 0, {}),
           (FIRST, 0, {"channels_last": True})]


@pytest.mark.parametrize("c,code,kw", REFUSED, ids=["147-taps", "float64", "complex64", "depthwise", "channels-last"])
def test_a_refused_call_keeps_its_route_and_its_bits(c, code, kw, monkeypatch):
    x, w, b = au.inputs(c, "centred", DEV, complex_=code == 4)
    x, w, b = (t.to(DTYPES[code]) for t in (x, w, b))
    before = call(c, x, w, b, **kw)
    monkeypatch.setenv(KNOB, "1")
    assert route(c, x, w, **kw) == "fft"
    after = call(c, x, w, b, **kw)
    assert after.stride() == before.stride() and torch.equal(after, before)


def test_a_strided_dx_keeps_its_plan_and_its_bits(monkeypatch):
    c = GROUPS
    x, w, _ = au.inputs(c, "centred", DEV)
    gy = au.grad_output((c.B, c.cout) + au.out_spatial(c), torch.float32, DEV)
    grads = []
    for knob in (None, "1"):
        if knob:
            monkeypatch.setenv(KNOB, knob)
        xr = x.clone().requires_grad_()
        assert autograd.dx_route(xr, tuple(w.shape), *conf(c)) == "plan"
        call(c, xr, w, None).backward(gy)
        grads.append(xr.grad)
    assert torch.equal(grads[0], grads[1])


def test_unset_switch_names_todays_routes():
    x, w, _ = au.inputs(FIRST, "centred", DEV)
    assert route(FIRST, x, w) == "fft" and autograd.dx_route(x, tuple(w.shape), *conf(FIRST)) == "plan"


def test_every_output_byte_is_written_and_y_is_not_read():
    c = FIRST
    assert_whole_in_float32(c, "offset", c.cin // c.g)
    x, w, b = au.inputs(c, "offset")
    want = au.truth(c, x, w, b)
    x, w, b = (t.to(DEV) for t in (x, w, b))
    results = []
    for fill in (float("nan"), 0.0):
        y = torch.full(tuple(want.shape), fill, device=DEV)
        with torch.cuda.device(DEV):
            _native.conv_direct(desc_of(c), x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        results.append(y)
    assert torch.equal(results[0], results[1]) and torch.equal(results[0].double().cpu(), want)


def test_accuracy_of_a_long_reduction(monkeypatch):
    """B2 64 -> 8 16^3 k3 'same': 1,728 terms per output in four chains of 432, against float64 conv3d and its autograd
    and the float32 rfftn baseline at the default margins (measured figures: DESIGN 4.5d)."""
    c = Case(2, 64, 8, (16, 16, 16), (3, 3, 3), p=1)
    gen = torch.Generator().manual_seed(5)
    x, w, b, gy = (torch.randn(s, generator=gen).to(DEV) for s in ((2, 64, 16, 16, 16), (8, 64, 3, 3, 3), (8,), (2, 8, 16, 16, 16)))
    xd, wd = x.double().requires_grad_(), w.double()
    yd = torch.nn.functional.conv3d(xd, wd, b.double(), padding=1)
    yd.backward(gy.double())
    base_y, base_dx = au.baseline_grads(c, x, w, b, gy, only_dx=True)[:2]
    monkeypatch.setenv(KNOB, "1")
    xr = x.clone().requires_grad_()
    assert route(c, xr, w) == "direct" and autograd.dx_route(xr, tuple(w.shape), *conf(c)) == "direct"
    y = call(c, xr, w, b)
    y.backward(gy)
    au.check("direct y", y.detach(), yd.detach(), base_y, torch.float32, rms_margin=au.RMS_MARGIN)
    au.check("direct dX", xr.grad, xd.grad, base_dx, torch.float32, rms_margin=au.RMS_MARGIN)
