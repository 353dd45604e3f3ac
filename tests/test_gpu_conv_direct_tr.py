"""The direct strided transposed convolution (``fc_conv_direct_tr``, csrc/conv_direct_tr.hpp) under FFTCONV_DIRECT_TR=1.

Inputs are the integers of tests/accuracy_util.py under the exactness condition of tests/test_gpu_conv_direct.py, so the
route must return the float64 truth itself, bit for bit (16-bit tensors: the truth rounded once).  The long reduction of
the last test is bounded by ``accuracy_util.check`` against the float32 rfftn baseline."""
import pytest
import torch

from fft_conv_pytorch_amd import _native, autograd, functional
from tests import accuracy_util as au
from tests.route_util import Case
from tests.test_gpu_conv_direct import DEV, DTYPES, assert_whole_in_float32, call, conf, ids, route
from tests.test_host_conv_direct import desc_of
from tests.test_host_conv_direct_tr import DX, FORWARD, KNOB, MIXED, NO_TAP, UNEVEN, T

pytestmark = pytest.mark.gpu
KNOBS = (KNOB, "FFTCONV_DIRECT", "FFTCONV_DIRECT_DW", "FFTCONV_WGRAD_DIRECT")


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)


# (float16: the centred class only, so that |y| stays below 65,504)
@pytest.mark.parametrize("c,code,cls", [(c, code, cls) for c, code in FORWARD for cls in au.CLASSES
                                        if code != 2 or cls == "centred"], ids=ids)
def test_forward_is_the_truth_bit_for_bit(c, code, cls, monkeypatch):
    assert_whole_in_float32(c, cls, c.cin // c.g)
    dtype = DTYPES[code]
    x, w, b = au.inputs(c, cls)
    want = au.truth(c, x, w, b)
    assert code != 2 or want.abs().max() < 65504
    monkeypatch.setenv(KNOB, "1")
    x, w, b = (t.to(DEV, dtype) for t in (x, w, b))
    assert route(c, x, w) == "direct-tr"
    got = call(c, x, w, b)
    assert got.dtype == dtype and torch.equal(got.cpu(), want.to(dtype))


@pytest.mark.parametrize("c,code", DX, ids=ids)
def test_dx_of_a_strided_layer_is_the_truth_bit_for_bit(c, code, monkeypatch):
    assert_whole_in_float32(c, "centred", c.cout // c.g)
    dtype = DTYPES[code]
    x, w, b = au.inputs(c, "centred")
    gy = au.grad_output((c.B, c.cout) + au.out_spatial(c), torch.float32)
    want = au.truth_grads(c, x, w, b, gy, only_dx=True)[0]
    monkeypatch.setenv(KNOB, "1")
    xr, w, gy = x.to(DEV, dtype).requires_grad_(), w.to(DEV, dtype), gy.to(DEV, dtype)
    assert autograd.dx_route(xr, tuple(w.shape), *conf(c)) == "direct-tr"
    call(c, xr, w, None).backward(gy)
    assert xr.grad.dtype == dtype and torch.equal(xr.grad.cpu(), want.to(dtype))


def test_every_output_byte_is_written_and_y_is_not_read():
    c = NO_TAP      # (three phases in four have no tap: their outputs are the bias)
    assert_whole_in_float32(c, "offset", c.cin // c.g)
    x, w, b = au.inputs(c, "offset")
    want = au.truth(c, x, w, b)
    x, w, b = (t.to(DEV) for t in (x, w, b))
    results = []
    for fill in (float("nan"), 0.0):
        y = torch.full(tuple(want.shape), fill, device=DEV)
        with torch.cuda.device(DEV):
            _native.conv_direct_tr(desc_of(c), x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        results.append(y)
    assert torch.equal(results[0], results[1]) and torch.equal(results[0].double().cpu(), want)


def test_without_the_switch_a_strided_transposed_call_keeps_its_route(monkeypatch):
    monkeypatch.setenv("FFTCONV_DIRECT", "1")
    for c in (UNEVEN, MIXED):
        x, w, _ = au.inputs(c, "centred", DEV)
        assert route(c, x, w) == "fft"
    for c, _ in DX:
        x, w, _ = au.inputs(c, "centred", DEV)
        assert autograd.dx_route(x, tuple(w.shape), *conf(c)) == "plan"


@pytest.mark.parametrize("c,code", [(UNEVEN, 1), (T(2, 5, 5, (7, 9), (3, 3), s=2, p=1, g=5), 0), (T(2, 4, 6, (7, 9), (3, 3), p=1), 0)],
                         ids=["float64", "depthwise", "stride-1"])
def test_a_refused_call_keeps_its_route_and_its_bits(c, code, monkeypatch):
    x, w, b = (t.to(DTYPES[code]) for t in au.inputs(c, "centred", DEV))
    before = call(c, x, w, b)
    monkeypatch.setenv(KNOB, "1")
    assert route(c, x, w) == "fft"
    after = call(c, x, w, b)
    assert after.stride() == before.stride() and torch.equal(after, before)


def test_accuracy_of_a_long_reduction(monkeypatch):
    """B2 64 -> 8 8^3 k3 s2 p1 op1 transposed on random data: y (up to 8 taps x 64 channels per output) against float64
    conv_transpose3d, and the dX of the strided layer B2 8 -> 64 16^3 k3 s2 p1, which is the same transposed convolution
    reached through autograd, against float64 autograd; both held to the float32 rfftn baseline at the default margins
    (measured figures: DESIGN 4.5h)."""
    c = T(2, 64, 8, (8, 8, 8), (3, 3, 3), s=2, p=1, op=1)
    layer = Case(2, 8, 64, (16, 16, 16), (3, 3, 3), s=2, p=1)
    gen = torch.Generator().manual_seed(5)
    x, w, b, xl = (torch.randn(s, generator=gen).to(DEV) for s in ((2, 64, 8, 8, 8), (64, 8, 3, 3, 3), (8,), (2, 8, 16, 16, 16)))
    yd = torch.nn.functional.conv_transpose3d(x.double(), w.double(), b.double(), stride=2, padding=1, output_padding=1)
    xd = xl.double().requires_grad_()
    torch.nn.functional.conv3d(xd, w.double(), None, stride=2, padding=1).backward(x.double())
    base_y = au.baseline(c, x, w, b)
    base_dx = au.baseline_grads(layer, xl, w, torch.zeros(64, device=DEV), x, only_dx=True)[1]
    monkeypatch.setenv(KNOB, "1")
    xr = xl.clone().requires_grad_()
    assert route(c, x, w) == "direct-tr" and autograd.dx_route(xr, tuple(w.shape), *conf(layer)) == "direct-tr"
    y = call(c, x, w, b)
    call(layer, xr, w, None).backward(x)
    au.check("direct-tr y", y, yd, base_y, torch.float32, rms_margin=au.RMS_MARGIN)
    au.check("direct-tr dX", xr.grad, xd.grad, base_dx, torch.float32, rms_margin=au.RMS_MARGIN)
