"""The direct depthwise forward and input gradient (``fc_conv_direct_dw``, csrc/conv_direct_dw.hpp) under
FFTCONV_DIRECT_DW=1.

Inputs are the integers of tests/accuracy_util.py.  With (channels of the reduction x taps) x max|x| x 8 + 8 < 2**24 every
float32 partial sum is a whole number below 2**24, so the route must return the float64 truth itself, bit for bit,
whatever its order of summation; each test asserts the condition for its shape first (the worst here is 8 x 121 x 72 x 8).
16-bit tensors: the truth rounded once.  The long reduction of the last test is bounded by ``accuracy_util.check``."""
import pytest
import torch

from fft_conv_pytorch_amd import _native, autograd
from tests import accuracy_util as au
from tests.route_util import Case
from tests.test_gpu_conv_direct import DEV, DTYPES, assert_whole_in_float32, call, conf, ids, route
from tests.test_host_conv_direct import DEPTHWISE, FIRST, desc_of
from tests.test_host_conv_direct_dw import DX, FORWARD, KNOB, MULT_9, STRIDED, TILES

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for knob in (KNOB, "FFTCONV_DIRECT", "FFTCONV_WGRAD_DIRECT"):
        monkeypatch.delenv(knob, raising=False)


# (float16: the centred class only, so that |y| stays below 65,504)
@pytest.mark.parametrize("c,code,cls", [(c, code, cls) for c, code in FORWARD for cls in au.CLASSES
                                        if code != 2 or cls == "centred"], ids=ids)
def test_direct_dw_forward_is_the_truth_bit_for_bit(c, code, cls, monkeypatch):
    assert_whole_in_float32(c, cls, c.cin // c.g)
    dtype = DTYPES[code]
    x, w, b = au.inputs(c, cls)
    want = au.truth(c, x, w, b)
    assert code != 2 or want.abs().max() < 65504
    monkeypatch.setenv(KNOB, "1")
    x, w, b = (t.to(DEV, dtype) for t in (x, w, b))
    assert route(c, x, w) == "direct-dw"
    got = call(c, x, w, b)
    assert got.dtype == dtype and torch.equal(got.cpu(), want.to(dtype))


def test_a_wide_layer_runs_in_more_than_one_tile_per_row():
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    geom = _native.conv_direct_dw_geometry(desc_of(TILES), cus)
    assert geom["tile1"] < au.out_spatial(TILES)[1]


@pytest.mark.parametrize("c,code", DX, ids=ids)
def test_direct_dw_dx_is_the_truth_bit_for_bit(c, code, monkeypatch):
    assert_whole_in_float32(c, "centred", c.cout // c.g)
    dtype = DTYPES[code]
    x, w, b = au.inputs(c, "centred")
    gy = au.grad_output((c.B, c.cout) + au.out_spatial(c), torch.float32)
    want = au.truth_grads(c, x, w, b, gy, only_dx=True)[0]
    monkeypatch.setenv(KNOB, "1")
    xr, w, gy = x.to(DEV, dtype).requires_grad_(), w.to(DEV, dtype), gy.to(DEV, dtype)
    assert autograd.dx_route(xr, tuple(w.shape), *conf(c)) == "direct-dw"
    call(c, xr, w, None).backward(gy)
    assert xr.grad.dtype == dtype and torch.equal(xr.grad.cpu(), want.to(dtype))


def test_a_strided_dx_keeps_its_plan_and_its_bits(monkeypatch):
    c = STRIDED
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


def test_the_other_switches_name_todays_routes(monkeypatch):
    x, w, _ = au.inputs(DEPTHWISE, "centred", DEV)
    for knob in (None, "FFTCONV_DIRECT"):
        if knob:
            monkeypatch.setenv(knob, "1")
        assert route(DEPTHWISE, x, w) == "fft" and autograd.dx_route(x, tuple(w.shape), *conf(DEPTHWISE)) == "plan"


@pytest.mark.parametrize("c,code,kw", [(FIRST, 0, {}), (MULT_9, 0, {}), (DEPTHWISE, 1, {}), (DEPTHWISE, 0, {"channels_last": True})],
                         ids=["dense", "multiplier-9", "float64", "channels-last"])
def test_a_refused_call_keeps_its_route_and_its_bits(c, code, kw, monkeypatch):
    x, w, b = (t.to(DTYPES[code]) for t in au.inputs(c, "centred", DEV))
    before = call(c, x, w, b, **kw)
    monkeypatch.setenv(KNOB, "1")
    assert route(c, x, w, **kw) == "fft"
    after = call(c, x, w, b, **kw)
    assert after.stride() == before.stride() and torch.equal(after, before)


def test_only_the_bytes_of_y_are_written_and_y_is_not_read():
    c = DEPTHWISE
    assert_whole_in_float32(c, "offset", 1)
    x, w, b = au.inputs(c, "offset")
    want = au.truth(c, x, w, b)
    x, w, b = (t.to(DEV) for t in (x, w, b))
    n, guard = want.numel(), 1003      # (an odd guard: y starts off a 16-byte boundary)
    for fill in (float("nan"), 0.0):
        buf = torch.full((n + 2 * guard,), fill, device=DEV)
        with torch.cuda.device(DEV):
            _native.conv_direct_dw(desc_of(c), x.data_ptr(), w.data_ptr(), b.data_ptr(), buf[guard:].data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(buf[guard:guard + n].view(want.shape).double().cpu(), want)
        sides = torch.cat((buf[:guard], buf[guard + n:]))
        assert bool(sides.isnan().all()) if fill != fill else bool((sides == 0).all())


def test_accuracy_of_a_long_reduction(monkeypatch):
    """B2, 8 channels x multiplier 8, 16^2 k11 'same': 121 terms per output sample and 968 per sample of dX, against float64
    conv2d and its autograd and the float32 rfftn baseline at the default margins (measured figures: DESIGN 4.5e)."""
    c = Case(2, 8, 64, (16, 16), (11, 11), p=5, g=8)
    gen = torch.Generator().manual_seed(5)
    x, w, b, gy = (torch.randn(s, generator=gen).to(DEV) for s in ((2, 8, 16, 16), (64, 1, 11, 11), (64,), (2, 64, 16, 16)))
    xd, wd = x.double().requires_grad_(), w.double()
    yd = torch.nn.functional.conv2d(xd, wd, b.double(), padding=5, groups=8)
    yd.backward(gy.double())
    base_y, base_dx = au.baseline_grads(c, x, w, b, gy, only_dx=True)[:2]
    monkeypatch.setenv(KNOB, "1")
    xr = x.clone().requires_grad_()
    assert route(c, xr, w) == "direct-dw" and autograd.dx_route(xr, tuple(w.shape), *conf(c)) == "direct-dw"
    y = call(c, xr, w, b)
    y.backward(gy)
    au.check("direct-dw y", y.detach(), yd.detach(), base_y, torch.float32, rms_margin=au.RMS_MARGIN)
    au.check("direct-dw dX", xr.grad, xd.grad, base_dx, torch.float32, rms_margin=au.RMS_MARGIN)
