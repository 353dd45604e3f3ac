"""The depthwise body of the direct weight gradient (csrc/wgrad_direct_dw.hpp) under FFTCONV_WGRAD_DIRECT=1.

As in tests/test_gpu_wgrad_direct.py the inputs are the integers of tests/accuracy_util.py and every float32 partial sum
is a whole number below 2**24 (each test asserts the condition first), so dW must be float64 autograd's dW bit for bit
whatever the order of summation.  The long reduction of the last test is bounded against the float32 rfftn baseline."""
import pytest
import torch

from fft_conv_pytorch_amd import _native, autograd
from tests import accuracy_util as au
from tests.route_util import Case
from tests.test_gpu_wgrad_direct import DEV, DTYPES, assert_whole_in_float32, operands, public_dw
from tests.test_host_wgrad_direct import KNOBS, desc_of
from tests.test_host_wgrad_direct_dw import BODY, DEPTHWISE, FIRST, TRANSPOSED, ident

pytestmark = pytest.mark.gpu
ACCURACY_MARGIN = au.RMS_MARGIN       # the default: three levels of short sums need no margin of their own


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for k in KNOBS + (BODY,):
        monkeypatch.delenv(k, raising=False)
    autograd._BWD_PLANS.clear()
    yield
    autograd._BWD_PLANS.clear()


def body_of(c, x, w, gy):
    signal, mode = (gy, "constant") if c.tr else (x, c.mode)
    return autograd.dw_direct_body(signal, tuple(w.shape), c.tup(c.s), c.tup(c.p), c.tup(c.d), c.g, mode)


@pytest.mark.parametrize("cls", au.CLASSES)
@pytest.mark.parametrize("c,code,slices", DEPTHWISE + [(TRANSPOSED, 0, None)], ids=ident)
def test_depthwise_dw_is_the_truth_bit_for_bit(c, code, slices, cls, monkeypatch):
    assert_whole_in_float32(c, cls)
    monkeypatch.setenv("FFTCONV_WGRAD_DIRECT", "1")
    if slices:
        monkeypatch.setenv("FFTCONV_WGRAD_DIRECT_SLICES", str(slices))
    x, w, gy, want = operands(c, cls, DTYPES[code])
    got, route = public_dw(c, x, w, gy)
    assert route == "direct" and body_of(c, x, w, gy) == "valu"
    # (a 16-bit weight receives the float32 dW rounded once: the truth, a whole number below 2**24, rounded the same way)
    assert got.dtype == w.dtype and torch.equal(got.cpu(), want.to(w.dtype))


def test_both_bodies_give_one_layer_the_truth(monkeypatch):
    assert_whole_in_float32(FIRST, "offset")
    monkeypatch.setenv("FFTCONV_WGRAD_DIRECT", "1")
    x, w, gy, want = operands(FIRST, "offset", torch.float32)
    seen = {}
    for knob in ("mfma", "valu"):
        monkeypatch.setenv(BODY, knob)
        got, route = public_dw(FIRST, x, w, gy)
        assert route == "direct" and body_of(FIRST, x, w, gy) == knob
        seen[knob] = got.double().cpu()
    assert torch.equal(seen["mfma"], want) and torch.equal(seen["valu"], want)


def test_bits_do_not_depend_on_the_workspace():
    c = FIRST
    assert_whole_in_float32(c, "offset")
    x, w, gy, want = operands(c, "offset", torch.float32)
    desc = desc_of(c)
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    assert _native.wgrad_direct_body(desc, cus) == "valu"
    geom = _native.wgrad_direct_geometry(desc, cus)
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


def test_accuracy_of_a_long_depthwise_reduction(monkeypatch):
    """Depthwise B2 C2 64^3 k3 'same': 524,288 terms per element of dW in three levels (a lane's runs of one unit, the
    units of a slice and the 64 lanes, the slices in blocks of 16), against float64 autograd and the float32 rfftn
    baseline."""
    c = Case(2, 2, 2, (64, 64, 64), (3, 3, 3), p=1, g=2)
    gen = torch.Generator().manual_seed(5)
    x, w, gy = (torch.randn(s, generator=gen).to(DEV) for s in ((2, 2, 64, 64, 64), (2, 1, 3, 3, 3), (2, 2, 64, 64, 64)))
    b = torch.zeros(2, device=DEV)
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    torch.nn.functional.conv3d(xr, wr, None, padding=1, groups=2).backward(gy.double())
    base = au.baseline_grads(c, x, w, b, gy)[2]
    monkeypatch.setenv("FFTCONV_WGRAD_DIRECT", "1")
    got, route = public_dw(c, x, w, gy)
    assert route == "direct" and body_of(c, x, w, gy) == "valu"
    au.check("depthwise direct dW", got, wr.grad, base, torch.float32, rms_margin=ACCURACY_MARGIN)
