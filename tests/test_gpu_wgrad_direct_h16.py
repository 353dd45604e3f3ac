"""The 16-bit MFMA body of the direct weight gradient (csrc/wgrad_direct_h16.hpp) under FFTCONV_WGRAD_DIRECT=1
FFTCONV_WGRAD_DIRECT_BODY=h16.

A product of two bfloat16 or two float16 values is exact in float32, so with the integers of tests/accuracy_util.py and
(terms per dW element) x max|x| x 8 < 2**24 every float32 partial sum is a whole number and dW must be float64 autograd's
dW, bit for bit, whatever the order of summation; each test asserts the condition first.  Random data: DESIGN 4.5g."""
import pytest
import torch

from fft_conv_pytorch_amd import _native, autograd
from tests import accuracy_util as au
from tests.route_util import Case
from tests.test_gpu_wgrad_direct import DEV, DTYPES, assert_whole_in_float32, public_dw
from tests.test_gpu_wgrad_direct_dw import body_of
from tests.test_host_wgrad_direct import FIRST, KNOBS, desc_of
from tests.test_host_wgrad_direct_dw import BODY, FIRST as DW_FIRST, ident
from tests.test_host_wgrad_direct_h16 import CASES, TWO_IN_BLOCKS

pytestmark = pytest.mark.gpu
CODES = {v: k for k, v in DTYPES.items()}


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for k in KNOBS + (BODY,):
        monkeypatch.delenv(k, raising=False)
    autograd._BWD_PLANS.clear()
    yield
    autograd._BWD_PLANS.clear()


def both(monkeypatch):
    monkeypatch.setenv("FFTCONV_WGRAD_DIRECT", "1")
    monkeypatch.setenv(BODY, "h16")


def operands(c, cls, dtype):
    """(x, w, dY on the device in ``dtype``, the float64 truth of dW); the integers survive the cast."""
    x, w, b = au.inputs(c, cls)
    gy = au.grad_output((c.B, c.cout) + au.out_spatial(c), torch.float32)
    assert all(torch.equal(t.to(dtype).to(t.dtype), t) for t in (x, w, gy))
    return x.to(DEV, dtype), w.to(DEV, dtype), gy.to(DEV, dtype), au.truth_grads(c, x, w, b, gy)[1]


def native_dw(c, dtype, x, gy, fill=float("nan"), edge=100):
    """float32 dW straight from ``fc_wgrad_direct`` inside ``edge`` guard elements, the workspace filled with ``fill``."""
    desc, n = desc_of(c, CODES[dtype]), torch.Size(c.wshape).numel()
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    assert _native.wgrad_direct_body(desc, cus) == "h16"
    ws = torch.full((_native.wgrad_direct_geometry(desc, cus)["workspace_bytes"] // 4,), fill, device=DEV)
    buf = torch.full((n + 2 * edge,), fill, device=DEV)
    before = buf.view(torch.int32).clone()
    with torch.cuda.device(DEV):
        _native.wgrad_direct(desc, x.data_ptr(), gy.data_ptr(), buf[edge:].data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    after = buf.view(torch.int32)
    assert torch.equal(after[:edge], before[:edge]) and torch.equal(after[-edge:], before[-edge:])
    return buf[edge:edge + n].reshape(c.wshape).clone()


@pytest.mark.parametrize("c,code,cls,slices", [(c, code, cls, None) for c in CASES for code, cls in ((3, "centred"), (3, "offset"), (2, "centred"))]
                         + [(FIRST, 3, "offset", 3)], ids=ident)
def test_h16_dw_is_the_truth_bit_for_bit(c, code, cls, slices, monkeypatch):
    assert_whole_in_float32(c, cls)
    both(monkeypatch)
    if slices:
        monkeypatch.setenv("FFTCONV_WGRAD_DIRECT_SLICES", str(slices))
    x, w, gy, want = operands(c, cls, DTYPES[code])
    if c is TWO_IN_BLOCKS:
        geom = autograd._wgrad_direct_geometry(x, tuple(w.shape), c.tup(c.s), c.tup(c.p), c.tup(c.d), c.g, c.mode)[1]
        assert geom["in_block"] < c.cin // c.g
    got, route = public_dw(c, x, w, gy)
    assert route == "direct" and body_of(c, x, w, gy) == "h16"
    # (the 16-bit weight receives the float32 dW rounded once: the truth, a whole number below 2**24, rounded the same way)
    assert got.dtype == w.dtype and torch.equal(got.cpu(), want.to(w.dtype))


def test_a_dead_position_of_a_rounded_up_run_contributes_nothing(monkeypatch):
    """FIRST has 19 outputs along x: the run 16..23 has 5 dead positions.  An inf at x index 18 (padded 19) meets live
    positions through taps kx = 1, 2 only; position 19, dead, would read it through kx = 0."""
    c = FIRST
    assert_whole_in_float32(c, "centred")
    both(monkeypatch)
    x, w, gy, _ = operands(c, "centred", torch.bfloat16)
    x[1, 3, 4, 5, 18] = float("inf")
    wd = w.double().cpu().requires_grad_()
    torch.nn.functional.conv3d(x.double().cpu(), wd, None, padding=1).backward(gy.double().cpu())
    got = native_dw(c, torch.bfloat16, x, gy).double().cpu()
    fin = torch.isfinite(wd.grad)
    assert not bool(fin.all()) and bool(fin[..., 0].all())
    assert torch.equal(torch.isfinite(got), fin) and torch.equal(got[fin], wd.grad[fin])


def test_bits_depend_on_neither_the_workspace_nor_the_guards(monkeypatch):
    c = FIRST
    assert_whole_in_float32(c, "offset")
    both(monkeypatch)
    x, w, gy, want = operands(c, "offset", torch.bfloat16)
    nan, zero = (native_dw(c, torch.bfloat16, x, gy, fill) for fill in (float("nan"), 0.0))
    assert torch.equal(nan.view(torch.int32), zero.view(torch.int32)) and torch.equal(nan.double().cpu(), want)


@pytest.mark.parametrize("code", [3, 2], ids=ident)
def test_accuracy_of_a_long_reduction_in_random_data(code, monkeypatch):
    """B2 2 -> 2 64^3 k3 'same': 524,288 exact products per element of dW summed in float32 in three levels, against
    float64 autograd on the same 16-bit values and the float32 rfftn baseline, default margins."""
    c, dtype = Case(2, 2, 2, (64, 64, 64), (3, 3, 3), p=1), DTYPES[code]
    gen = torch.Generator().manual_seed(5)
    x, w, gy = (torch.randn(s, generator=gen).to(DEV, dtype) for s in ((2, 2, 64, 64, 64), (2, 2, 3, 3, 3), (2, 2, 64, 64, 64)))
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    torch.nn.functional.conv3d(xr, wr, None, padding=1).backward(gy.double())
    base = au.baseline_grads(c, x.float(), w.float(), torch.zeros(2, device=DEV), gy.float())[2]
    both(monkeypatch)
    au.check(f"h16 dW {dtype}", native_dw(c, dtype, x, gy), wr.grad, base, torch.float32)


@pytest.mark.parametrize("c,code,on,body", [(FIRST, 0, "1", "mfma"), (DW_FIRST, 3, "1", "valu"), (FIRST, 3, None, None)],
                         ids=["float32", "depthwise", "switch-unset"])
def test_every_other_call_keeps_its_route_and_its_bits(c, code, on, body, monkeypatch):
    x, w, gy, _ = operands(c, "centred", DTYPES[code])
    if on:
        monkeypatch.setenv("FFTCONV_WGRAD_DIRECT", on)
    before, route_before = public_dw(c, x, w, gy)
    assert body_of(c, x, w, gy) == body
    monkeypatch.setenv(BODY, "h16")
    autograd._BWD_PLANS.clear()
    after, route_after = public_dw(c, x, w, gy)
    assert route_after == route_before and body_of(c, x, w, gy) == body and torch.equal(after, before)
