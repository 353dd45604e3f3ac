"""The direct forward and input gradient on the 16-bit matrix instructions (``fc_conv_direct_h16``,
csrc/conv_direct_h16.hpp) under FFTCONV_DIRECT=1 FFTCONV_DIRECT_BODY=h16.

A product of two bfloat16 or two float16 values is exact in float32, so wherever every float32 partial sum is exact too
the route must return the float64 truth rounded once to the tensors' dtype, bit for bit; each test asserts that condition
for its inputs first.  Random data: DESIGN 4.5f has the measured figures."""
import math

import pytest
import torch

from fft_conv_pytorch_amd import _native, autograd
from tests import accuracy_util as au
from tests.route_util import Case
from tests.test_gpu_conv_direct import DEV, DTYPES, assert_whole_in_float32, call, conf, ids, route
from tests.test_host_conv_direct import DEPTHWISE, DX, FIRST, FORWARD, KNOB, TRANSPOSED, desc_of
from tests.test_host_conv_direct_h16 import TWO_IN_BLOCKS_H16

pytestmark = pytest.mark.gpu
BODY = "FFTCONV_DIRECT_BODY"
CASES = list({c.ident(): c for c, _ in FORWARD}.values()) + [TRANSPOSED, TWO_IN_BLOCKS_H16]


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for name in (KNOB, BODY, "FFTCONV_DIRECT_DW", "FFTCONV_HALF_IO"):
        monkeypatch.delenv(name, raising=False)


def both(monkeypatch):
    monkeypatch.setenv(KNOB, "1")
    monkeypatch.setenv(BODY, "h16")


# (float16: the centred class only, so that |y| stays below 65,504)
@pytest.mark.parametrize("c,code,cls", [(c, code, cls) for c in CASES for code, cls in ((3, "centred"), (3, "offset"), (2, "centred"))],
                         ids=ids)
def test_h16_forward_is_the_truth_rounded_once(c, code, cls, monkeypatch):
    assert_whole_in_float32(c, cls, c.cin // c.g)
    dtype = DTYPES[code]
    x, w, b = au.inputs(c, cls)
    want = au.truth(c, x, w, b)
    assert code != 2 or want.abs().max() < 65504
    both(monkeypatch)
    x, w, b = (t.to(DEV, dtype) for t in (x, w, b))
    assert route(c, x, w) == "direct-h16"
    got = call(c, x, w, b)
    assert got.dtype == dtype and torch.equal(got.cpu(), want.to(dtype))


@pytest.mark.parametrize("code", [3, 2], ids=ids)
@pytest.mark.parametrize("c", [c for c, _ in DX[1:]], ids=ids)
def test_h16_dx_is_the_truth_rounded_once(c, code, monkeypatch):
    assert_whole_in_float32(c, "centred", c.cout // c.g)
    dtype = DTYPES[code]
    x, w, b = au.inputs(c, "centred")
    gy = au.grad_output((c.B, c.cout) + au.out_spatial(c), torch.float32)
    want = au.truth_grads(c, x, w, b, gy, only_dx=True)[0]
    assert want.abs().max() < 65504
    both(monkeypatch)
    xr, w, gy = x.to(DEV, dtype).requires_grad_(), w.to(DEV, dtype), gy.to(DEV, dtype)
    assert autograd.dx_route(xr, tuple(w.shape), *conf(c)) == "direct-h16"
    call(c, xr, w, None).backward(gy)
    assert xr.grad.dtype == dtype and torch.equal(xr.grad.cpu(), want.to(dtype))


odd = lambda shape, gen: (2 * torch.randint(-128, 128, shape, generator=gen) + 1).double()      # noqa: E731
whole = lambda shape, gen, top: torch.randint(-top, top + 1, shape, generator=gen).double()      # noqa: E731
# (dtype code, x, w, the largest |partial sum| in units of the smallest product, which must stay below 2**24)
FULL = {
    "bfloat16-odd-255": (3, odd, odd, 216 * 255 * 255),
    "float16-2047-over-2048": (2, lambda s, g: whole(s, g, 2047) * 2.0 ** -11, lambda s, g: whole(s, g, 8), 216 * 2047 * 8),
    "float16-subnormal-x": (2, lambda s, g: whole(s, g, 8) * 2.0 ** -24, lambda s, g: whole(s, g, 8) * 2.0 ** 10, 216 * 8 * 8),
}


@pytest.mark.parametrize("name", FULL)
def test_full_mantissas_are_the_truth_rounded_once(name, monkeypatch):
    c, (code, draw_x, draw_w, units) = FIRST, FULL[name]
    assert math.prod(c.k) * c.cin // c.g == 216 and units < 2 ** 24      # every partial sum is exact in float32
    gen = torch.Generator().manual_seed(11)
    x, w = draw_x((c.B, c.cin) + c.size, gen), draw_w(c.wshape, gen)
    dtype = DTYPES[code]
    assert torch.equal(x.to(dtype).double(), x) and torch.equal(w.to(dtype).double(), w)
    want = au.direct(c, x, w, None)
    both(monkeypatch)
    x, w = x.to(DEV, dtype), w.to(DEV, dtype)
    assert route(c, x, w) == "direct-h16"
    assert torch.equal(call(c, x, w, None).cpu(), want.to(dtype))


@pytest.mark.parametrize("code", [3, 2], ids=ids)
def test_accuracy_of_a_long_reduction_in_random_data(code, monkeypatch):
    """B2 64 -> 8 16^3 k3 'same': 1,728 terms per output in two chains of 864.  At every sample
    |got - want| <= ulp16(want) / 2 + MAX_MARGIN * max|base - want|, base the float32 rfftn baseline on the same values."""
    c, dtype, bits = Case(2, 64, 8, (16, 16, 16), (3, 3, 3), p=1), DTYPES[code], 7 if code == 3 else 10
    gen = torch.Generator().manual_seed(5)
    x, w, b, gy = (torch.randn(s, generator=gen).to(DEV, dtype) for s in ((2, 64, 16, 16, 16), (8, 64, 3, 3, 3), (8,), (2, 8, 16, 16, 16)))
    xd = x.double().requires_grad_()
    yd = torch.nn.functional.conv3d(xd, w.double(), b.double(), padding=1)
    yd.backward(gy.double())
    base_y, base_dx = au.baseline_grads(c, x.float(), w.float(), b.float(), gy.float(), only_dx=True)[:2]
    both(monkeypatch)
    xr = x.clone().requires_grad_()
    assert route(c, xr, w) == "direct-h16" and autograd.dx_route(xr, tuple(w.shape), *conf(c)) == "direct-h16"
    y = call(c, xr, w, b)
    y.backward(gy)
    for what, got, want, base in (("y", y.detach(), yd.detach(), base_y), ("dX", xr.grad, xd.grad, base_dx)):
        allowed = 0.5 * torch.exp2(torch.floor(torch.log2(want.abs())) - bits) + au.MAX_MARGIN * (base.double() - want).abs().max()
        err = (got.double() - want).abs()
        print(f"    h16 {what} {dtype}: max(|got - want| / allowance) {(err / allowed).max().item():.3f}")
        assert bool((err <= allowed).all())


def test_every_output_byte_is_written_and_nothing_else():
    c, edge = FIRST, 100
    assert_whole_in_float32(c, "offset", c.cin // c.g)
    x, w, b = au.inputs(c, "offset")
    want = au.truth(c, x, w, b).to(torch.bfloat16)
    x, w, b = (t.to(DEV, torch.bfloat16) for t in (x, w, b))
    results = []
    for fill in (float("nan"), 0.0):
        buf = torch.full((want.numel() + 2 * edge,), fill, device=DEV, dtype=torch.bfloat16)
        before = buf.view(torch.int16).clone()
        y = buf[edge:edge + want.numel()]
        with torch.cuda.device(DEV):
            _native.conv_direct_h16(desc_of(c, 3), x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        after = buf.view(torch.int16)
        assert torch.equal(after[:edge], before[:edge]) and torch.equal(after[-edge:], before[-edge:])
        results.append(y.reshape(want.shape).cpu())
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], want)


@pytest.mark.parametrize("c,code,kw,name", [(FIRST, 0, {}, "direct"), (DEPTHWISE, 3, {}, "fft"),
                                            (FIRST, 3, {"channels_last": True}, "fft")], ids=["float32", "depthwise", "channels-last"])
def test_every_other_call_keeps_its_route_and_its_bits(c, code, kw, name, monkeypatch):
    x, w, b = (t.to(DTYPES[code]) for t in au.inputs(c, "centred", DEV))
    monkeypatch.setenv(KNOB, "1")
    assert route(c, x, w, **kw) == name
    before = call(c, x, w, b, **kw)
    monkeypatch.setenv(BODY, "h16")
    assert route(c, x, w, **kw) == name
    after = call(c, x, w, b, **kw)
    assert after.stride() == before.stride() and torch.equal(after, before)


def test_the_body_alone_switches_nothing(monkeypatch):
    x, w, b = (t.to(torch.bfloat16) for t in au.inputs(FIRST, "centred", DEV))
    before = call(FIRST, x, w, b)
    monkeypatch.setenv(BODY, "h16")
    assert route(FIRST, x, w) == "fft" and autograd.dx_route(x, tuple(w.shape), *conf(FIRST)) == "plan"
    assert torch.equal(call(FIRST, x, w, b), before)
