"""The direct strided transposed convolution on the 16-bit matrix instructions (``fc_conv_direct_tr_h16``,
csrc/conv_direct_tr_h16.hpp) under FFTCONV_DIRECT_TR=1 FFTCONV_DIRECT_BODY=h16.

A product of two bfloat16 or two float16 values is exact in float32, so wherever every float32 partial sum is exact too
the route must return the float64 truth rounded once to the tensors' dtype, bit for bit; each test asserts that condition
for its inputs first.  Random data: DESIGN 4.5i has the measured figures."""
import pytest
import torch

from fft_conv_pytorch_amd import _native, autograd
from tests import accuracy_util as au
from tests.route_util import Case
from tests.test_gpu_conv_direct import DEV, DTYPES, assert_whole_in_float32, call, conf, ids, route
from tests.test_host_conv_direct import CUS, desc_of
from tests.test_host_conv_direct_tr import DX, KNOB, NO_TAP, UNEVEN, T
from tests.test_host_conv_direct_tr_h16 import CASES, TWO_IN_BLOCKS

pytestmark = pytest.mark.gpu
BODY = "FFTCONV_DIRECT_BODY"
PAST_THE_KERNEL = next(c for c in CASES if c.note == "padding-past-the-kernel")


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for name in (KNOB, BODY, "FFTCONV_DIRECT", "FFTCONV_DIRECT_DW", "FFTCONV_WGRAD_DIRECT", "FFTCONV_HALF_IO"):
        monkeypatch.delenv(name, raising=False)


def both(monkeypatch):
    monkeypatch.setenv(KNOB, "1")
    monkeypatch.setenv(BODY, "h16")


# (float16: every case, in the centred class only: there |y| stays below 65,504, which the test asserts)
@pytest.mark.parametrize("c,code,cls", [(c, code, cls) for c in CASES for code, cls in ((3, "centred"), (3, "offset"), (2, "centred"))],
                         ids=ids)
def test_forward_is_the_truth_rounded_once(c, code, cls, monkeypatch):
    assert_whole_in_float32(c, cls, c.cin // c.g)
    dtype = DTYPES[code]
    x, w, b = au.inputs(c, cls)
    want = au.truth(c, x, w, b)
    assert code != 2 or want.abs().max() < 65504
    assert c is not TWO_IN_BLOCKS or _native.conv_direct_tr_h16_geometry(desc_of(c, code), CUS)["in_blocks"] >= 2
    both(monkeypatch)
    x, w, b = (t.to(DEV, dtype) for t in (x, w, b))
    assert route(c, x, w) == "direct-tr-h16"
    got = call(c, x, w, b)
    assert got.dtype == dtype and torch.equal(got.cpu(), want.to(dtype))


@pytest.mark.parametrize("code", [3, 2], ids=ids)
@pytest.mark.parametrize("c", list({c.ident(): c for c, _ in DX}.values()), ids=ids)
def test_dx_of_a_strided_layer_is_the_truth_rounded_once(c, code, monkeypatch):
    assert_whole_in_float32(c, "centred", c.cout // c.g)
    dtype = DTYPES[code]
    x, w, b = au.inputs(c, "centred")
    gy = au.grad_output((c.B, c.cout) + au.out_spatial(c), torch.float32)
    want = au.truth_grads(c, x, w, b, gy, only_dx=True)[0]
    assert want.abs().max() < 65504
    both(monkeypatch)
    xr, w, gy = x.to(DEV, dtype).requires_grad_(), w.to(DEV, dtype), gy.to(DEV, dtype)
    assert autograd.dx_route(xr, tuple(w.shape), *conf(c)) == "direct-tr-h16"
    call(c, xr, w, None).backward(gy)
    assert xr.grad.dtype == dtype and torch.equal(xr.grad.cpu(), want.to(dtype))


def test_every_output_byte_is_written_and_nothing_else():
    c, edge = NO_TAP, 100      # (three phases in four have no tap: their outputs are the bias)
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
            _native.conv_direct_tr_h16(desc_of(c, 3), x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        after = buf.view(torch.int16)
        assert torch.equal(after[:edge], before[:edge]) and torch.equal(after[-edge:], before[-edge:])
        results.append(y.reshape(want.shape).cpu())
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], want)


def test_a_dead_position_or_column_never_multiplies(monkeypatch):
    """k3 s2 p3: x[.., 0, 0] reaches t = k - 3 < 0 only, so no output depends on it, yet it is the first cell of the
    first tile's halo, the one a dead column's or position's clamped read lands on: an Inf there must change no bit."""
    c = PAST_THE_KERNEL
    x, w, b = (t.to(DEV, torch.bfloat16) for t in au.inputs(c, "centred"))
    both(monkeypatch)
    want = call(c, x, w, b)
    x[:, :, 0, 0] = float("inf")
    assert route(c, x, w) == "direct-tr-h16"
    got = call(c, x, w, b)
    assert not got.isnan().any() and torch.equal(got, want)


@pytest.mark.parametrize("c,code,name", [(UNEVEN, 0, "direct-tr"), (T(2, 5, 5, (7, 9), (3, 3), s=2, p=1, g=5), 3, "fft")],
                         ids=["float32", "depthwise"])
def test_every_other_call_keeps_its_route_and_its_bits(c, code, name, monkeypatch):
    x, w, b = (t.to(DTYPES[code]) for t in au.inputs(c, "centred", DEV))
    monkeypatch.setenv(KNOB, "1")
    assert route(c, x, w) == name
    before = call(c, x, w, b)
    monkeypatch.setenv(BODY, "h16")
    assert route(c, x, w) == name
    after = call(c, x, w, b)
    assert after.stride() == before.stride() and torch.equal(after, before)


def test_the_body_alone_switches_nothing(monkeypatch):
    x, w, b = (t.to(torch.bfloat16) for t in au.inputs(UNEVEN, "centred", DEV))
    before = call(UNEVEN, x, w, b)
    monkeypatch.setenv(BODY, "h16")
    assert route(UNEVEN, x, w) == "fft"
    assert torch.equal(call(UNEVEN, x, w, b), before)


@pytest.mark.parametrize("code", [3, 2], ids=ids)
def test_accuracy_of_a_long_reduction_in_random_data(code, monkeypatch):
    """B2 64 -> 8 8^3 k3 s2 p1 op1 transposed (up to 8 taps x 64 channels per output) and the dX of the strided layer
    B2 8 -> 64 16^3 k3 s2 p1, the same transposed convolution through autograd.  At every sample
    |got - want| <= ulp16(want) / 2 + MAX_MARGIN * max|base - want|, base the float32 rfftn baseline on the same values."""
    c, layer = T(2, 64, 8, (8, 8, 8), (3, 3, 3), s=2, p=1, op=1), Case(2, 8, 64, (16, 16, 16), (3, 3, 3), s=2, p=1)
    dtype, bits = DTYPES[code], 7 if code == 3 else 10
    gen = torch.Generator().manual_seed(5)
    x, w, b, xl = (torch.randn(s, generator=gen).to(DEV, dtype) for s in ((2, 64, 8, 8, 8), (64, 8, 3, 3, 3), (8,), (2, 8, 16, 16, 16)))
    yd = torch.nn.functional.conv_transpose3d(x.double(), w.double(), b.double(), stride=2, padding=1, output_padding=1)
    xd = xl.double().requires_grad_()
    torch.nn.functional.conv3d(xd, w.double(), None, stride=2, padding=1).backward(x.double())
    base_y = au.baseline(c, x.float(), w.float(), b.float())
    base_dx = au.baseline_grads(layer, xl.float(), w.float(), torch.zeros(64, device=DEV), x.float(), only_dx=True)[1]
    both(monkeypatch)
    xr = xl.clone().requires_grad_()
    assert route(c, x, w) == "direct-tr-h16" and autograd.dx_route(xr, tuple(w.shape), *conf(layer)) == "direct-tr-h16"
    y = call(c, x, w, b)
    call(layer, xr, w, None).backward(x)
    for what, got, want, base in (("y", y, yd, base_y), ("dX", xr.grad, xd.grad, base_dx)):
        allowed = 0.5 * torch.exp2(torch.floor(torch.log2(want.abs())) - bits) + au.MAX_MARGIN * (base.double() - want).abs().max()
        err = (got.double() - want).abs()
        print(f"    tr-h16 {what} {dtype}: max(|got - want| / allowance) {(err / allowed).max().item():.3f}")
        assert bool((err <= allowed).all())
