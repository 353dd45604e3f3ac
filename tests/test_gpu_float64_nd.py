"""float64 2-D / 3-D and transposed convolutions through FFTs (csrc/nd_f64.hip; 1-D transposed: csrc/fft_f64.hip),
the way the reference runs complex128 rfftn / irfftn on float64 tensors (functional.py:66-75, :155-162).  Every case
against torch's float64 convolution on the GPU at 1e-12 of the result's max magnitude; every shape past the planner's
crossover also asserts that its plan is on the FFT path (plan.tile > 0), not on the direct kernel.  Small shapes below
the crossover (axes of extent 1-5, few channels) run the FFT path under FFTCONV_F64_FFT=2, so that it is checked too."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12
CROSSOVER = 100      # direct-kernel multiply-adds per output (Cin/g x prod(k), / prod(stride) when forward): N-d plans take the FFT


@pytest.fixture
def fft_path(monkeypatch):
    """Call with (Cin/g, kernel extents, ndim, stride, transposed): below the crossover, N-d plans are made with FFTCONV_F64_FFT=2 (the FFT
    path at any size); the plan cache is emptied around each test (the knob is read at plan creation)."""
    from fft_conv_pytorch_amd import _native

    def set_for(cig, k, nd, stride, transposed=False):
        stride = (1,) * nd if transposed else (stride,) * nd if isinstance(stride, int) else tuple(stride)
        forced = nd > 1 and cig * math.prod(k) < CROSSOVER * math.prod(stride)
        if forced:
            monkeypatch.setenv("FFTCONV_F64_FFT", "2")
        else:
            monkeypatch.delenv("FFTCONV_F64_FFT", raising=False)
        _native.clear_plan_cache()
        return forced
    yield set_for
    monkeypatch.delenv("FFTCONV_F64_FFT", raising=False)
    _native.clear_plan_cache()


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _torch_conv(x, w, b, stride, padding, dilation, groups, mode):
    nd = x.ndim - 2
    conv = (F.conv1d, F.conv2d, F.conv3d)[nd - 1]
    pads = (padding,) * nd if isinstance(padding, int) else tuple(padding)
    if mode == "constant":
        return conv(x, w, b, stride=stride, padding=pads, dilation=dilation, groups=groups)
    flat = [q for p in reversed(pads) for q in (p, p)]
    return conv(F.pad(x, flat, mode=mode), w, b, stride=stride, dilation=dilation, groups=groups)


def _rand(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64).to(DEV)


FWD_CASES = [
    # x shape, w shape, stride, padding, dilation, groups, mode, bias
    ((2, 4, 37, 50), (6, 4, 5, 7), 1, (2, 3), 1, 1, "constant", True),
    ((1, 3, 33, 40), (5, 3, 3, 5), (1, 2), (2, 1), (2, 1), 1, "circular", True),
    ((3, 6, 29, 31), (9, 2, 4, 3), (2, 3), (3, 1), 1, 3, "reflect", False),            # groups, ragged, stride
    ((2, 8, 24, 26), (8, 1, 7, 5), 1, (3, 2), (1, 2), 8, "replicate", True),          # depthwise, dilation
    ((5, 5, 3, 5), (3, 5, 3, 4), 1, (1, 2), 1, 1, "constant", True),                  # axes of extent 3 and 5
    ((2, 8, 1, 2), (4, 8, 1, 2), 1, 0, 1, 1, "constant", True),                       # axes of extent 1 and 2
    ((1, 2, 8, 5000), (3, 2, 3, 65), 1, (1, 32), 1, 1, "constant", True),             # overlap-save tiles along x
    ((1, 1, 40, 1500), (2, 1, 3, 513), 1, 0, (1, 2), 1, "constant", False),           # dilated extent 1025 along x
    ((1, 2, 3000, 9), (2, 2, 40, 3), (3, 1), (5, 1), 1, 1, "reflect", True),          # overlap-save tiles along y
    ((2, 3, 12, 14, 16), (4, 3, 3, 3, 3), 1, 1, 1, 1, "constant", True),
    ((1, 4, 11, 9, 13), (6, 2, 2, 3, 4), (2, 1, 3), (1, 1, 2), (2, 1, 1), 2, "reflect", True),
    ((3, 2, 10, 12, 9), (2, 2, 3, 2, 3), (1, 2, 1), (2, 1, 1), 1, 1, "circular", False),
    ((2, 3, 7, 10, 8), (5, 3, 2, 3, 2), 1, (1, 1, 1), (1, 2, 1), 1, "replicate", True),
    ((2, 6, 9, 8, 7), (6, 1, 3, 3, 3), 1, 1, 1, 6, "constant", True),                 # depthwise 3-D
    ((1, 1, 5, 4, 200), (1, 1, 2, 2, 9), 1, 0, (1, 1, 20), 1, "constant", True),      # extent 4 / 5 axes, long dilated x
    ((2, 2, 300, 5, 4), (3, 2, 17, 2, 2), (2, 1, 1), (8, 0, 1), 1, 1, "constant", True),   # 3-D, tiles along z
    ((1, 1, 2500, 10), (1, 1, 513, 3), 1, 0, (2, 1), 1, "constant", True),          # dilated extent 1025 past 2048
    ((1, 1, 10, 2500), (2, 1, 3, 513), 1, (1, 0), (1, 2), 1, "constant", True),     # samples: 2048-point tiles
    ((1, 1, 6, 2300), (1, 1, 3, 1025), (1, 2), 0, 1, 1, "reflect", False),
]


@pytest.mark.parametrize("case", FWD_CASES, ids=[f"{len(c[0]) - 2}d-{'x'.join(map(str, c[0][2:]))}-k{'x'.join(map(str, c[1][2:]))}-{c[6]}"
                                                  for c in FWD_CASES])
def test_float64_nd_forward_matches_torch(case, fft_path):
    from fft_conv_pytorch_amd.functional import _plan_for, fft_conv
    xs, ws, s, p, d, g, mode, has_b = case
    fft_path(xs[1] // g, ws[2:], len(xs) - 2, s)
    gen = torch.Generator().manual_seed(sum(xs) + sum(ws))
    x, w = _rand(gen, *xs), _rand(gen, *ws)
    b = _rand(gen, ws[0]) if has_b else None
    got = fft_conv(x, w, b, stride=s, padding=p, dilation=d, groups=g, padding_mode=mode)
    plan = _plan_for(x, w, b, s, p, d, g, mode)
    assert plan.tile > 0, ("expected the FFT path", case)
    want = _torch_conv(x, w, b, s, p, d, g, mode)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert _rel(got, want) < TOL, (case, _rel(got, want))


TR_CASES = [
    # x shape, w shape (Cin, Cout/g, *k), stride, padding, output_padding, dilation, groups, bias
    ((2, 4, 300), (4, 3, 33), 2, 5, 1, 1, 1, True),
    ((1, 6, 200), (6, 2, 17), 3, 4, 4, 5, 2, True),                               # output_padding >= stride (dilation 5)
    ((2, 4, 9, 11), (4, 3, 3, 4), (2, 3), (1, 2), (2, 1), (3, 1), 2, True),
    ((1, 8, 16, 16), (8, 4, 4, 4), 2, 1, 0, 1, 1, False),                         # stride-2 decoder layer
    ((2, 3, 5, 6, 7), (3, 4, 3, 2, 3), (2, 1, 2), (1, 0, 2), (1, 0, 3), (1, 2, 4), 1, True),
    ((1, 4, 4, 5, 6), (4, 1, 2, 3, 3), 1, (0, 1, 1), 0, 1, 4, True),
]


@pytest.mark.parametrize("case", TR_CASES, ids=[f"{len(c[0]) - 2}d-{'x'.join(map(str, c[0][2:]))}-k{'x'.join(map(str, c[1][2:]))}"
                                                 for c in TR_CASES])
def test_float64_transposed_matches_torch(case, fft_path):
    from fft_conv_pytorch_amd.functional import _plan_for, fft_conv_transpose
    xs, ws, s, p, op, d, g, has_b = case
    nd = len(xs) - 2
    fft_path(xs[1] // g, ws[2:], nd, s, transposed=True)
    gen = torch.Generator().manual_seed(7 * sum(xs) + sum(ws))
    x, w = _rand(gen, *xs), _rand(gen, *ws)
    b = _rand(gen, ws[1] * g) if has_b else None
    got = fft_conv_transpose(x, w, b, stride=s, padding=p, output_padding=op, dilation=d, groups=g)
    plan = _plan_for(x, w, b, s, p, d, g, "constant", transposed=True, output_padding=op)
    assert plan.tile > 0, ("expected the FFT path", case)
    want = (F.conv_transpose1d, F.conv_transpose2d, F.conv_transpose3d)[nd - 1](
        x, w, b, stride=s, padding=p, output_padding=op, dilation=d, groups=g)
    assert got.shape == want.shape
    assert _rel(got, want) < TOL, (case, _rel(got, want))


def _grad_input_plan(layer, x):
    """The transposed plan autograd runs for dX of this layer (autograd._grad_input builds the same descriptor)."""
    from fft_conv_pytorch_amd.functional import _plan_for
    n = x.ndim - 2
    gy_shape = layer(x).shape
    gy = torch.zeros(gy_shape, device=DEV, dtype=torch.float64)
    mode = "constant" if layer.padding_mode == "zeros" else layer.padding_mode
    pad = layer.padding if mode == "constant" else (0,) * n
    full = tuple(s + 2 * (p if mode != "constant" else 0) for s, p in zip(x.shape[2:], layer.padding))
    out_pad = tuple(full[i] - ((gy_shape[2 + i] - 1) * layer.stride[i] - 2 * pad[i] +
                               layer.dilation[i] * (layer.weight.shape[2 + i] - 1) + 1) for i in range(n))
    return _plan_for(gy, layer.weight, None, layer.stride, pad, layer.dilation, layer.groups, "constant",
                     transposed=True, output_padding=out_pad)


@pytest.mark.parametrize("nd", [2, 3])
def test_float64_module_gradients_match_autograd(nd):
    from fft_conv_pytorch_amd import FFTConv2d, FFTConv3d
    torch.manual_seed(11 + nd)
    if nd == 2:
        layer = FFTConv2d(16, 12, (5, 7), stride=(2, 1), padding=(2, 3), dilation=(1, 2), groups=2, bias=True,
                          padding_mode="reflect")
        x = torch.randn(3, 16, 30, 34, dtype=torch.float64, device=DEV)
    else:
        layer = FFTConv3d(4, 4, 3, padding=1, bias=True)
        x = torch.randn(2, 4, 10, 12, 9, dtype=torch.float64, device=DEV)
    layer = layer.to(DEV).double()
    x.requires_grad_()
    y = layer(x)
    gy = torch.randn(y.shape, dtype=torch.float64, device=DEV)
    y.backward(gy)
    xr = x.detach().clone().requires_grad_()
    wr = layer.weight.detach().clone().requires_grad_()
    br = layer.bias.detach().clone().requires_grad_()
    mode = "constant" if layer.padding_mode == "zeros" else layer.padding_mode
    want = _torch_conv(xr, wr, br, layer.stride, layer.padding, layer.dilation, layer.groups, mode)
    want.backward(gy)
    assert _rel(y, want) < TOL
    for name, a_, b_ in (("dX", x.grad, xr.grad), ("dW", layer.weight.grad, wr.grad), ("db", layer.bias.grad, br.grad)):
        assert _rel(a_, b_) < TOL, (name, _rel(a_, b_))
    assert _grad_input_plan(layer, x.detach()).tile > 0          # dX ran on the FFT path


def test_float64_transposed_module_gradients_match_autograd():
    from fft_conv_pytorch_amd import FFTConvTranspose2d
    torch.manual_seed(5)
    layer = FFTConvTranspose2d(40, 4, (4, 3), stride=2, padding=1, output_padding=1, bias=True).to(DEV).double()
    x = torch.randn(2, 40, 13, 15, dtype=torch.float64, device=DEV, requires_grad=True)
    y = layer(x)
    from fft_conv_pytorch_amd.functional import _plan_for
    assert _plan_for(x, layer.weight, layer.bias, 2, 1, 1, 1, "constant", transposed=True, output_padding=1).tile > 0
    gy = torch.randn(y.shape, dtype=torch.float64, device=DEV)
    y.backward(gy)
    xr = x.detach().clone().requires_grad_()
    wr = layer.weight.detach().clone().requires_grad_()
    br = layer.bias.detach().clone().requires_grad_()
    want = F.conv_transpose2d(xr, wr, br, stride=2, padding=1, output_padding=1)
    want.backward(gy)
    assert _rel(y, want) < TOL
    for name, a_, b_ in (("dX", x.grad, xr.grad), ("dW", layer.weight.grad, wr.grad), ("db", layer.bias.grad, br.grad)):
        assert _rel(a_, b_) < TOL, (name, _rel(a_, b_))


def test_float64_long_dilated_axis_stays_on_the_direct_kernel():
    from fft_conv_pytorch_amd.functional import _plan_for, fft_conv
    gen = torch.Generator().manual_seed(3)
    x, w, b = _rand(gen, 1, 2, 6, 1400), _rand(gen, 2, 2, 3, 600), _rand(gen, 2)
    plan = _plan_for(x, w, b, 1, 0, (1, 2), 1, "constant")       # dilated extent 1199 > 1025 along x
    assert plan.tile == 0 and plan.workspace_bytes == 0
    got = fft_conv(x, w, b, dilation=(1, 2))
    assert _rel(got, F.conv2d(x, w, b, dilation=(1, 2))) < TOL


def test_float64_knob_direct_kernel_agrees_with_the_fft_path(monkeypatch):
    from fft_conv_pytorch_amd import _native
    from fft_conv_pytorch_amd.functional import _plan_for, fft_conv
    gen = torch.Generator().manual_seed(9)
    x, w, b = _rand(gen, 2, 4, 10, 12, 14), _rand(gen, 4, 4, 3, 3, 3), _rand(gen, 4)
    outs = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("FFTCONV_F64_FFT", knob)               # (read at plan creation)
        _native.clear_plan_cache()
        outs[knob] = fft_conv(x, w, b, padding=1, padding_mode="circular")
        assert (_plan_for(x, w, b, 1, 1, 1, 1, "circular").tile > 0) == (knob == "1")
    monkeypatch.delenv("FFTCONV_F64_FFT", raising=False)
    _native.clear_plan_cache()
    assert _rel(outs["1"], outs["0"]) < TOL


def test_float64_3d_cached_spectrum_equals_uncached():
    from fft_conv_pytorch_amd import FFTConv3d
    torch.manual_seed(2)
    layer = FFTConv3d(4, 4, (3, 5, 3), padding=(1, 2, 1), bias=True).to(DEV).double()
    x = torch.randn(2, 4, 9, 16, 11, dtype=torch.float64, device=DEV)
    with torch.no_grad():
        layer.cache_kernel_spectrum = False
        uncached = layer(x)                  # transforms the weight in the call
        layer.cache_kernel_spectrum = True
        layer.eval()
        first = layer(x)
        cached = layer(x)                    # eval: the kernel spectrum of the first call
    assert layer.__dict__["_spectrum_cache"][1].plan.tile > 0
    assert torch.equal(first, cached) and torch.equal(uncached, cached)
    want = F.conv3d(x, layer.weight, layer.bias, padding=(1, 2, 1))
    assert _rel(cached, want) < TOL


def test_float64_2d_forward_replays_from_a_captured_graph():
    from fft_conv_pytorch_amd import FFTConv2d
    torch.manual_seed(4)
    layer = FFTConv2d(4, 4, 7, padding=3, bias=True).to(DEV).double().eval()
    x = torch.randn(2, 4, 40, 48, dtype=torch.float64, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        eager = layer(x)                     # warm: plan and kernel spectrum exist before the capture
        eager = layer(x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        out = layer(x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert _rel(eager, F.conv2d(x, layer.weight, layer.bias, padding=3)) < TOL
