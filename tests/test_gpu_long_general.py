"""Stride, dilation and padding modes of ``fft_long_conv`` / ``FFTLongConv1d`` on the GPU (the mapped builds of the column
kernels, csrc/long1d.hpp).  Rows just past the 4096-point hand-off, so the long kernels run: a spy on ``LongPlan`` shows the
plans that did.  The reference is the float64 oracle on CPU copies and the bound route_util.TOL32 on
max|got - want| / max|want|; 16-bit results are compared bit for bit with the cast path."""
import math

import pytest
import torch

from fft_conv_pytorch_amd import FFTLongConv1d, _native, autograd, fft_conv, fft_long_conv
from fft_conv_pytorch_amd import functional as F_
from tests.route_util import TOL32
from tests.test_host_long_general import MODES, _expect

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HALF = (torch.float16, torch.bfloat16)
KNOBS = ("FFTCONV_LONG_N", "FFTCONV_LONG_WS_MB", "FFTCONV_HALF_IO", "FFTCONV_TILE")


def _clear():
    _native.clear_plan_cache()
    F_._REFUSED_HALF.clear()
    autograd._BWD_PLANS.clear()


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    _clear()
    yield
    _clear()


@pytest.fixture
def ran(monkeypatch):
    """The long plans whose forward ran: (key without the tag, info words, x dtype code, y dtype code) per launch."""
    seen = []
    real = _native.LongPlan.forward

    def forward(plan, x_ptr, spectrum_ptr, bias_ptr, y_ptr, workspace_ptr, stream, x_dtype=0, y_dtype=0):
        seen.append((plan.key, dict(plan.info), x_dtype, y_dtype))
        return real(plan, x_ptr, spectrum_ptr, bias_ptr, y_ptr, workspace_ptr, stream, x_dtype, y_dtype)
    monkeypatch.setattr(_native.LongPlan, "forward", forward)
    return seen


def _err(got, want):
    return (got.double().cpu() - want.double()).abs().max().item() / max(want.double().abs().max().item(), 1e-300)


def _tensors(B, cin, cout, g, L, K, bias=True, seed=0):
    gen = torch.Generator().manual_seed(seed + L + 3 * K)
    x = torch.randn(B, cin, L, generator=gen).to(DEV)
    w = torch.randn(cout, cin // g, K, generator=gen).to(DEV)
    b = torch.randn(cout, generator=gen).to(DEV) if bias else None
    return x, w, b


def _want(x, w, b, padding, g, causal, s, d, mode):
    return _expect(x.double().cpu(), w.double().cpu(), None if b is None else b.double().cpu(), padding, g, causal, s, d, mode)


def _ext(padding_mode, s, d):
    return (MODES[padding_mode], 1, d, s)


def _check(ran, B, cin, cout, g, L, K, padding, causal, s, d, mode, bias=True):
    x, w, b = _tensors(B, cin, cout, g, L, K, bias)
    del ran[:]
    got = fft_long_conv(x, w, b, padding=padding, groups=g, causal=causal, stride=s, dilation=d, padding_mode=mode)
    want = _want(x, w, b, padding, g, causal, s, d, mode)
    # the long kernels ran, once, on the extended plan of these arguments
    assert len(ran) == 1 and ran[0][0][11:] == _ext(mode, s, d), ran
    assert ran[0][1]["N1"] * ran[0][1]["N2"] > F_.LONG_HANDOFF_POINTS and ran[0][1]["out_len"] == want.shape[2]
    assert got.shape == want.shape and got.dtype == torch.float32 and got.is_contiguous()
    err = _err(got, want)
    print(f"long B{B} {cin}->{cout} g{g} L{L} K{K} p{padding} causal={causal} s{s} d{d} {mode} "
          f"N={ran[0][1]['N1']}x{ran[0][1]['N2']}: err {err:.2e}")
    assert err <= TOL32
    return x, w, b, got, want


# ------------------------------------------------------------------------------------------------ forward
FORWARD = [
    # B, cin, cout, g, L, K, padding, causal, stride, dilation, mode
    (3, 4, 4, 4, 5000, 1200, 0, False, 2, 1, "constant"),         # stride 2, depthwise
    (3, 6, 4, 2, 5001, 1000, 0, False, 3, 1, "constant"),         # stride 3, grouped
    (3, 2, 3, 1, 6000, 1500, 0, False, 1, 2, "constant"),         # dilation 2, dense
    (3, 4, 4, 4, 7000, 2000, 0, False, 1, 3, "constant"),         # dilation 3
    (3, 2, 2, 1, 7000, 1200, 0, False, 1, 5, "constant"),         # dilation 5
    (3, 6, 4, 2, 5000, 1200, 37, False, 2, 3, "constant"),        # both, zero padding 37
    (3, 4, 4, 4, 5000, 1200, 37, False, 2, 3, "reflect"),
    (3, 2, 2, 1, 5000, 1000, 4999, False, 1, 1, "reflect"),       # reflect at L - 1
    (3, 4, 6, 2, 5000, 1000, 37, False, 1, 2, "replicate"),
    (3, 2, 2, 2, 5000, 3000, 37, False, 3, 1, "circular"),
    (3, 4, 4, 4, 5000, 1000, "same", False, 1, 3, "constant"),    # 'same' with dilation: 2997 = 1498 + 1499
    (3, 2, 2, 1, 5000, 1000, "same", False, 1, 3, "circular"),
    (3, 3, 3, 3, 5000, 2000, 0, True, 3, 1, "constant"),          # causal with stride
    (3, 2, 4, 2, 5000, 1500, 0, True, 1, 4, "constant"),          # causal, dilated extent 5997 > L
    (3, 2, 2, 1, 5001, 1500, 0, True, 2, 5, "constant"),
]


@pytest.mark.parametrize("B,cin,cout,g,L,K,padding,causal,s,d,mode", FORWARD)
def test_forward_parity(B, cin, cout, g, L, K, padding, causal, s, d, mode, ran):
    _check(ran, B, cin, cout, g, L, K, padding, causal, s, d, mode, bias=(L + K) % 2 == 0)


# the column blocks are 16 / 8 / 4 / 2 wide depending on N1
COLUMN_GEOMETRIES = [(64, 128), (128, 64), (256, 64), (512, 64), (1024, 64), (2048, 64), (4096, 64), (64, 4096)]


@pytest.mark.parametrize("N1,N2", COLUMN_GEOMETRIES)
def test_every_column_geometry_runs_the_mapped_case(N1, N2, monkeypatch, ran):
    """(64 x 64 holds 4096 points, fewer than this case's 5074: N1 = 64 runs as 64 x 128 here and as 64 x 64 below.)"""
    monkeypatch.setenv("FFTCONV_LONG_N", f"{N1}x{N2}")
    _clear()
    _check(ran, 3, 4, 4, 2, 5000, 1200, 37, False, 2, 3, "reflect")
    assert (ran[0][1]["N1"], ran[0][1]["N2"]) == (N1, N2)


def test_64_x_64_runs_the_mapped_case_at_the_primitive(monkeypatch):
    """A row of at most 4096 points goes to fft_conv in the functional, so the primitive itself is called (as
    test_gpu_long_conv.py does for this factorisation): the mapped case on a row that fits, into a NaN-filled output."""
    monkeypatch.setenv("FFTCONV_LONG_N", "64x64")
    _clear()
    B, cin, cout, g, L, K, s, d, mode = 3, 4, 4, 2, 3900, 900, 2, 3, "reflect"
    x, w, b = _tensors(B, cin, cout, g, L, K)
    plan = F_._long_plan(x, cout, g, K, 37, 37, False, 0, True, pad_mode=MODES[mode], tap_dil=d, out_step=s)
    assert (plan.info["N1"], plan.info["N2"]) == (64, 64)
    spectrum = F_.transform_kernel(plan, w)
    out = torch.full((B, cout, plan.out_len), float("nan"), device=DEV)
    ws = F_.new_workspace(plan, x.device)
    plan.forward(x.data_ptr(), spectrum.buf.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = _want(x, w, b, 37, g, False, s, d, mode)
    assert out.shape == want.shape and not torch.isnan(out).any()
    assert _err(out, want) <= TOL32


@pytest.mark.parametrize("L", [5001, 5002, 5003])
def test_seam_of_the_last_strided_sample(L, ran):
    """K = 1000 at dilation 2 covers 1999 positions: at L = 5002 the last stride-1 sample, 3003, is a kept one (3 * 1001);
    one sample more and one less leave it between two kept ones."""
    x, w, b, got, want = _check(ran, 3, 2, 2, 2, L, 1000, 0, False, 3, 2, "constant")
    assert got.shape[2] == (L - 1999) // 3 + 1
    tail = (got[..., -2:].double().cpu() - want[..., -2:]).abs().max().item() / want.abs().max().item()
    assert tail <= TOL32


@pytest.mark.parametrize("pad,L", [(48, 5008), (41, 5003)])
def test_circular_wrap_against_the_column_blocks(pad, L, ran):
    """Padding 48 on L = 5008 puts both wraps (row positions 48 and 5056) on the first column of a 16-wide block; padding
    41 on L = 5003 puts them inside a block (positions 41 and 5044 = 16 * 315 + 4), so one block reads both ends of x."""
    x, w, b, got, want = _check(ran, 3, 2, 2, 1, L, 1000, pad, False, 1, 1, "circular")
    assert ran[0][1]["N2"] % 16 == 0
    head = (got[..., :pad + 2].double().cpu() - want[..., :pad + 2]).abs().max().item() / want.abs().max().item()
    assert head <= TOL32


def test_agrees_with_the_segment_route_of_fft_conv(ran):
    x, w, b = _tensors(3, 4, 4, 4, 9000, 2500, seed=4)
    kw = dict(stride=2, padding=37, dilation=3, groups=4, padding_mode="reflect")
    long = fft_long_conv(x, w, b, **kw)
    assert len(ran) == 1
    seg = fft_conv(x, w, b, **kw)
    assert long.shape == seg.shape
    assert (long - seg).abs().max().item() / seg.abs().max().item() <= 2 * TOL32


def test_short_rows_go_to_the_fft_conv_kernels_with_the_arguments_passed_through(ran):
    x, w, b = _tensors(3, 4, 4, 2, 3000, 400)
    for kw in (dict(padding=37, stride=2, dilation=3, padding_mode="circular"), dict(causal=True, stride=3, dilation=2)):
        got = fft_long_conv(x, w, b, groups=2, **kw)
        want = _want(x, w, b, kw.get("padding", 0), 2, kw.get("causal", False), kw["stride"], kw["dilation"],
                     kw.get("padding_mode", "constant"))
        assert got.shape == want.shape and _err(got, want) <= TOL32
    assert ran == []


# ------------------------------------------------------------------------------------------------ gradients
GRADS = [
    # B, cin, cout, g, L, K, padding, causal, stride, dilation, mode
    (3, 4, 4, 4, 5000, 1200, 0, False, 2, 3, "constant"),
    (2, 4, 6, 2, 5000, 1000, 37, False, 2, 1, "reflect"),
    (3, 2, 2, 1, 5000, 2000, 0, True, 3, 1, "constant"),
]


@pytest.mark.parametrize("B,cin,cout,g,L,K,padding,causal,s,d,mode", GRADS)
def test_gradients_match_float64_autograd_through_the_oracle(B, cin, cout, g, L, K, padding, causal, s, d, mode, ran):
    x, w, b = _tensors(B, cin, cout, g, L, K)
    x64, w64, b64 = (t.double().cpu().requires_grad_() for t in (x, w, b))
    want = _expect(x64, w64, b64, padding, g, causal, s, d, mode)
    gy = torch.randn(want.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    want.backward(gy)
    xs, ws, bs = (t.clone().requires_grad_() for t in (x, w, b))
    y = fft_long_conv(xs, ws, bs, padding=padding, groups=g, causal=causal, stride=s, dilation=d, padding_mode=mode)
    y.backward(gy.float().to(DEV))
    torch.cuda.synchronize()
    # forward, dX (dY spread by the stride, the taps at the dilation), dW (dY as taps at the stride, every d-th lag kept)
    code = MODES[mode]
    assert [r[0][11:] for r in ran] == [(code, 1, d, s), (0, s, d, 1), (code, 1, s, d)], [r[0] for r in ran]
    assert all(r[1]["N1"] * r[1]["N2"] > F_.LONG_HANDOFF_POINTS for r in ran)
    for name, got, ref in (("y", y.detach(), want.detach()), ("dX", xs.grad, x64.grad), ("dW", ws.grad, w64.grad),
                           ("db", bs.grad, b64.grad)):
        assert got.shape == ref.shape, name
        err = _err(got, ref)
        print(f"grad s{s} d{d} {mode} causal={causal}: {name} err {err:.2e}")
        assert err <= TOL32, name


# ------------------------------------------------------------------------------------------------ 16 bits
def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not torch.equal(got.view(torch.int16), want.view(torch.int16)):
        n = (got.view(torch.int16) != want.view(torch.int16)).sum().item()
        raise AssertionError(f"{what}: {n} samples differ from the cast path "
                             f"(max |diff| {(got.float() - want.float()).abs().max().item():.3e})")


def _train_step(fn, x, w, b, gy):
    xs, ws, bs = (t.detach().clone().requires_grad_() for t in (x, w, b))
    y = fn(xs, ws, bs)
    saved = [(t.dtype, t.numel()) for t in y.grad_fn.saved_tensors] if hasattr(y.grad_fn, "saved_tensors") else None
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), xs.grad, ws.grad, bs.grad, saved


@pytest.mark.parametrize("dtype", HALF)
def test_sixteen_bit_output_and_gradients_have_the_bits_of_the_cast_path(dtype, monkeypatch, ran):
    B, cin, cout, g, L, K = 3, 4, 4, 2, 5001, 1201
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(B, cin, L, generator=gen).to(DEV).to(dtype)
    w = (torch.randn(cout, cin // g, K, generator=gen) / math.sqrt(cin // g * K)).to(DEV).to(dtype)
    b = torch.randn(cout, generator=gen).to(DEV).to(dtype)
    kw = dict(padding=37, groups=g, stride=2, dilation=3, padding_mode="reflect")
    fn = lambda xs, ws, bs: fft_long_conv(xs, ws, bs, **kw)      # noqa: E731
    with torch.no_grad():
        y_eval = fn(x, w, b)
    gy = torch.randn(y_eval.shape, generator=gen).to(DEV).to(dtype)
    c = F_._DTYPE_CODES[dtype]
    del ran[:]
    y, dx, dw, db, saved = _train_step(fn, x, w, b, gy)
    # forward 16 -> 16; dX of the padded row in float32 (folded, then rounded once); dW float32 from 16-bit operands
    assert [(r[2], r[3]) for r in ran] == [(c, c), (c, 0), (c, 0)], ran
    assert saved is not None and sorted(saved) == sorted([(dtype, x.numel()), (dtype, w.numel())]), saved
    assert (dx.dtype, dw.dtype, db.dtype) == (dtype,) * 3 and dx.shape == x.shape and dw.shape == w.shape
    _same_bits(y, y_eval, "training forward against the eval forward")

    del ran[:]
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    y0, dx0, dw0, db0, _ = _train_step(fn, x, w, b, gy)
    monkeypatch.delenv("FFTCONV_HALF_IO")
    assert [(r[2], r[3]) for r in ran] == [(0, 0)] * 3
    for name, got, ref in (("y", y, y0), ("dX", dx, dx0), ("dW", dw, dw0), ("db", db, db0)):
        _same_bits(got, ref, f"{dtype} {name} (FFTCONV_HALF_IO=0)")

    # the cast written out by hand: float32 leaves, the float32 function, everything rounded once
    x32, w32, b32 = (t.float().requires_grad_() for t in (x, w, b))
    y32 = fn(x32, w32, b32)
    y32.backward(gy.float())
    for name, got, ref in (("y", y, y32.detach()), ("dX", dx, x32.grad), ("dW", dw, w32.grad), ("db", db, b32.grad)):
        _same_bits(got, ref.to(dtype), f"{dtype} {name} against the float32 function")


@pytest.mark.parametrize("dtype", HALF)
def test_sixteen_bit_zero_padded_gradient_is_written_in_sixteen_bits(dtype, ran):
    """With zero padding dX needs no fold: the kernels write it in the dtype (causal, stride 2, dilation 2)."""
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(3, 2, 5001, generator=gen).to(DEV).to(dtype)
    w = (torch.randn(2, 1, 1501, generator=gen) / math.sqrt(1501)).to(DEV).to(dtype)
    kw = dict(groups=2, causal=True, stride=2, dilation=2)
    xs, ws = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = fft_long_conv(xs, ws, None, **kw)
    gy = torch.randn(y.shape, generator=gen).to(DEV).to(dtype)
    y.backward(gy)
    c = F_._DTYPE_CODES[dtype]
    assert [(r[2], r[3]) for r in ran] == [(c, c), (c, c), (c, 0)]
    x32, w32 = x.float().requires_grad_(), w.float().requires_grad_()
    y32 = fft_long_conv(x32, w32, None, **kw)
    y32.backward(gy.float())
    for name, got, ref in (("y", y.detach(), y32.detach()), ("dX", xs.grad, x32.grad), ("dW", ws.grad, w32.grad)):
        _same_bits(got, ref.to(dtype), f"{dtype} {name}")


# ------------------------------------------------------------------------------------------------ module
def test_module_loads_a_conv1d_state_dict_and_matches_it(monkeypatch, ran):
    torch.manual_seed(0)
    ref = torch.nn.Conv1d(4, 6, 1200, stride=2, padding=37, dilation=3, groups=2, padding_mode="circular").double()
    layer = FFTLongConv1d(4, 6, 1200, padding=37, groups=2, stride=2, dilation=3, padding_mode="circular")
    layer.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    layer = layer.to(DEV)
    ref.load_state_dict({k: v.double().cpu() for k, v in layer.state_dict().items()})       # (the float32 values)
    x = torch.randn(3, 4, 5000, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        want = ref(x.double().cpu())

    calls = []
    real = F_.transform_kernel
    monkeypatch.setattr(F_, "transform_kernel", lambda plan, kernel: calls.append(plan.key) or real(plan, kernel))
    layer.eval()
    with torch.no_grad():
        y1, y2 = layer(x), layer(x)
    assert len(calls) == 1 and calls[0][11:] == (3, 1, 3, 2), calls      # one transform for two calls, the extended plan
    assert len(ran) == 2 and ran[0][0] == ran[1][0] == calls[0]
    assert y1.shape == want.shape and _err(y1, want) <= TOL32 and torch.equal(y1, y2)
    layer.invalidate_kernel_spectrum()
    with torch.no_grad():
        y3 = layer(x)
    assert len(calls) == 2 and torch.equal(y3, y1)

    # a warmed call captures and replays
    static_x = x.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        static_y = layer(static_x)
    assert len(calls) == 2
    for seed in (2, 3):
        fresh = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed)).to(DEV)
        static_x.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            assert torch.equal(static_y, layer(fresh)), seed
