"""complex64 tensors through ``fft_long_conv`` / ``FFTLongConv1d``: the complex builds of the two column kernels
(csrc/long1d.hpp, one batch item per row of the transform), complex plans, the gradients in PyTorch's convention.

The reference is torch's own ``conv1d`` on complex128 CPU copies (forward and autograd); the error measure is
max|got - want| / max|want| with complex magnitudes and the bound ``route_util.TOL32``, the project's float32 bound, for
outputs and gradients alike.  Spies on ``LongPlan`` show the plans and the element types of every launch."""
import functools

import pytest
import torch
import torch.nn.functional as F

from fft_conv_pytorch_amd import FFTLongConv1d, _native, autograd, fft_long_conv
from fft_conv_pytorch_amd import functional as F_
from tests.route_util import TOL32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C64 = torch.complex64
KNOBS = ("FFTCONV_LONG_N", "FFTCONV_LONG_WS_MB", "FFTCONV_HALF_IO", "FFTCONV_TILE")
TILE_LENGTHS = (64, 128, 256, 512, 1024, 2048, 4096)


def _clear():
    _native.clear_plan_cache()
    autograd._BWD_PLANS.clear()


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    _clear()
    yield
    _clear()


@functools.lru_cache(maxsize=None)
def _tensors(B, cin, cout, g, L, K, seed=0):
    """complex64 signal, weight and bias on the CPU (shared, never written)."""
    gen = torch.Generator().manual_seed(seed + L + 3 * K)
    x = torch.randn(B, cin, L, 2, generator=gen)
    w = torch.randn(cout, cin // g, K, 2, generator=gen) / (cin // g * K) ** 0.5
    b = torch.randn(cout, 2, generator=gen)
    return tuple(torch.view_as_complex(t) for t in (x, w, b))


def _pad_mode(x, p, mode):
    """F.pad in a padding mode on the two planes (the same map for each)."""
    return torch.complex(F.pad(x.real, (p, p), mode=mode), F.pad(x.imag, (p, p), mode=mode))


def _conv_ref(x, w, b, padding, g, causal, stride, dilation, mode):
    """torch's conv1d on complex128 CPU tensors; the causal form on the left-padded row and the flipped kernel."""
    if causal:
        return F.conv1d(F.pad(x, (dilation * (w.shape[2] - 1), 0)), w.flip(-1), b, stride=stride, dilation=dilation, groups=g)
    if mode != "constant" and not isinstance(padding, str):
        x, padding = _pad_mode(x, padding, mode), 0
    return F.conv1d(x, w, b, stride=stride, padding=padding, dilation=dilation, groups=g)


@functools.lru_cache(maxsize=None)
def _want(B, cin, cout, g, L, K, padding, causal, stride=1, dilation=1, mode="constant", bias=True):
    x, w, b = (t.to(torch.complex128) for t in _tensors(B, cin, cout, g, L, K))
    return _conv_ref(x, w, b if bias else None, padding, g, causal, stride, dilation, mode)


def _bits(t):
    """The (re, im) planes of a complex tensor, a lazy conjugate or negation resolved first."""
    return torch.view_as_real(t.resolve_conj().resolve_neg())


def _err(got, want):
    return ((got.detach().cpu().to(torch.complex128) - want).abs().max() / want.abs().max()).item()


def _run(B, cin, cout, g, L, K, padding, causal, stride=1, dilation=1, mode="constant", bias=True):
    x, w, b = (t.to(DEV) for t in _tensors(B, cin, cout, g, L, K))
    got = fft_long_conv(x, w, b if bias else None, padding=padding, groups=g, causal=causal, stride=stride,
                        dilation=dilation, padding_mode=mode)
    want = _want(B, cin, cout, g, L, K, padding, causal, stride, dilation, mode, bias)
    assert got.dtype == C64 and got.is_contiguous() and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    err = _err(got, want)
    print(f"B{B} {cin}->{cout} g{g} L{L} K{K} p{padding} causal={causal} s{stride} d{dilation} {mode}: err {err:.3e}")
    return err


class _Spies:
    """Every LongPlan created (its key) and the fc_dtype codes of every launch: (x, y) of LongPlan.forward, the weight's
    of LongPlan.transform_kernel, and the plan of each."""

    def __init__(self, monkeypatch):
        self.forwards, self.transforms, self.created, self.plans = [], [], [], []
        real_init, real_fwd, real_tk = _native.LongPlan.__init__, _native.LongPlan.forward, _native.LongPlan.transform_kernel

        def init(plan, key, device_index=0):
            self.created.append(tuple(key))
            return real_init(plan, key, device_index)

        def forward(plan, x_ptr, spectrum_ptr, bias_ptr, y_ptr, workspace_ptr, stream, x_dtype=0, y_dtype=0):
            self.forwards.append((x_dtype, y_dtype))
            self.plans.append(plan)
            return real_fwd(plan, x_ptr, spectrum_ptr, bias_ptr, y_ptr, workspace_ptr, stream, x_dtype, y_dtype)

        def transform_kernel(plan, weight_ptr, spectrum_ptr, workspace_ptr, stream, weight_dtype=0):
            self.transforms.append(weight_dtype)
            self.plans.append(plan)
            return real_tk(plan, weight_ptr, spectrum_ptr, workspace_ptr, stream, weight_dtype)
        monkeypatch.setattr(_native.LongPlan, "__init__", init)
        monkeypatch.setattr(_native.LongPlan, "forward", forward)
        monkeypatch.setattr(_native.LongPlan, "transform_kernel", transform_kernel)


# ------------------------------------------------------------------------------------------------ forward
SWEEP = (3, 2, 2, 1, 3000, 700, 350, False)       # odd batch: nothing is paired; 3700 points fit 64 x 64


@pytest.mark.parametrize("N1,N2", [(n, 64) for n in TILE_LENGTHS] + [(64, n) for n in TILE_LENGTHS[1:]])
def test_every_column_and_row_geometry(N1, N2, monkeypatch):
    monkeypatch.setenv("FFTCONV_LONG_N", f"{N1}x{N2}")
    _clear()
    spies = _Spies(monkeypatch)
    assert _run(*SWEEP) <= TOL32
    assert [(p.info["N1"], p.info["N2"]) for p in spies.plans] == [(N1, N2)] * 2


def test_the_c_level_forward_writes_every_sample_and_nothing_else():
    """Into a NaN-filled output with a guard row behind it: every sample of the kept window written, the guard untouched."""
    B, cin, cout, g, L, K = 3, 2, 2, 1, 3001, 700
    x, w, b = (t.to(DEV) for t in _tensors(B, cin, cout, g, L, K))
    plan = F_._long_plan(x, cout, g, K, 350, 350, False, 0, True)
    assert plan.complex and plan.kind == _native.LONG_COMPLEX and plan.dtype == C64
    spectrum = F_.transform_kernel(plan, w)
    ws = F_.new_workspace(plan, x.device)
    nan = float("nan")
    out = torch.full((B + 1, cout, plan.out_len), complex(nan, nan), device=DEV, dtype=C64)
    plan.forward(x.data_ptr(), spectrum.buf.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(),
                 torch.cuda.current_stream().cuda_stream, 4, 4)
    torch.cuda.synchronize()
    assert not torch.isnan(_bits(out[:B])).any()
    assert torch.isnan(_bits(out[B])).all()
    assert _err(out[:B], _want(B, cin, cout, g, L, K, 350, False)) <= TOL32


LAYOUTS = [
    # B, cin, cout, g, L, K, padding, causal
    (3, 6, 4, 2, 5001, 1201, 100, False),        # grouped, Cin != Cout, odd row
    (2, 4, 4, 4, 4097, 4097, 0, True),           # depthwise, K = L
    (3, 3, 5, 1, 5000, 900, "same", False),      # dense, 'same' with an even kernel
    (2, 2, 2, 1, 3001, 6000, 0, True),           # causal, K > L
    (1, 2, 2, 2, 5000, 33, 0, False),            # one item, a short filter, no padding
]


@pytest.mark.parametrize("B,cin,cout,g,L,K,padding,causal", LAYOUTS)
def test_channel_layouts_and_causal(B, cin, cout, g, L, K, padding, causal):
    assert _run(B, cin, cout, g, L, K, padding, causal) <= TOL32
    assert _run(B, cin, cout, g, L, K, padding, causal, bias=False) <= TOL32


def test_a_short_row_runs_a_complex_long_plan_at_64_by_64(monkeypatch):
    """L = K = 100, causal: a real call hands such a row to fft_conv, which has no complex route."""
    spies = _Spies(monkeypatch)
    assert _run(2, 2, 2, 1, 100, 100, 0, True) <= TOL32
    assert spies.forwards == [(4, 4)] and spies.transforms == [4]
    assert [(p.info["N1"], p.info["N2"], p.complex) for p in spies.plans] == [(64, 64, True)] * 2
    # and the real call on the same shape creates no long plan at all
    spies.created.clear()
    x, w, b = (t.real.contiguous().to(DEV) for t in _tensors(2, 2, 2, 1, 100, 100))
    fft_long_conv(x, w, b, causal=True)
    assert spies.created == []


MAPPED = [
    # B, cin, cout, g, L, K, padding, causal, stride, dilation, mode
    (3, 4, 4, 2, 5000, 1200, 100, False, 2, 1, "constant"),       # stride: the mapped long_cols_inv
    (3, 4, 4, 2, 5000, 1200, 100, False, 1, 3, "constant"),       # dilation: the mapped filter transform
    (3, 2, 2, 1, 5000, 1000, 37, False, 1, 1, "reflect"),         # the mapped long_cols_fwd, one mode each
    (3, 2, 2, 1, 5000, 1000, 37, False, 1, 1, "replicate"),
    (3, 2, 2, 1, 5003, 1000, 41, False, 1, 1, "circular"),
    (3, 4, 6, 2, 5000, 1200, 37, False, 2, 3, "circular"),        # all three at once
    (3, 3, 3, 3, 5000, 2000, 0, True, 3, 2, "constant"),          # causal, strided and dilated
]


@pytest.mark.parametrize("geometry", ["128x64", "256x128"])
@pytest.mark.parametrize("B,cin,cout,g,L,K,padding,causal,stride,dilation,mode", MAPPED)
def test_mapped_builds_forward(B, cin, cout, g, L, K, padding, causal, stride, dilation, mode, geometry, monkeypatch):
    n1, n2 = (int(v) for v in geometry.split("x"))
    extent = dilation * (K - 1) + 1
    need = L + extent - 1 if causal else L + 2 * padding
    if n1 * n2 >= need:
        monkeypatch.setenv("FFTCONV_LONG_N", geometry)
    else:
        monkeypatch.setenv("FFTCONV_LONG_N", f"{n1 * 2}x{n2}")       # (the row is longer than the smaller plan)
    _clear()
    assert _run(B, cin, cout, g, L, K, padding, causal, stride, dilation, mode) <= TOL32


# ------------------------------------------------------------------------------------------------ gradients
def _train_step(fn, x, w, b, gy):
    xs, ws, bs = (t.detach().clone().requires_grad_() for t in (x, w, b))
    y = fn(xs, ws, bs)
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), xs.grad, ws.grad, bs.grad


GRAD_CASES = [
    # B, cin, cout, g, L, K, padding, causal, stride, dilation, mode, forced geometry
    (3, 6, 4, 2, 5000, 1200, 100, False, 1, 1, "constant", None),           # plain
    (3, 3, 3, 3, 3000, 5000, 0, True, 1, 1, "constant", None),              # causal, K > L
    (3, 4, 4, 2, 5000, 1200, 37, False, 2, 3, "reflect", None),             # strided + dilated with a padding mode
    (2, 4, 6, 2, 5000, 1200, 37, False, 2, 3, "circular", "256x128"),       # ... at a second geometry
    (2, 2, 2, 1, 5000, 800, 33, False, 1, 1, "replicate", "128x64"),
]


@pytest.mark.parametrize("B,cin,cout,g,L,K,padding,causal,stride,dilation,mode,geometry", GRAD_CASES)
def test_gradients_match_complex128_autograd(B, cin, cout, g, L, K, padding, causal, stride, dilation, mode, geometry,
                                             monkeypatch):
    if geometry:
        monkeypatch.setenv("FFTCONV_LONG_N", geometry)
        _clear()
    x, w, b = _tensors(B, cin, cout, g, L, K)
    x64, w64, b64 = (t.to(torch.complex128).requires_grad_() for t in (x, w, b))
    want = _conv_ref(x64, w64, b64, padding, g, causal, stride, dilation, mode)
    gen = torch.Generator().manual_seed(1)
    gy = torch.view_as_complex(torch.randn(tuple(want.shape) + (2,), generator=gen))
    want.backward(gy.to(torch.complex128))
    spies = _Spies(monkeypatch)
    fn = lambda xs, ws, bs: fft_long_conv(xs, ws, bs, padding=padding, groups=g, causal=causal, stride=stride,      # noqa: E731
                                          dilation=dilation, padding_mode=mode)
    y, dx, dw, db = _train_step(fn, x.to(DEV), w.to(DEV), b.to(DEV), gy.to(DEV))
    errs = {"y": _err(y, want.detach()), "dX": _err(dx, x64.grad), "dW": _err(dw, w64.grad), "db": _err(db, b64.grad)}
    print(f"B{B} {cin}->{cout} g{g} L{L} K{K} p{padding} causal={causal} s{stride} d{dilation} {mode}: "
          + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for name, got, leaf in (("dX", dx, x), ("dW", dw, w), ("db", db, b)):
        assert got.dtype == C64 and got.shape == leaf.shape, name
    assert all(v <= TOL32 for v in errs.values()), errs
    # forward, dX, dW: one run of the primitive each, all on complex plans with complex64 operands
    assert spies.forwards == [(4, 4)] * 3 and spies.transforms == [4] * 3, (spies.forwards, spies.transforms)
    assert all(len(key) == 16 and key[15] & _native.LONG_COMPLEX for key in spies.created), spies.created
    assert sorted(key[15] for key in spies.created) == [1, 1 | _native.LONG_CONJ_SIGNAL, 1 | _native.LONG_CONJ_TAPS]
    assert all(p.complex for p in spies.plans)


def test_gradient_flows_through_a_lazily_conjugated_leaf():
    x, w, b = (t.to(DEV) for t in _tensors(2, 2, 2, 1, 5000, 300))
    gy = torch.view_as_complex(torch.randn(2, 2, 4701, 2, generator=torch.Generator().manual_seed(2))).to(DEV)
    _, dx, dw, db = _train_step(lambda xs, ws, bs: fft_long_conv(xs.conj(), ws.conj(), bs.conj()), x, w, b, gy)
    _, dx0, dw0, db0 = _train_step(lambda xs, ws, bs: fft_long_conv(xs, ws, bs),
                                   x.conj().resolve_conj(), w.conj().resolve_conj(), b.conj().resolve_conj(), gy)
    # d/d(leaf) of f(conj(leaf)) is the conjugate of the gradient at the conjugated point
    for got, ref in ((dx, dx0), (dw, dw0), (db, db0)):
        assert torch.equal(_bits(got), _bits(ref.conj()))


# ------------------------------------------------------------------------------------------------ conjugates, real data
def test_lazy_conjugates_equal_resolved_copies_bit_for_bit():
    x, w, b = (t.to(DEV) for t in _tensors(3, 4, 4, 2, 5001, 1201))
    lazy = (x.conj(), w.conj(), b.conj())
    assert all(t.is_conj() for t in lazy)
    got = fft_long_conv(*lazy, padding=100, groups=2)
    ref = fft_long_conv(*(t.resolve_conj() for t in lazy), padding=100, groups=2)
    assert not got.is_conj() and torch.equal(_bits(got), _bits(ref))
    want = _conv_ref(*(t.cpu().to(torch.complex128).conj() for t in (x, w, b)), 100, 2, False, 1, 1, "constant")
    assert _err(got, want) <= TOL32
    # the neg bit is treated the same way
    xn = torch._neg_view(x)
    assert xn.is_neg()
    assert torch.equal(_bits(fft_long_conv(xn, w, b, padding=100, groups=2)),
                       _bits(fft_long_conv(-x, w, b, padding=100, groups=2)))


def test_real_valued_complex_input_agrees_with_the_float32_call():
    B, cin, cout, g, L, K = 3, 4, 4, 2, 5001, 1201
    x, w, b = _tensors(B, cin, cout, g, L, K)
    xr, wr, br = (t.real.contiguous().to(DEV) for t in (x, w, b))
    xc, wc, bc = (torch.complex(t, torch.zeros_like(t)) for t in (xr, wr, br))
    y32 = fft_long_conv(xr, wr, br, padding=100, groups=g)
    yc = fft_long_conv(xc, wc, bc, padding=100, groups=g)
    assert yc.dtype == C64 and y32.dtype == torch.float32
    scale = y32.abs().max().item()
    re, im = (yc.real - y32).abs().max().item() / scale, yc.imag.abs().max().item() / scale
    print(f"real-valued complex input: real parts {re:.3e}, imaginary parts {im:.3e} of max|y|")
    assert re <= TOL32 and im <= TOL32


# ------------------------------------------------------------------------------------------------ plans and launches
def test_one_complex_plan_and_one_launch_per_forward_call(monkeypatch):
    x, w, b = (t.to(DEV) for t in _tensors(3, 4, 4, 2, 5001, 1201))
    spies = _Spies(monkeypatch)
    fft_long_conv(x, w, b, padding=100, groups=2)
    assert spies.forwards == [(4, 4)] and spies.transforms == [4]
    assert len(spies.created) == 1 and len(spies.created[0]) == 16 and spies.created[0][15] == _native.LONG_COMPLEX
    plan = spies.plans[0]
    assert plan.complex and spies.plans[1] is plan
    assert plan.info["slab_pairs"] == 3 and plan.info["workspace_bytes"] == 3 * 8 * plan.info["N1"] * plan.info["N2"] * 8
    fft_long_conv(x, w, b, padding=100, groups=2)
    assert len(spies.created) == 1 and spies.forwards == [(4, 4)] * 2           # the cached plan
    # the real plan of the same shape is another plan under another key
    fft_long_conv(x.real.contiguous(), w.real.contiguous(), b.real.contiguous(), padding=100, groups=2)
    assert len(spies.created) == 2 and len(spies.created[1]) == 11 and not spies.plans[-1].complex


def test_slabs_of_batch_items_match_one_slab(monkeypatch):
    x, w, b = (t.to(DEV) for t in _tensors(5, 4, 4, 4, 16001, 9000))
    one = fft_long_conv(x, w, b, groups=4, causal=True)
    monkeypatch.setenv("FFTCONV_LONG_WS_MB", "5")        # 32768 points x 8 channels x 8 bytes = 2 MiB per item
    _clear()
    plan = F_._long_plan(x, 4, 4, 9000, 8999, 0, True, 16001, True)
    assert plan.info["slabs"] == 3 and plan.info["slab_pairs"] == 2
    got = fft_long_conv(x, w, b, groups=4, causal=True)
    assert torch.equal(_bits(got), _bits(one))
    assert _err(one, _want(5, 4, 4, 4, 16001, 9000, 0, True)) <= TOL32


# ------------------------------------------------------------------------------------------------ module
def test_module_matches_a_complex_conv1d_loaded_from_its_state_dict(monkeypatch):
    torch.manual_seed(0)
    layer = FFTLongConv1d(4, 6, 1200, padding=37, groups=2, stride=2, dilation=3, padding_mode="circular", dtype=C64).to(DEV)
    assert layer.weight.dtype == C64 and layer.bias.dtype == C64
    ref = torch.nn.Conv1d(4, 6, 1200, stride=2, padding=37, dilation=3, groups=2, padding_mode="circular",
                          dtype=torch.complex128)
    ref.load_state_dict({k: v.cpu().to(torch.complex128) for k, v in layer.state_dict().items()})
    back = torch.nn.Conv1d(4, 6, 1200, stride=2, padding=37, dilation=3, groups=2, padding_mode="circular", dtype=C64)
    back.load_state_dict(layer.state_dict())                         # interchanges both ways
    layer.load_state_dict(back.state_dict())
    x = torch.view_as_complex(torch.randn(3, 4, 5000, 2, generator=torch.Generator().manual_seed(1)))
    with torch.no_grad():
        want = ref(x.to(torch.complex128))

    calls = []
    real = F_.transform_kernel
    monkeypatch.setattr(F_, "transform_kernel", lambda plan, kernel: calls.append(kernel.dtype) or real(plan, kernel))
    layer.eval()
    xd = x.to(DEV)
    with torch.no_grad():
        y1, y2 = layer(xd), layer(xd)
    assert calls == [C64]                                            # one kernel transform for two calls
    assert y1.dtype == C64 and _err(y1, want) <= TOL32
    assert torch.equal(_bits(y1), _bits(y2))
    layer.invalidate_kernel_spectrum()
    with torch.no_grad():
        y3 = layer(xd)
    assert calls == [C64, C64]                                       # rebuilt
    assert torch.equal(_bits(y3), _bits(y1))

    # a training step against complex128 autograd through the reference module
    layer.train()
    xs = xd.clone().requires_grad_()
    x64 = x.to(torch.complex128).requires_grad_()
    gy = torch.view_as_complex(torch.randn(tuple(want.shape) + (2,), generator=torch.Generator().manual_seed(2)))
    layer(xs).backward(gy.to(DEV))
    ref(x64).backward(gy.to(torch.complex128))
    assert _err(xs.grad, x64.grad) <= TOL32
    assert _err(layer.weight.grad, ref.weight.grad) <= TOL32 and _err(layer.bias.grad, ref.bias.grad) <= TOL32
    assert layer.weight.grad.dtype == C64

    # a float32 layer converted afterwards
    conv = FFTLongConv1d(2, 2, 300, padding=10).to(DEV).to(C64)
    assert conv.weight.dtype == C64
    with torch.no_grad():
        y = conv(xd[:, :2])
        w64, b64 = conv.weight.cpu().to(torch.complex128), conv.bias.cpu().to(torch.complex128)
        assert _err(y, F.conv1d(x[:, :2].to(torch.complex128), w64, b64, padding=10)) <= TOL32


# ------------------------------------------------------------------------------------------------ refusals
def test_complex128_and_mixes_raise_type_error():
    x, w, b = (t.to(DEV) for t in _tensors(2, 2, 2, 1, 5000, 300))
    for args in ((x.to(torch.complex128), w.to(torch.complex128), b.to(torch.complex128)),
                 (x, w.real.contiguous(), b), (x.real.contiguous(), w, b), (x, w, b.real.contiguous()),
                 (x.real.contiguous(), w.real.contiguous(), b), (x, w.to(torch.complex128), b)):
        with pytest.raises(TypeError, match="share"):
            fft_long_conv(*args)
    with pytest.raises(TypeError, match="float64"):
        fft_long_conv(x.to(torch.complex128), w.to(torch.complex128), None)
    with pytest.raises(TypeError):
        F_.fft_conv(x, w, b)                                       # fft_conv has no complex route


def test_library_refuses_codes_that_do_not_fit_the_plan():
    x, w, b = (t.to(DEV) for t in _tensors(2, 2, 2, 1, 5000, 300))
    stream = torch.cuda.current_stream().cuda_stream
    cplan = F_._long_plan(x, 2, 1, 300, 0, 0, False, 0, True)
    rplan = F_._long_plan(x.real, 2, 1, 300, 0, 0, False, 0, True)
    assert cplan.complex and not rplan.complex and cplan is not rplan
    spec = torch.empty(cplan.spectrum_bytes // 4, device=DEV)
    ws = F_.new_workspace(cplan, x.device)
    out = torch.empty(2, 2, cplan.out_len, device=DEV, dtype=C64)
    args = (x.data_ptr(), spec.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), stream)
    for codes in ((4, 4), (4, 0), (0, 4)):
        with pytest.raises(ValueError, match="real plan"):
            rplan.forward(*args, *codes)
    with pytest.raises(ValueError, match="real plan"):
        rplan.transform_kernel(w.data_ptr(), spec.data_ptr(), ws.data_ptr(), stream, 4)
    for codes in ((0, 0), (4, 0), (2, 4), (4, 3)):
        with pytest.raises(ValueError, match="complex plan"):
            cplan.forward(*args, *codes)
    for code in (0, 2, 3):
        with pytest.raises(ValueError, match="complex plan"):
            cplan.transform_kernel(w.data_ptr(), spec.data_ptr(), ws.data_ptr(), stream, code)
    # float64 and unknown codes answer as on a real plan
    with pytest.raises(NotImplementedError, match="float64"):
        cplan.forward(*args, 1, 4)
    with pytest.raises(ValueError, match="dtype code 7"):
        cplan.forward(*args, 7, 4)
    with pytest.raises(ValueError, match="dtype code -1"):
        cplan.transform_kernel(w.data_ptr(), spec.data_ptr(), ws.data_ptr(), stream, -1)
    torch.cuda.synchronize()
