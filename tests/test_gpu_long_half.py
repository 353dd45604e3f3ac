"""float16 / bfloat16 tensors through ``fft_long_conv`` / ``FFTLongConv1d``: the column kernels read the 16-bit signal and
taps and write the 16-bit output themselves (csrc/long1d.hpp, Io<>), autograd saves the 16-bit tensors, and backward runs
the same primitive on 16-bit dY, x and the transposed weight.

The contract is the one of the 16-bit ``fft_conv``: float32 arithmetic, and every result has exactly the bits of "widen, run
the float32 function, round once" -- so outputs and gradients are compared bit for bit against that cast, written out by
hand, and against FFTCONV_HALF_IO=0.  One check per dtype bounds the error against the float64 oracle by the float32
path's bound plus one rounding to nearest.  Spies on ``LongPlan`` show the element types every launch was given."""
import copy
import math
import pickle

import pytest
import torch
import torch.nn.functional as F

from fft_conv_pytorch_amd import FFTLongConv1d, _native, autograd, fft_long_conv
from fft_conv_pytorch_amd import functional as F_
from oracle.fft_conv_oracle import fft_conv_oracle_torch
from tests.route_util import TOL32
from tests.test_gpu_long_conv import FORCED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HALF = (torch.float16, torch.bfloat16)
CODE = {torch.float32: 0, torch.float16: 2, torch.bfloat16: 3}
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}       # half an ulp of 1: one rounding to nearest
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


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, \
        f"{what}: {got.dtype} {tuple(got.shape)} vs {want.dtype} {tuple(want.shape)}"
    if not torch.equal(got.view(torch.int16), want.view(torch.int16)):
        diff = (got.float() - want.float()).abs().max().item()
        n = (got.view(torch.int16) != want.view(torch.int16)).sum().item()
        raise AssertionError(f"{what}: {n} samples differ from the cast path (max |diff| {diff:.3e})")


def _tensors(B, cin, cout, g, L, K, bias, dtype, seed=0):
    """16-bit signal, weight scaled by 1 / sqrt(Cin/g * K) (outputs of order one: nothing overflows in float16), bias."""
    gen = torch.Generator().manual_seed(seed + L + 3 * K)
    x = torch.randn(B, cin, L, generator=gen).to(DEV).to(dtype)
    w = (torch.randn(cout, cin // g, K, generator=gen) / math.sqrt(cin // g * K)).to(DEV).to(dtype)
    b = torch.randn(cout, generator=gen).to(DEV).to(dtype) if bias else None
    return x, w, b


def _by_hand(x, w, b, **kw):
    """What a caller writes without 16-bit kernels: widen, the float32 function, round once."""
    assert x.dtype in HALF
    y32 = fft_long_conv(x.float(), w.float(), None if b is None else b.float(), **kw)
    assert y32.dtype == torch.float32
    return y32.to(x.dtype)


def _knob_off(monkeypatch, x, w, b, **kw):
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    try:
        return fft_long_conv(x, w, b, **kw)
    finally:
        monkeypatch.delenv("FFTCONV_HALF_IO")


def _forward_bits(monkeypatch, B, cin, cout, g, L, K, padding, causal, bias, dtype, what):
    x, w, b = _tensors(B, cin, cout, g, L, K, bias, dtype)
    kw = dict(padding=padding, groups=g, causal=causal)
    got = fft_long_conv(x, w, b, **kw)
    assert got.dtype == dtype and got.is_contiguous(), what
    _same_bits(got, _by_hand(x, w, b, **kw), what)
    _same_bits(got, _knob_off(monkeypatch, x, w, b, **kw), what + " (FFTCONV_HALF_IO=0)")
    return x, w, b, got


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("N1,N2", FORCED)
def test_forward_bits_and_coverage_for_forced_factorisations(N1, N2, dtype, monkeypatch):
    """Every tile length on each side; odd L and odd output lengths, so row bases are only 2-byte aligned.  The C-level
    forward into a NaN-filled 16-bit output writes every sample, with the bits of the float32 C-level forward rounded."""
    monkeypatch.setenv("FFTCONV_LONG_N", f"{N1}x{N2}")
    _clear()
    B, cin, cout, g, L, K = 3, 4, 6, 2, (2501 if N1 * N2 == 4096 else 3001), 1501
    causal = (N1 + N2) % 3 != 0
    padding = 0 if causal else 700
    what = f"{N1}x{N2} {dtype}"
    x, w, b, got = _forward_bits(monkeypatch, B, cin, cout, g, L, K, padding, causal, True, dtype, what)
    assert got.shape[2] % 2 == 1 and L % 2 == 1

    pl, pr = (K - 1, 0) if causal else (padding, padding)
    plan = F_._long_plan(x, cout, g, K, pl, pr, causal, L if causal else 0, True)
    assert (plan.info["N1"], plan.info["N2"]) == (N1, N2)
    stream = torch.cuda.current_stream().cuda_stream
    spec16, spec32 = F_.transform_kernel(plan, w), F_.transform_kernel(plan, w.float())
    assert spec16.buf.dtype == torch.float32
    assert torch.equal(spec16.buf.view(torch.int32), spec32.buf.view(torch.int32)), what + ": spectrum of the 16-bit weight"
    b32 = b.float()
    out = torch.full((B, cout, plan.out_len), float("nan"), device=DEV, dtype=dtype)
    ref = torch.full((B, cout, plan.out_len), float("nan"), device=DEV)
    ws = F_.new_workspace(plan, x.device)
    plan.forward(x.data_ptr(), spec16.buf.data_ptr(), b32.data_ptr(), out.data_ptr(), ws.data_ptr(), stream,
                 CODE[dtype], CODE[dtype])
    x32 = x.float()
    plan.forward(x32.data_ptr(), spec32.buf.data_ptr(), b32.data_ptr(), ref.data_ptr(), ws.data_ptr(), stream)
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and not torch.isnan(ref).any(), what
    _same_bits(out, ref.to(dtype), what + " (C level)")
    if N1 * N2 > 4096:
        _same_bits(out, got, what + " (C level against the functional)")


PICKED = [
    # B, cin, cout, g, L, K, padding, causal, bias
    (3, 4, 4, 4, 4097, 4097, 0, True, True),            # K = L, depthwise, odd batch, odd row
    (2, 3, 5, 1, 5001, 5007, 0, True, False),           # K > L, one group with Cin != Cout
    (5, 6, 4, 2, 9001, 3000, "same", False, True),      # 'same' with an even kernel, 1 < g < C, odd batch
    (2, 4, 6, 2, 16385, 33, 0, False, False),           # a short filter on a long row, no bias
    (1, 4, 4, 4, 20001, 4001, 2000, False, True),       # padding K // 2, one batch item (a pair with zeros)
    (2, 2, 2, 1, 3001, 6000, 0, True, True),            # K = 2L
]


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("B,cin,cout,g,L,K,padding,causal,bias", PICKED)
def test_forward_bits_for_planner_picked_shapes(B, cin, cout, g, L, K, padding, causal, bias, dtype, monkeypatch):
    _forward_bits(monkeypatch, B, cin, cout, g, L, K, padding, causal, bias, dtype,
                  f"B{B} {cin}->{cout} g{g} L{L} K{K} p{padding} causal={causal} {dtype}")


@pytest.mark.parametrize("dtype", HALF)
def test_short_rows_keep_going_to_the_fft_conv_kernels(dtype, monkeypatch):
    _forward_bits(monkeypatch, 2, 4, 4, 2, 3001, 500, 200, False, True, dtype, f"short {dtype}")
    _forward_bits(monkeypatch, 3, 2, 2, 2, 1501, 2000, 0, True, True, dtype, f"short causal {dtype}")


@pytest.mark.parametrize("dtype", HALF)
def test_accuracy_against_the_float64_oracle(dtype):
    """The float32 path's bound plus one rounding to nearest (u = half an ulp of 1 in the dtype), elementwise:
    |got - want| <= (1 + u) * TOL32 * max|want| + u * |want| + 2^-25, want = the oracle on the widened 16-bit inputs."""
    u = UNIT[dtype]
    B, cin, cout, g, L, K = 3, 4, 4, 4, 5001, 5001
    x, w, b = _tensors(B, cin, cout, g, L, K, True, dtype)
    got = fft_long_conv(x, w, b, groups=g, causal=True).double().cpu()
    x64, w64, b64 = x.double().cpu(), w.double().cpu(), b.double().cpu()
    want = fft_conv_oracle_torch(F.pad(x64, (K - 1, 0)), w64.flip(-1), b64, groups=g)
    bound = (1 + u) * TOL32 * want.abs().max() + u * want.abs() + 2.0 ** -25
    excess = ((got - want).abs() - bound).max().item()
    print(f"long {dtype}: max|got - want| {(got - want).abs().max().item():.3e}, max|want| {want.abs().max().item():.3e}, "
          f"worst excess over the bound {excess:.3e}")
    assert got.shape == want.shape
    assert excess <= 0.0


@pytest.mark.parametrize("dtype", HALF)
def test_slabs_of_batch_pairs_match_one_slab(dtype, monkeypatch):
    x, w, b = _tensors(7, 4, 4, 4, 16001, 9000, True, dtype)
    one = fft_long_conv(x, w, b, groups=4, causal=True)
    monkeypatch.setenv("FFTCONV_LONG_WS_MB", "3")        # 32768 points x 8 channels x 8 bytes = 2 MiB per pair
    _clear()
    plan = F_._long_plan(x, 4, 4, 9000, 8999, 0, True, 16001, True)
    assert plan.info["slabs"] == 4 and plan.info["slab_pairs"] == 1
    _same_bits(fft_long_conv(x, w, b, groups=4, causal=True), one, f"slabs {dtype}")
    monkeypatch.delenv("FFTCONV_LONG_WS_MB")
    _clear()
    _same_bits(one, _by_hand(x, w, b, groups=4, causal=True), f"one slab {dtype}")


def test_special_values(monkeypatch):
    kw = dict(groups=4, causal=True)
    # inf in x: the rows of its transform pair turn NaN / inf exactly where the cast path's do
    for dtype in HALF:
        x, w, b = _tensors(4, 4, 4, 4, 5001, 5001, True, dtype, seed=2)
        x[1, 2, 1234] = float("inf")
        want, got = _by_hand(x, w, b, **kw), fft_long_conv(x, w, b, **kw)
        assert torch.isnan(want).any() or torch.isinf(want).any()
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want)), dtype
        fin = torch.isfinite(want)
        assert torch.equal(got[fin].view(torch.int16), want[fin].view(torch.int16)), dtype
        assert torch.equal(got[torch.isinf(got)], want[torch.isinf(want)]), dtype
    # float16 outputs beyond 65504 round to inf as .to() rounds them
    x, w, b = _tensors(2, 4, 4, 4, 5001, 5001, True, torch.float16, seed=3)
    x, w = x * 2000, w * 32                       # outputs of about 64000 sigma-one
    want, got = _by_hand(x, w, b, **kw), fft_long_conv(x, w, b, **kw)
    assert torch.isinf(want).any() and not torch.isnan(want).any(), "the case must overflow"
    assert torch.equal(torch.isinf(got), torch.isinf(want))
    _same_bits(got, want, "float16 overflow")
    # a bfloat16 NaN stays a NaN
    x, w, b = _tensors(2, 4, 4, 4, 5001, 5001, True, torch.bfloat16, seed=4)
    x[0, 1, 77] = float("nan")
    want, got = _by_hand(x, w, b, **kw), fft_long_conv(x, w, b, **kw)
    assert torch.isnan(want).any()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    fin = ~torch.isnan(want)
    assert torch.equal(got[fin].view(torch.int16), want[fin].view(torch.int16))


@pytest.mark.parametrize("dtype", HALF)
def test_mixed_dtypes_and_float64_raise_type_error(dtype):
    x, w, b = _tensors(2, 4, 4, 4, 5001, 5001, True, dtype)
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    with pytest.raises(TypeError, match="share"):
        fft_long_conv(x, w.float(), b, groups=4, causal=True)
    with pytest.raises(TypeError, match="share"):
        fft_long_conv(x, w.to(other), b.to(other), groups=4, causal=True)
    with pytest.raises(TypeError, match="share"):
        fft_long_conv(x, w, b.float(), groups=4, causal=True)
    with pytest.raises(TypeError, match="share"):
        fft_long_conv(x.float(), w, b, groups=4, causal=True)
    with pytest.raises(TypeError, match="float64"):
        fft_long_conv(x.double(), w.double(), b.double(), groups=4, causal=True)


def test_library_refuses_float64_and_unknown_dtype_codes():
    x, w, b = _tensors(2, 2, 2, 2, 5001, 5001, True, torch.float16)
    plan = F_._long_plan(x, 2, 2, 5001, 5000, 0, True, 5001, True)
    spectrum = F_.transform_kernel(plan, w)
    ws = F_.new_workspace(plan, x.device)
    out = torch.empty(2, 2, 5001, device=DEV, dtype=torch.float16)
    stream = torch.cuda.current_stream().cuda_stream
    args = (x.data_ptr(), spectrum.buf.data_ptr(), b.float().data_ptr(), out.data_ptr(), ws.data_ptr(), stream)
    with pytest.raises(NotImplementedError, match="float64"):
        plan.forward(*args, 1, 2)
    with pytest.raises(NotImplementedError, match="float64"):
        plan.forward(*args, 2, 1)
    with pytest.raises(ValueError, match="dtype code 7"):
        plan.forward(*args, 7, 2)
    with pytest.raises(NotImplementedError, match="float64"):
        plan.transform_kernel(w.data_ptr(), spectrum.buf.data_ptr(), ws.data_ptr(), stream, 1)
    with pytest.raises(ValueError, match="dtype code -1"):
        plan.transform_kernel(w.data_ptr(), spectrum.buf.data_ptr(), ws.data_ptr(), stream, -1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ training
class _Spies:
    """fc_dtype codes of every launch: (x, y) of LongPlan.forward and the weight's of LongPlan.transform_kernel."""

    def __init__(self, monkeypatch):
        self.forwards, self.transforms = [], []
        real_fwd, real_tk = _native.LongPlan.forward, _native.LongPlan.transform_kernel

        def forward(plan, x_ptr, spectrum_ptr, bias_ptr, y_ptr, workspace_ptr, stream, x_dtype=0, y_dtype=0):
            self.forwards.append((x_dtype, y_dtype))
            return real_fwd(plan, x_ptr, spectrum_ptr, bias_ptr, y_ptr, workspace_ptr, stream, x_dtype, y_dtype)

        def transform_kernel(plan, weight_ptr, spectrum_ptr, workspace_ptr, stream, weight_dtype=0):
            self.transforms.append(weight_dtype)
            return real_tk(plan, weight_ptr, spectrum_ptr, workspace_ptr, stream, weight_dtype)
        monkeypatch.setattr(_native.LongPlan, "forward", forward)
        monkeypatch.setattr(_native.LongPlan, "transform_kernel", transform_kernel)

    def reset(self):
        self.forwards.clear()
        self.transforms.clear()


def _train_step(fn, x, w, b, gy):
    xs, ws, bs = (t.detach().clone().requires_grad_() for t in (x, w, b))
    y = fn(xs, ws, bs)
    saved = [(t.dtype, t.numel()) for t in y.grad_fn.saved_tensors] if hasattr(y.grad_fn, "saved_tensors") else None
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), xs.grad, ws.grad, bs.grad, saved


GRAD_CASES = [
    # the three shapes of test_gradients_match_float64_autograd_through_the_oracle ...
    (3, 4, 4, 4, 5000, 5000, 0, True),
    (2, 6, 4, 2, 7000, 3000, 100, False),
    (2, 2, 2, 1, 3000, 6000, 0, True),
    # ... and padding wider than the filter: the leading / trailing output samples never met the data (pl < 0 in backward)
    (2, 4, 4, 2, 6001, 50, 100, False),
]


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("B,cin,cout,g,L,K,padding,causal", GRAD_CASES)
def test_gradient_bits_saved_tensors_and_routes(B, cin, cout, g, L, K, padding, causal, dtype, monkeypatch):
    what = f"B{B} {cin}->{cout} g{g} L{L} K{K} p{padding} causal={causal} {dtype}"
    c = CODE[dtype]
    x, w, b = _tensors(B, cin, cout, g, L, K, True, dtype)
    fn = lambda xs, ws, bs: fft_long_conv(xs, ws, bs, padding=padding, groups=g, causal=causal)      # noqa: E731
    with torch.no_grad():
        shape = fn(x, w, b).shape
    gy = torch.randn(shape, generator=torch.Generator().manual_seed(1)).to(DEV).to(dtype)
    spies = _Spies(monkeypatch)

    y, dx, dw, db, saved = _train_step(fn, x, w, b, gy)
    # forward, dX (16-bit dY and transposed weight -> 16-bit dX), dW (16-bit x and dY, a 16-bit filter transform -> float32)
    assert spies.forwards == [(c, c), (c, c), (c, 0)], (what, spies.forwards)
    assert spies.transforms == [c, c, c], (what, spies.transforms)
    assert saved is not None and sorted(saved) == sorted([(dtype, x.numel()), (dtype, w.numel())]), (what, saved)
    assert dx.dtype == dtype and dx.shape == x.shape and dw.dtype == dtype and dw.shape == w.shape, what
    assert db.dtype == dtype and db.shape == b.shape, what

    spies.reset()
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    y0, dx0, dw0, db0, _ = _train_step(fn, x, w, b, gy)
    monkeypatch.delenv("FFTCONV_HALF_IO")
    assert spies.forwards == [(0, 0)] * 3 and spies.transforms == [0, 0, 0], (what, spies.forwards, spies.transforms)
    for name, got, want in (("y", y, y0), ("dX", dx, dx0), ("dW", dw, dw0), ("db", db, db0)):
        _same_bits(got, want, f"{what}: {name}")

    # the cast written out by hand: float32 leaves, float32 function, gradients rounded once
    x32, w32, b32 = (t.float().requires_grad_() for t in (x, w, b))
    fn(x32, w32, b32).backward(gy.float())
    for name, got, want in (("dX", dx, x32.grad), ("dW", dw, w32.grad), ("db", db, b32.grad)):
        _same_bits(got, want.to(dtype), f"{what}: {name} against the float32 function")


@pytest.mark.parametrize("dtype", HALF)
def test_forward_routes(dtype, monkeypatch):
    c = CODE[dtype]
    x, w, b = _tensors(3, 4, 4, 4, 5001, 5001, True, dtype)
    spies = _Spies(monkeypatch)
    fft_long_conv(x, w, b, groups=4, causal=True)
    assert spies.forwards == [(c, c)] and spies.transforms == [c]
    spies.reset()
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    fft_long_conv(x, w, b, groups=4, causal=True)
    assert spies.forwards == [(0, 0)] and spies.transforms == [0]


# ------------------------------------------------------------------------------------------------ module
@pytest.mark.parametrize("dtype", HALF)
def test_module_cache_bits_training_and_copies(dtype, monkeypatch):
    torch.manual_seed(0)
    layer = FFTLongConv1d(4, 4, 3001, padding=1500, groups=2).to(DEV)
    with torch.no_grad():
        layer.weight.mul_(1.0 / math.sqrt(2 * 3001) / layer.weight.std())
    layer = layer.to(dtype)
    assert layer.weight.dtype == dtype and layer.bias.dtype == dtype
    x = torch.randn(3, 4, 6001, device=DEV).to(dtype)
    want = fft_long_conv(x, layer.weight.detach(), layer.bias.detach(), padding=1500, groups=2)

    calls = []
    real = F_.transform_kernel
    monkeypatch.setattr(F_, "transform_kernel", lambda plan, kernel: calls.append(kernel.dtype) or real(plan, kernel))
    layer.eval()
    with torch.no_grad():
        y1, y2 = layer(x), layer(x)
    assert calls == [dtype], calls                       # one kernel transform for two calls, of the 16-bit weight
    assert layer.__dict__["_spectrum_cache"][1].buf.dtype == torch.float32
    _same_bits(y1, want, f"module {dtype}")
    _same_bits(y2, want, f"module {dtype}, cached spectrum")
    with torch.no_grad():
        layer.weight.mul_(0.5)                           # bumps the version counter
        y3 = layer(x)
    assert len(calls) == 2
    _same_bits(y3, fft_long_conv(x, layer.weight.detach(), layer.bias.detach(), padding=1500, groups=2), "module, new weight")
    calls.clear()

    clone, pickled = copy.deepcopy(layer), pickle.loads(pickle.dumps(layer))
    for other in (clone, pickled):
        assert "_spectrum_cache" not in other.__dict__ and other.causal is False and other.weight.dtype == dtype
        with torch.no_grad():
            _same_bits(other(x), y3, "copied module")

    # a training step: gradients with the bits of the cast path
    layer.train()
    gy = torch.randn(y3.shape, generator=torch.Generator().manual_seed(5)).to(DEV).to(dtype)

    def step():
        layer.zero_grad(set_to_none=True)
        xs = x.detach().clone().requires_grad_()
        y = layer(xs)
        y.backward(gy)
        torch.cuda.synchronize()
        return y.detach(), xs.grad, layer.weight.grad.clone(), layer.bias.grad.clone()
    native = step()
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    cast = step()
    monkeypatch.delenv("FFTCONV_HALF_IO")
    for name, got, ref in zip(("y", "dX", "dW", "db"), native, cast):
        _same_bits(got, ref, f"module train step {dtype}: {name}")
    assert native[2].dtype == dtype and native[3].dtype == dtype


@pytest.mark.parametrize("dtype", HALF)
def test_warm_forward_is_capturable_and_replays_bit_for_bit(dtype):
    x, w, b = _tensors(3, 4, 4, 4, 20001, 20001, True, dtype)
    plan = F_._long_plan(x, 4, 4, 20001, 20000, 0, True, 20001, True)
    assert plan.info["slabs"] == 1
    spectrum = F_.transform_kernel(plan, w)
    static_x = x.clone()
    fft_long_conv(static_x, w, b, groups=4, causal=True)       # warm: plan and device tables exist
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = F_._long_run(static_x, w, b, 20000, 0, True, 20001, 4, spectrum)
    assert static_y.dtype == dtype
    for seed in (1, 2, 3):
        fresh = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed)).to(DEV).to(dtype)
        static_x.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        eager = F_._long_run(fresh, w, b, 20000, 0, True, 20001, 4, spectrum)
        _same_bits(static_y, eager, f"replay {seed} {dtype}")


# ------------------------------------------------------------------------------------------------ memory
def _added_peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def test_peak_memory_is_below_the_cast_paths_by_the_float32_copies(monkeypatch):
    """Derived, not measured: the cast path holds a float32 x (4 bytes per input sample) and a float32 y where the native
    call holds a 16-bit y; spectrum and workspace are equal.  So native + 4 bytes per input sample <= cast, for a forward
    call and for a forward + backward step."""
    dtype = torch.bfloat16
    B, C, L = 4, 64, 65536
    gen = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(B, C, L, generator=gen, device=DEV).to(dtype)
    w = (torch.randn(C, 1, L, generator=gen, device=DEV) / math.sqrt(L)).to(dtype)
    b = torch.randn(C, generator=gen, device=DEV).to(dtype)
    gy = torch.randn(B, C, L, generator=gen, device=DEV).to(dtype)

    def forward():
        with torch.no_grad():
            return fft_long_conv(x, w, b, groups=C, causal=True)

    def step():
        xs, ws, bs = (t.detach().clone().requires_grad_() for t in (x, w, b))
        fft_long_conv(xs, ws, bs, groups=C, causal=True).backward(gy)
        return xs.grad, ws.grad, bs.grad

    for name, fn in (("forward", forward), ("forward + backward", step)):
        fn()                                              # warm: plans and tables
        native = _added_peak(fn)
        monkeypatch.setenv("FFTCONV_HALF_IO", "0")
        fn()
        cast = _added_peak(fn)
        monkeypatch.delenv("FFTCONV_HALF_IO")
        print(f"{name} B{B} C{C} K=L={L} {dtype}: added peak native {native / 2**20:.1f} MiB, cast {cast / 2**20:.1f} MiB, "
              f"4 bytes per input sample {4 * x.numel() / 2**20:.1f} MiB")
        assert native + 4 * x.numel() <= cast, name
