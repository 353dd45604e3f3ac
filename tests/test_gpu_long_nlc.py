"""(batch, length, channels) tensors through ``fft_long_conv`` / ``FFTLongConv1d``: a signal that is the transposed view of
a contiguous (B, L, C) tensor is read where it lies, ``channels_last=True`` has the column kernels write y that way, and
backward reads a dY that lies so and writes dX in the signal's layout (csrc/long1d.hpp, the channels-last builds).

The yardstick is bits.  A row's arithmetic does not depend on which workgroup slot runs it, so every result must equal,
bit for bit, the same call on ``.contiguous()`` tensors with ``channels_last=False`` -- the existing path, which has its own
tests against the oracle.  A spy on ``LongPlan.forward_lay`` shows that the kernels, not torch copies, served the layouts."""
import copy
import math
import pickle

import pytest
import torch

from fft_conv_pytorch_amd import FFTLongConv1d, _native, autograd, fft_long_conv
from fft_conv_pytorch_amd import functional as F_
from tests import guard_util as gu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F16, BF16, C64 = torch.float32, torch.float16, torch.bfloat16, torch.complex64
DTYPES = (F32, F16, BF16, C64)
KNOBS = ("FFTCONV_LONG_N", "FFTCONV_LONG_WS_MB", "FFTCONV_HALF_IO", "FFTCONV_TILE", "FFTCONV_LONG_NLC")
NCL, NLC = _native.LONG_NCL, _native.LONG_NLC
COMBOS = [(False, False), (True, False), (False, True), (True, True)]      # (strided signal, channels_last)


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
def lay(monkeypatch):
    """(x_layout, y_layout) of every ``LongPlan.forward_lay`` call."""
    calls = []
    real = _native.LongPlan.forward_lay

    def forward_lay(plan, x_ptr, spectrum_ptr, bias_ptr, y_ptr, workspace_ptr, stream, x_dtype=0, y_dtype=0,
                    x_layout=NCL, y_layout=NCL):
        calls.append((x_layout, y_layout))
        return real(plan, x_ptr, spectrum_ptr, bias_ptr, y_ptr, workspace_ptr, stream, x_dtype, y_dtype, x_layout, y_layout)
    monkeypatch.setattr(_native.LongPlan, "forward_lay", forward_lay)
    return calls


def _randn(shape, dtype, gen):
    if dtype == C64:
        return torch.complex(torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)).to(DEV)
    return torch.randn(shape, generator=gen).to(DEV).to(dtype)


def _tensors(B, cin, cout, g, L, K, bias, dtype, seed=0):
    """u (B, L, Cin) contiguous -- the user's tensor --, weight scaled so that outputs are of order one, bias."""
    gen = torch.Generator().manual_seed(seed + L + 3 * K + 7 * cin)
    u = _randn((B, L, cin), dtype, gen)
    w = _randn((cout, cin // g, K), dtype, gen) * (1.0 / math.sqrt(cin // g * K))
    b = _randn((cout,), dtype, gen) if bias else None
    return u, w.to(dtype), b


def _strides_nlc(t):
    return tuple(t.stride()) == (t.shape[1] * t.shape[2], 1, t.shape[1])


def _check_combos(fn, u, what, lay_calls=None, native=True):
    """``fn(signal, channels_last)`` for the four layout combinations against the contiguous call."""
    x = u.transpose(1, 2)
    assert F_._long_layout(x) in ("nlc", "ncl")
    want = fn(x.contiguous(), False)
    assert want.is_contiguous()
    for strided, cl in COMBOS:
        if lay_calls is not None:
            lay_calls.clear()
        got = fn(x if strided else x.contiguous(), cl)
        tag = f"{what}: strided signal {strided}, channels_last {cl}"
        if cl:
            assert _strides_nlc(got) and got.transpose(1, 2).is_contiguous(), (tag, got.stride())
        else:
            assert got.is_contiguous(), tag
        gu.same_bits(got, want, tag)
        if lay_calls is not None and native:
            x_nlc = strided and F_._long_layout(x) == "nlc"
            assert lay_calls == ([(NLC if x_nlc else NCL, NLC if cl else NCL)] if (x_nlc or cl) else []), (tag, lay_calls)
    return want


# ------------------------------------------------------------------------------------------------ forward
FORCED_N1 = [64, 128, 256, 512, 1024, 2048, 4096]


def _forced(N1, N2, dtype, monkeypatch, lay):
    """B = 3 (a last pair without a second item), C = 5 depthwise (a tail channel block at every NC > 1), L + K - 1 fills
    the transform, bias on."""
    monkeypatch.setenv("FFTCONV_LONG_N", f"{N1}x{N2}")
    _clear()
    N = N1 * N2
    B, C, K = 3, 5, N // 4
    L = N - K + 1
    u, w, b = _tensors(B, C, C, C, L, K, True, dtype)
    if N <= F_.LONG_HANDOFF_POINTS and dtype != C64:
        # (a real row this short hands off to fft_conv: the primitive itself, as the causal call runs it)
        fn = lambda x, cl: F_._long_run(x, w, b, K - 1, 0, True, L, C, channels_last=cl)            # noqa: E731
    else:
        fn = lambda x, cl: fft_long_conv(x, w, b, groups=C, causal=True, channels_last=cl)           # noqa: E731
    want = _check_combos(fn, u, f"{N1}x{N2} {dtype}", lay)
    assert want.shape == (B, C, L) and L % 2 == 1
    plan = F_._long_plan(u.transpose(1, 2), C, C, K, K - 1, 0, True, L, True)
    assert (plan.info["N1"], plan.info["N2"]) == (N1, N2)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("N1", FORCED_N1)
def test_forced_factorisations(N1, dtype, monkeypatch, lay):
    _forced(N1, 64, dtype, monkeypatch, lay)


def test_forced_factorisation_with_long_rows_of_the_workspace(monkeypatch, lay):
    _forced(64, 4096, F32, monkeypatch, lay)


PICKED = [
    # B, cin, cout, g, L, K, bias, kw  (the row needs just over 4096 points: N = 8192)
    (1, 2, 2, 2, 2100, 2100, True, dict(causal=True)),
    (2, 3, 3, 3, 2100, 2100, False, dict(causal=True)),
    (1, 8, 8, 8, 2100, 2100, False, dict(causal=True)),
    (2, 17, 17, 17, 2100, 2100, True, dict(causal=True)),
    (1, 17, 17, 17, 2100, 2100, True, dict(causal=True)),
    (2, 8, 8, 8, 2101, 2000, True, dict(causal=True)),
    (2, 6, 4, 2, 4000, 301, True, dict(padding=100)),                       # grouped: Cig 3, Cog 2
    (2, 4, 6, 1, 4000, 301, False, dict(padding=100)),                      # dense 4 -> 6
    (2, 3, 3, 3, 2500, 3000, True, dict(causal=True)),                      # causal with K > L
    (2, 3, 5, 1, 4000, 301, True, dict(padding="same")),
    (2, 3, 3, 1, 4000, 201, True, dict(padding=100, padding_mode="reflect")),
    (1, 5, 5, 5, 4000, 201, False, dict(padding=100, padding_mode="replicate")),
    (2, 2, 4, 2, 4000, 201, True, dict(padding=100, padding_mode="circular")),
    (2, 3, 3, 3, 4301, 101, True, dict(stride=2)),
    (1, 4, 2, 2, 4301, 101, False, dict(stride=3, padding=7)),
    (2, 3, 3, 1, 4301, 101, True, dict(dilation=2)),
    (2, 3, 3, 3, 4200, 2000, True, dict(causal=True, stride=2, dilation=2)),
]


@pytest.mark.parametrize("B,cin,cout,g,L,K,bias,kw", PICKED, ids=[f"{i}" for i in range(len(PICKED))])
def test_planner_picked_shapes(B, cin, cout, g, L, K, bias, kw, lay):
    for dtype in (F32, BF16) if cin != 17 else DTYPES:
        u, w, b = _tensors(B, cin, cout, g, L, K, bias, dtype)
        fn = lambda x, cl: fft_long_conv(x, w, b, groups=g, channels_last=cl, **kw)                  # noqa: E731
        _check_combos(fn, u, f"B{B} {cin}->{cout} g{g} L{L} K{K} {kw} {dtype}", lay)


@pytest.mark.parametrize("dtype", (F32, BF16, C64), ids=str)
def test_signal_at_a_storage_offset(dtype, lay):
    B, C, L, K = 2, 5, 2100, 2100
    big, w, b = _tensors(B + 1, C, C, C, L, K, True, dtype)
    x = big[1:].transpose(1, 2)
    assert x.storage_offset() == L * C and F_._long_layout(x) == "nlc"
    want = fft_long_conv(x.contiguous(), w, b, groups=C, causal=True)
    before = big.clone()
    got = fft_long_conv(x, w, b, groups=C, causal=True, channels_last=True)
    assert lay == [(NLC, NLC)]
    gu.same_bits(got, want, f"storage offset {dtype}")
    gu.same_bits(big, before, "the buffer the signal is a view of")
    # an offset that is only element-aligned
    flat = torch.zeros(B * L * C + 1, dtype=dtype, device=DEV)
    flat[1:] = big[:B].reshape(-1)
    odd = flat[1:].view(B, L, C).transpose(1, 2)
    gu.same_bits(fft_long_conv(odd, w, b, groups=C, causal=True), fft_long_conv(odd.contiguous(), w, b, groups=C, causal=True),
                 f"odd storage offset {dtype}")
    assert lay[-1] == (NLC, NCL)


@pytest.mark.parametrize("dtype", (F32, BF16, C64), ids=str)
def test_slabs_give_the_bits_of_one_slab(dtype, monkeypatch, lay):
    B, C, L, K = 5, 5, 2100, 2100
    u, w, b = _tensors(B, C, C, C, L, K, True, dtype)
    x = u.transpose(1, 2)
    one = fft_long_conv(x.contiguous(), w, b, groups=C, causal=True)
    monkeypatch.setenv("FFTCONV_LONG_WS_MB", "1")        # 8192 points x 10 channels x 8 bytes = 640 KiB per pair / item
    _clear()
    plan = F_._long_plan(x, C, C, K, K - 1, 0, True, L, True)
    assert plan.info["slabs"] == (5 if dtype == C64 else 3) and plan.info["slab_pairs"] == 1
    lay.clear()
    got = fft_long_conv(x, w, b, groups=C, causal=True, channels_last=True)
    assert lay == [(NLC, NLC)]
    gu.same_bits(got, one, f"slabs {dtype}")


def test_short_rows_and_the_knob_keep_values_and_strides(monkeypatch, lay):
    # rows that hand off to fft_conv (need <= 4096): torch copies, the requested strides
    for dtype in (F32, BF16):
        u, w, b = _tensors(3, 5, 5, 5, 1501, 700, True, dtype)
        for kw in (dict(causal=True), dict(padding=300)):
            fn = lambda x, cl: fft_long_conv(x, w, b, groups=5, channels_last=cl, **kw)              # noqa: E731
            _check_combos(fn, u, f"short {kw} {dtype}", lay, native=False)
        assert lay == []
    # the long path under FFTCONV_LONG_NLC=0, and the FFTCONV_HALF_IO=0 cast path
    for dtype, env in ((F32, {}), (C64, {}), (BF16, {}), (BF16, {"FFTCONV_HALF_IO": "0"})):
        u, w, b = _tensors(3, 5, 5, 5, 2100, 2100, True, dtype)
        fn = lambda x, cl: fft_long_conv(x, w, b, groups=5, causal=True, channels_last=cl)           # noqa: E731
        want = fn(u.transpose(1, 2).contiguous(), False)
        monkeypatch.setenv("FFTCONV_LONG_NLC", "0")
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        lay.clear()
        gu.same_bits(_check_combos(fn, u, f"FFTCONV_LONG_NLC=0 {env} {dtype}", lay, native=False), want, f"knob {dtype}")
        assert lay == []
        monkeypatch.delenv("FFTCONV_LONG_NLC")
        for k in env:
            monkeypatch.delenv(k)
        if env:      # the cast path with the kernels' layouts: float32 launches, strides kept by the rounding pass
            monkeypatch.setenv("FFTCONV_HALF_IO", "0")
            _check_combos(fn, u, f"FFTCONV_HALF_IO=0 {dtype}", lay)
            monkeypatch.delenv("FFTCONV_HALF_IO")


# ------------------------------------------------------------------------------------------------ gradients
def _step(x, w, b, cl, kw, gy=None, downstream=None):
    """One training step on leaves with the strides of ``x`` -> (y, dX, dW, db, the dY that reached the function)."""
    xs = x.detach().clone(memory_format=torch.preserve_format).requires_grad_()
    assert xs.stride() == x.stride()
    ws, bs = w.detach().clone().requires_grad_(), b.detach().clone().requires_grad_()
    y = fft_long_conv(xs, ws, bs, channels_last=cl, **kw)
    seen = []
    y.register_hook(seen.append)
    if downstream is not None:
        M, G = downstream
        (y.transpose(1, 2) @ M).backward(G)
    else:
        y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), xs.grad, ws.grad, bs.grad, seen[0]


GRAD_KW = [
    ("causal", 3, 5, 5, 5, 2100, 2100, dict(causal=True)),
    ("grouped", 2, 6, 4, 2, 4000, 301, dict(padding=100)),
    ("reflect fold", 2, 3, 3, 1, 4000, 201, dict(padding=100, padding_mode="reflect")),
    ("stride 2", 3, 5, 5, 5, 4301, 101, dict(stride=2)),
]


@pytest.mark.parametrize("dtype", (F32, BF16, C64), ids=str)
@pytest.mark.parametrize("name,B,cin,cout,g,L,K,kw", GRAD_KW, ids=[c[0] for c in GRAD_KW])
def test_gradient_bits_and_strides(name, B, cin, cout, g, L, K, kw, dtype, lay):
    u, w, b = _tensors(B, cin, cout, g, L, K, True, dtype)
    kw = dict(kw, groups=g)
    x = u.transpose(1, 2)
    with torch.no_grad():
        shape = fft_long_conv(x, w, b, **kw).shape
    gen = torch.Generator().manual_seed(1)
    gy = _randn(shape, dtype, gen)
    want = _step(x.contiguous(), w, b, False, kw, gy)
    assert want[1].is_contiguous()
    for strided, cl in COMBOS[1:]:
        lay.clear()
        xin = x if strided else x.contiguous()
        # (a dY with the strides of y, as autograd would deliver it from an elementwise consumer)
        got = _step(xin, w, b, cl, kw, F_._as_channels_last(gy) if cl else gy)
        tag = f"{name} {dtype}: strided signal {strided}, channels_last {cl}"
        for what, a, r in zip(("y", "dX", "dW", "db"), got, want):
            gu.same_bits(a, r, f"{tag}: {what}")
        assert got[1].stride() == xin.stride(), (tag, got[1].stride())
        assert got[2].is_contiguous() and got[3].is_contiguous()
        # forward in the call's layouts; dX reads dY as it lies and is written as the signal lies (with a padding mode to
        # fold, torch restores the layout after the fold); dW runs on torch's transposed copies
        x_lay, y_lay = NLC if strided else NCL, NLC if cl else NCL
        expect = [(x_lay, y_lay), (y_lay, x_lay)]
        assert lay == expect, (tag, lay)


@pytest.mark.parametrize("dtype", (F32, BF16, C64), ids=str)
def test_dy_delivered_strided_by_a_downstream_matmul(dtype, lay):
    B, C, L, K = 3, 5, 2100, 2100
    u, w, b = _tensors(B, C, C, C, L, K, True, dtype)
    kw = dict(groups=C, causal=True)
    gen = torch.Generator().manual_seed(2)
    M, G = _randn((C, 7), dtype, gen), _randn((B, L, 7), dtype, gen)
    x = u.transpose(1, 2)
    for strided, cl in COMBOS:
        lay.clear()
        xin = x if strided else x.contiguous()
        got = _step(xin, w, b, cl, kw, downstream=(M, G))
        dy = got[4]
        assert F_._long_layout(dy) == "nlc", "the matmul's gradient reaches the function as a transposed view"
        assert lay[-1] == (NLC, NLC if strided else NCL), lay
        want = _step(x.contiguous(), w, b, False, kw, dy.contiguous())
        for what, a, r in zip(("y", "dX", "dW", "db"), got, want):
            gu.same_bits(a, r, f"downstream matmul {dtype}, strided signal {strided}, channels_last {cl}: {what}")
        assert got[1].stride() == xin.stride()


# ------------------------------------------------------------------------------------------------ module
@pytest.mark.parametrize("dtype", (F32, BF16), ids=str)
def test_module_cache_and_bits(dtype, monkeypatch, lay):
    torch.manual_seed(0)
    layer = FFTLongConv1d(5, 5, 2100, groups=5, causal=True, channels_last=True).to(DEV)
    with torch.no_grad():
        layer.weight.mul_(1.0 / math.sqrt(2100) / layer.weight.std())
    layer = layer.to(dtype)
    u = torch.randn(3, 2100, 5, device=DEV).to(dtype)
    x = u.transpose(1, 2)
    want = fft_long_conv(x.contiguous(), layer.weight.detach(), layer.bias.detach(), groups=5, causal=True)
    calls = []
    real = F_.transform_kernel
    monkeypatch.setattr(F_, "transform_kernel", lambda plan, kernel: calls.append(kernel.dtype) or real(plan, kernel))
    layer.eval()
    with torch.no_grad():
        y1, y2 = layer(x), layer(x)
    assert calls == [dtype], calls                      # one kernel transform for two calls
    assert lay == [(NLC, NLC)] * 2
    for y in (y1, y2):
        assert _strides_nlc(y)
        gu.same_bits(y, want, f"module {dtype}")
    for other in (copy.deepcopy(layer), pickle.loads(pickle.dumps(layer))):
        assert other.channels_last is True
        with torch.no_grad():
            gu.same_bits(other(x), want, "copied module")
    layer.train()
    xs = x.detach().clone(memory_format=torch.preserve_format).requires_grad_()
    y = layer(xs)
    assert _strides_nlc(y)
    gu.same_bits(y.detach(), want, "module in training")
    gy = torch.randn(want.shape, generator=torch.Generator().manual_seed(3)).to(DEV).to(dtype)
    y.backward(F_._as_channels_last(gy))
    ref = _step(x.contiguous(), layer.weight.detach(), layer.bias.detach(), False, dict(groups=5, causal=True), gy)
    gu.same_bits(xs.grad, ref[1], "module dX")
    gu.same_bits(layer.weight.grad, ref[2], "module dW")
    gu.same_bits(layer.bias.grad, ref[3], "module db")
    assert xs.grad.stride() == xs.stride()


# ------------------------------------------------------------------------------------------------ memory discipline
RUNS = (0x00, 0xFF, 0x7F, 0x00)


@pytest.mark.parametrize("dtype", (F32, BF16, C64), ids=str)
def test_strided_call_and_backward_between_guard_bands(dtype, monkeypatch, lay):
    """Strided in, strided out, forward and backward, every torch.empty poisoned, the caller's tensors between guard bands:
    no byte outside a tensor changes and the runs agree bit for bit, so every sample of y and dX is written.  B = 3, C = 5
    at 256 x 64: the tail channel block and the pair without a partner are the cases under guard."""
    monkeypatch.setenv("FFTCONV_LONG_N", "256x64")
    _clear()
    B, C, N = 3, 5, 256 * 64
    K = N // 4
    L = N - K + 1
    u, w, b = _tensors(B, C, C, C, L, K, True, dtype)
    gy = _randn((B, L, C), dtype, torch.Generator().manual_seed(4))
    want = _step(u.transpose(1, 2).contiguous(), w, b, False, dict(groups=C, causal=True), gy.transpose(1, 2).contiguous())[:4]
    first = None
    for n, pattern in enumerate(RUNS):
        pairs = [gu.guarded(t, pattern) for t in (u, w, b, gy)]
        ug, wg, bg, gyg = (p[0] for p in pairs)
        lay.clear()
        with gu.guarded_empty(pattern) as ge:
            xs = ug.transpose(1, 2).detach().requires_grad_()
            ws, bs = wg.detach().requires_grad_(), bg.detach().requires_grad_()
            y = fft_long_conv(xs, ws, bs, groups=C, causal=True, channels_last=True)
            y.backward(gyg.transpose(1, 2))
            out = (y.detach(), xs.grad, ws.grad, bs.grad)
        tag = f"{dtype}, run {n} ({pattern:#04x})"
        assert lay[:2] == [(NLC, NLC), (NLC, NLC)], (tag, lay)
        assert ge.served and ge.violations() == [], f"{tag}: guard bytes of a library buffer changed: {ge.violations()}"
        for i, (_, check) in enumerate(pairs):
            assert check() == [], f"{tag}: input {i} or its guards changed: {check()}"
        assert _strides_nlc(out[0]) and _strides_nlc(out[1])
        for what, a, r in zip(("y", "dX", "dW", "db"), out, want):
            gu.same_bits(a, r, f"{tag}: {what} against the contiguous call")
        if first is None:
            first = out
        for what, a, r in zip(("y", "dX", "dW", "db"), out, first):
            gu.same_bits(a, r, f"{tag}: {what} against the first run")


def _added_peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def test_no_hidden_copy(monkeypatch, lay):
    """Derived, not measured: the copy path holds the signal's contiguous copy alive across the launches (and a second y
    while it transposes the result), the native call allocates y, the workspace and the spectrum and nothing else.  Every
    size is a multiple of 2 MiB, so the allocator adds only its 512-byte rounding."""
    B, C, L = 4, 64, 16384
    gen = torch.Generator(device=DEV).manual_seed(0)
    u = torch.randn(B, L, C, generator=gen, device=DEV)
    w = torch.randn(C, 1, L, generator=gen, device=DEV) / math.sqrt(L)
    b = torch.randn(C, generator=gen, device=DEV)
    x = u.transpose(1, 2)

    def forward():
        with torch.no_grad():
            return fft_long_conv(x, w, b, groups=C, causal=True, channels_last=True)
    want = forward()                                      # warm: plan and tables
    plan = F_._long_plan(x, C, C, L, L - 1, 0, True, L, True)
    assert lay == [(NLC, NLC)]
    native = _added_peak(forward)
    monkeypatch.setenv("FFTCONV_LONG_NLC", "0")
    gu.same_bits(forward(), want, "copy path")
    copied = _added_peak(forward)
    monkeypatch.delenv("FFTCONV_LONG_NLC")
    nbytes = x.numel() * x.element_size()
    bound = want.numel() * want.element_size() + plan.workspace_bytes + plan.spectrum_bytes + 3 * 512
    print(f"B{B} C{C} K=L={L}: added peak native {native / 2**20:.1f} MiB, copy path {copied / 2**20:.1f} MiB, "
          f"signal {nbytes / 2**20:.1f} MiB, y + workspace + spectrum {bound / 2**20:.1f} MiB")
    assert native <= copied - nbytes
    assert native <= bound


# ------------------------------------------------------------------------------------------------ library
def test_library_answers():
    C, L, K = 5, 2100, 2100
    u, w, b = _tensors(2, C, C, C, L, K, True, F32)
    x = u.transpose(1, 2)
    plan = F_._long_plan(x, C, C, K, K - 1, 0, True, L, True)
    spectrum = F_.transform_kernel(plan, w)
    ws = F_.new_workspace(plan, x.device)
    out = torch.empty(2, L, C, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    args = (x.data_ptr(), spectrum.buf.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), stream, 0, 0)
    with pytest.raises(ValueError, match="x has layout code 7"):
        plan.forward_lay(*args, 7, NLC)
    with pytest.raises(ValueError, match="y has layout code -1"):
        plan.forward_lay(*args, NLC, -1)
    plan.forward_lay(*args, NLC, NLC)
    torch.cuda.synchronize()
    gu.same_bits(out.transpose(1, 2), fft_long_conv(x.contiguous(), w, b, groups=C, causal=True), "C level")
    # one batch item's (L, C) block of 2^31 bytes: refused before any pointer is used (none of these tensors has that size)
    big_c, big_l = 4096, 1 << 17
    key = ("long", 1, big_c, big_c, big_c, big_l, 4097, 4096, 0, big_l, 1, 0)
    big = _native.get_plan(0, key)
    assert big.out_len * big_c * 4 == 1 << 31
    with pytest.raises(NotImplementedError, match=r"x in the channels-last layout.*2147483648 bytes"):
        big.forward_lay(*args, NLC, NCL)
    with pytest.raises(NotImplementedError, match=r"y in the channels-last layout.*2147483648 bytes"):
        big.forward_lay(*args, NCL, NLC)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ capture
@pytest.mark.parametrize("dtype", (F32, BF16), ids=str)
def test_warm_strided_call_is_capturable_and_replays_bit_for_bit(dtype):
    B, C, L = 3, 5, 20001
    u, w, b = _tensors(B, C, C, C, L, L, True, dtype)
    plan = F_._long_plan(u.transpose(1, 2), C, C, L, L - 1, 0, True, L, True)
    assert plan.info["slabs"] == 1
    spectrum = F_.transform_kernel(plan, w)
    static_u = u.clone()
    static_x = static_u.transpose(1, 2)
    fft_long_conv(static_x, w, b, groups=C, causal=True, channels_last=True)       # warm: plan and device tables exist
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = F_._long_run(static_x, w, b, L - 1, 0, True, L, C, spectrum, channels_last=True)
    assert static_y.dtype == dtype and _strides_nlc(static_y)
    for seed in (1, 2, 3):
        fresh = torch.randn(u.shape, generator=torch.Generator().manual_seed(seed)).to(DEV).to(dtype)
        static_u.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        eager = F_._long_run(fresh.transpose(1, 2).contiguous(), w, b, L - 1, 0, True, L, C, spectrum)
        gu.same_bits(static_y, eager, f"replay {seed} {dtype}")
