"""float16 / bfloat16 training without float32 copies: autograd saves the 16-bit signal and weight, and backward reads
16-bit dY and x in the kernels themselves (fc_wgrad1d / fc_wgrad_nd with a 16-bit descriptor, the 16-bit transposed plan
of dX).

Every gradient must have exactly the bits of the cast path (FFTCONV_HALF_IO=0: widen, run the float32 function, round),
so dX, dW and db are compared bit for bit against it, in both dtypes, over the weight-gradient routes, the widened
fallbacks (forward-plan dW, refused dX plans, non-constant padding), transposed calls and the modules.  Spies show that
each case took the 16-bit route it is meant to."""
import math

import pytest
import torch

from tests import route_util as ru

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HALF = (torch.float16, torch.bfloat16)
KNOBS = ("FFTCONV_PERS", "FFTCONV_PH2", "FFTCONV_TILE", "FFTCONV_DENSE", "FFTCONV_DENSE_SLAB", "FFTCONV_PLANES",
         "FFTCONV_WIDE", "FFTCONV_DIAG", "FFTCONV_XTILE", "FFTCONV_YTILE", "FFTCONV_ZEROWRAP", "FFTCONV_NDSEG",
         "FFTCONV_HALF_IO")


def _clear():
    from fft_conv_pytorch_amd import _native, autograd, functional
    _native.clear_plan_cache()
    functional._REFUSED_HALF.clear()
    autograd._BWD_PLANS.clear()


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    _clear()
    yield
    _clear()


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)} vs {want.dtype} {tuple(want.shape)}"
    if not torch.equal(got.view(torch.int16), want.view(torch.int16)):
        diff = (got.float() - want.float()).abs().max().item()
        n = (got.view(torch.int16) != want.view(torch.int16)).sum().item()
        raise AssertionError(f"{what}: {n} samples differ from the cast path (max |diff| {diff:.3e})")


def _tensors(c, dtype, seed=0):
    gen = torch.Generator(device=DEV).manual_seed(sum(c.size) + 7 * c.B + c.cin + seed)
    x = torch.randn((c.B, c.cin) + tuple(c.size), generator=gen, device=DEV).to(dtype)
    w = (torch.randn(c.wshape, generator=gen, device=DEV) / math.sqrt(math.prod(c.wshape[1:]))).to(dtype)
    b = torch.randn(c.cout, generator=gen, device=DEV).to(dtype)
    return x, w, b, gen


def _op(c):
    from fft_conv_pytorch_amd.functional import fft_conv, fft_conv_transpose
    if c.tr:
        return lambda x, w, b: fft_conv_transpose(x, w, b, stride=c.tup(c.s), padding=c.tup(c.p),
                                                  output_padding=c.tup(c.op), dilation=c.tup(c.d), groups=c.g)
    return lambda x, w, b: fft_conv(x, w, b, stride=c.tup(c.s), padding=c.tup(c.p), dilation=c.tup(c.d), groups=c.g,
                                    padding_mode=c.mode)


class _Saved:
    """What autograd saves during a forward (saved_tensors_hooks)."""

    def __init__(self):
        self.items = []

    def __enter__(self):
        self._ctx = torch.autograd.graph.saved_tensors_hooks(self._pack, lambda t: t)
        self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        self._ctx.__exit__(*exc)

    def _pack(self, t):
        self.items.append((t.dtype, t.numel()))
        return t

    def float32_of(self, numel):
        return [it for it in self.items if it[0] == torch.float32 and it[1] == numel]


def _train_step(fn, x, w, b, gy, saved=None):
    xs, ws, bs = (t.detach().clone().requires_grad_() for t in (x, w, b))
    if saved is not None:
        with saved:
            y = fn(xs, ws, bs)
    else:
        y = fn(xs, ws, bs)
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), xs.grad, ws.grad, bs.grad


class _Spies:
    """dtype codes of the descriptors the weight-gradient entry points receive, whether the forward-plan dW ran, and the
    dtype of every plan that ran a forward launch (the forward itself, dX, forward-plan dW)."""

    def __init__(self, monkeypatch):
        from fft_conv_pytorch_amd import _native, autograd as A, functional as F_
        self.w1d, self.wnd, self.plans, self.launches = [], [], [], []
        real_db, real_init, real_plans = _native.wgrad1d_db, _native.WgradPlan.__init__, A._grad_weight_plans
        real_fwd = F_._forward_native

        def forward_native(signal, spectrum, bias):
            self.launches.append(spectrum.plan.dtype)
            return real_fwd(signal, spectrum, bias)
        monkeypatch.setattr(F_, "_forward_native", forward_native)

        def wgrad1d_db(desc, *a, **k):
            self.w1d.append(int(desc.dtype))
            return real_db(desc, *a, **k)

        def wgrad_init(obj, desc):
            self.wnd.append(int(desc.dtype))
            return real_init(obj, desc)

        def plans(x, *a, **k):
            self.plans.append(x.dtype)
            return real_plans(x, *a, **k)
        monkeypatch.setattr(_native, "wgrad1d_db", wgrad1d_db)
        monkeypatch.setattr(_native.WgradPlan, "__init__", wgrad_init)
        monkeypatch.setattr(A, "_grad_weight_plans", plans)


CODE = {torch.float16: 2, torch.bfloat16: 3}
C = ru.C
# (name, knobs, case, weight-gradient route: "w1d" fc_wgrad1d, "wnd" fc_wgrad_nd, "plans" forward plans on widened tensors)
CASES = [
    ("1d-dense-db", {}, C(2, 8, 8, (3000,), (33,), p=16), "w1d"),
    ("1d-stride3", {}, C(2, 8, 6, (3001,), (17,), s=3, p=5), "w1d"),
    ("1d-reflect", {}, C(2, 8, 8, (2000,), (9,), p=4, mode="reflect"), "w1d"),
    ("1d-replicate", {}, C(2, 6, 8, (1000,), (20,), p=3, mode="replicate"), "w1d"),
    ("1d-circular-s2", {}, C(2, 12, 8, (3000,), (31,), s=2, p=15, mode="circular"), "w1d"),
    ("1d-wgrad-segments", {}, C(1, 8, 16, (5000,), (1000,), p=5), "w1d"),
    ("1d-depthwise", {}, C(3, 16, 16, (2000,), (65,), g=16, p=32), "w1d"),
    ("1d-many-channels", {}, C(2, 72, 72, (600,), (5,), p=2), "plans"),
    ("2d-separable", {"FFTCONV_PLANES": "0"}, C(2, 4, 6, (30, 44), (5, 3), s=(2, 1), p=(1, 2), g=2), "wnd"),
    ("2d-default", {}, C(2, 3, 4, (40, 60), (9, 11), p=2), "wnd"),
    ("3d-plane-major", {}, C(2, 3, 4, (17, 19, 23), (3, 5, 3), p=1), "wnd"),
    ("3d-separable-strided", {"FFTCONV_PLANES": "0"}, C(2, 4, 4, (12, 14, 16), (3, 3, 3), s=2, p=1), "wnd"),
    ("1d-transposed", {}, C(2, 4, 6, (1001,), (33,), s=3, p=5, op=1, tr=True), "w1d"),
    ("2d-transposed", {}, C(2, 4, 6, (20, 24), (3, 5), s=2, p=1, op=1, tr=True), "wnd"),
]


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("name,env,c,route", CASES, ids=[cs[0] for cs in CASES])
def test_gradient_bits_match_cast_path(name, env, c, route, dtype, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    x, w, b, gen = _tensors(c, dtype)
    fn = _op(c)
    with torch.no_grad():
        gy = torch.randn(fn(x, w, b).shape, generator=gen, device=DEV).to(dtype)
    spies = _Spies(monkeypatch)
    saved = _Saved()
    got = _train_step(fn, x, w, b, gy, saved)
    assert not saved.float32_of(x.numel()), f"{name}: a float32 copy of the signal was saved"
    if route == "w1d":
        assert spies.w1d and all(code == CODE[dtype] for code in spies.w1d), f"{name}: fc_wgrad1d got {spies.w1d}"
    elif route == "wnd":
        assert spies.wnd and all(code == CODE[dtype] for code in spies.wnd), f"{name}: fc_wgrad_nd got {spies.wnd}"
    else:
        assert spies.plans and not spies.w1d and not spies.wnd, name
    # the forward and, under zero padding, dX ran 16-bit plans; reflect / replicate / circular dX widens dY (one float32 plan)
    widened = [dt for dt in spies.launches if dt != dtype]
    if c.mode == "constant" and route != "plans":
        assert len(spies.launches) >= 2 and not widened, f"{name}: forward launches ran plans of {spies.launches}"
    elif route != "plans":
        assert widened == [torch.float32] and spies.launches[0] == dtype, f"{name}: {spies.launches}"
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    want = _train_step(fn, x, w, b, gy)
    for part, g_, w_ in zip(("y", "dX", "dW", "db"), got, want):
        _same_bits(g_, w_, f"{name} {dtype} {part}")


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
def test_saved_tensors_are_16bit(dtype):
    """fft_conv, fft_conv_transpose and a training module save 16-bit tensors: nothing float32 of the signal's size."""
    from fft_conv_pytorch_amd import FFTConv1d
    from fft_conv_pytorch_amd.functional import fft_conv, fft_conv_transpose
    torch.manual_seed(0)
    x = torch.randn(2, 8, 3000, device=DEV).to(dtype).requires_grad_()
    w = (torch.randn(8, 8, 33, device=DEV) / 16).to(dtype).requires_grad_()
    wt = (torch.randn(8, 4, 33, device=DEV) / 16).to(dtype).requires_grad_()
    b = torch.randn(8, device=DEV).to(dtype).requires_grad_()
    layer = FFTConv1d(8, 8, 33, padding=16).to(DEV).to(dtype).train()
    calls = {"fft_conv": lambda: fft_conv(x, w, b, padding=16),
             "fft_conv_transpose": lambda: fft_conv_transpose(x, wt, None, stride=2, padding=3, output_padding=1),
             "module": lambda: layer(x)}
    for name, call in calls.items():
        saved = _Saved()
        with saved:
            y = call()
        assert y.dtype == dtype, name
        assert saved.items, f"{name}: nothing saved for backward"
        assert not saved.float32_of(x.numel()), f"{name} saved a float32 copy of the signal: {saved.items}"
        assert any(dt == dtype and n == x.numel() for dt, n in saved.items), f"{name}: {saved.items}"
        y.float().sum().backward()
        assert x.grad.dtype == dtype
        x.grad = None


def test_library_takes_16bit_weight_gradient_descriptors():
    """fc_wgrad1d_slices and fc_wgrad_nd_plan_create accept float16 / bfloat16 descriptors, sized as the float32 ones."""
    from fft_conv_pytorch_amd import _native
    one = (1, 4, 8, 8, 1, (4096,), (33,), (1,), (0,), (1,), 0)
    with torch.cuda.device(0):
        s32 = _native.wgrad1d_slices(_native.conv_desc(*one))
        s16 = _native.wgrad1d_slices(_native.conv_desc(*one, dtype=3))
        assert s16 > 0 and s16 == s32
        assert _native.wgrad1d_slices(_native.conv_desc(*one, dtype=2)) == s32
        assert _native.wgrad1d_db_supported(_native.conv_desc(*one, dtype=3))
        two = (2, 4, 8, 8, 1, (64, 64), (3, 3), (1, 1), (1, 1), (1, 1), 0)
        p32 = _native.WgradPlan(_native.conv_desc(*two))
        p16 = _native.WgradPlan(_native.conv_desc(*two, dtype=2))
        assert (p16.spectrum_bytes, p16.workspace_bytes, p16.tile) == (p32.spectrum_bytes, p32.workspace_bytes, p32.tile)
        with pytest.raises(NotImplementedError):
            _native.WgradPlan(_native.conv_desc(*two, dtype=1))      # float64 x / dY: not a weight-gradient plan


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("n,taps", [(2, "8"), (3, "4")])
def test_nd_weight_gradient_segments_of_taps(n, taps, dtype, monkeypatch):
    """A weight-gradient plan cut into segments of taps adds into its float32 dW: 16-bit x / dY give the float32 bits."""
    from fft_conv_pytorch_amd import autograd as A
    monkeypatch.setenv("FFTCONV_NDSEG", taps)
    monkeypatch.setenv("FFTCONV_PLANES", "0")
    size, k = ((30, 40), (3, 5)) if n == 2 else ((10, 12, 14), (3, 3, 3))
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn((2, 4) + size, generator=gen, device=DEV).to(dtype)
    lo = tuple(s + 2 - kk + 1 for s, kk in zip(size, k))
    gy = torch.randn((2, 6) + lo, generator=gen, device=DEV).to(dtype)
    args = ((6, 4) + k, (1,) * n, (1,) * n, (1,) * n, 1, "constant")
    got = A._grad_weight_nd_native(x, gy, *args)
    want = A._grad_weight_nd_native(x.float(), gy.float(), *args)
    assert got is not None and want is not None
    assert torch.equal(got, want), f"max |diff| {(got - want).abs().max().item():.3e}"


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
def test_refused_dx_plan_widens(dtype):
    """dX of a shape whose 16-bit transposed plan is refused (1-D segments of taps): widened dY, float32 plan, one
    rounding."""
    from fft_conv_pytorch_amd import autograd as A, functional as F_
    gen = torch.Generator(device=DEV).manual_seed(9)
    c = C(2, 8, 8, (20000,), (5000,))
    w = (torch.randn(c.wshape, generator=gen, device=DEV) / 100).to(dtype)
    gy = torch.randn(2, 8, 20000 - 5000 + 1, generator=gen, device=DEV).to(dtype)
    args = ((20000,), (1,), (0,), (1,), 1, "constant")
    got = A._grad_input(gy, w, *args)
    assert F_._REFUSED_HALF, "the 16-bit dX plan of this shape was expected to be refused"
    want = A._grad_input(gy.float(), w.float(), *args).to(dtype)
    _same_bits(got, want, "refused dX")


MODULES = [
    ("FFTConv1d", lambda m: m.FFTConv1d(8, 8, 65, padding=32), (2, 8, 3000)),
    ("FFTConv1d-reflect", lambda m: m.FFTConv1d(8, 8, 9, padding=4, padding_mode="reflect"), (2, 8, 2000)),
    ("FFTConv2d", lambda m: m.FFTConv2d(4, 6, (5, 3), padding=(2, 1)), (2, 4, 30, 40)),
    ("FFTConv3d", lambda m: m.FFTConv3d(3, 4, 3, padding=1), (2, 3, 12, 14, 16)),
    ("FFTConvTranspose1d", lambda m: m.FFTConvTranspose1d(8, 4, 33, stride=2, padding=5, output_padding=1), (2, 8, 700)),
    ("FFTConvTranspose2d", lambda m: m.FFTConvTranspose2d(4, 6, (3, 5), stride=2, padding=1, output_padding=1), (2, 4, 20, 24)),
]


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("name,make,shape", MODULES, ids=[m[0] for m in MODULES])
def test_module_training_bits(name, make, shape, dtype, monkeypatch):
    import fft_conv_pytorch_amd as fca
    torch.manual_seed(1)
    layer = make(fca).to(DEV).to(dtype).train()
    x = torch.randn(shape, device=DEV).to(dtype)

    def step():
        layer.zero_grad(set_to_none=True)
        xs = x.clone().requires_grad_()
        saved = _Saved()
        with saved:
            y = layer(xs)
        y.backward(gy)
        torch.cuda.synchronize()
        return saved, (y.detach(), xs.grad, layer.weight.grad, layer.bias.grad)

    with torch.no_grad():
        gy = torch.randn(layer(x).shape, device=DEV).to(dtype)
    saved, got = step()
    assert not saved.float32_of(x.numel()), f"{name}: a float32 copy of the signal was saved"
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    _, want = step()
    for part, g_, w_ in zip(("y", "dX", "dW", "db"), got, want):
        _same_bits(g_, w_, f"{name} {dtype} {part}")


def test_peak_memory_training_step(monkeypatch):
    """cfgA-sized bf16 forward + backward: the native step raises the peak by at least 4 bytes per input sample less than
    the cast path does."""
    from fft_conv_pytorch_amd import FFTConv1d
    torch.manual_seed(0)
    layer = FFTConv1d(8, 8, 512, bias=True).to(DEV).to(torch.bfloat16).train()
    x = torch.randn(32, 8, 32768, device=DEV).to(torch.bfloat16).requires_grad_()
    with torch.no_grad():
        gy = torch.randn(layer(x).shape, device=DEV).to(torch.bfloat16)

    def peak():
        for _ in range(2):          # the second run is measured (plans, twiddles and the allocator warm)
            layer.zero_grad(set_to_none=True)
            x.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            layer(x).backward(gy)
            torch.cuda.synchronize()
            grow = torch.cuda.max_memory_allocated() - base
        return grow

    native = peak()
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    cast = peak()
    assert native + 4 * x.numel() <= cast, f"native step peak +{native} B, cast path +{cast} B, x has {x.numel()} samples"


def test_graph_captured_training_step():
    """One bf16 training step of FFTConv1d captured with torch.cuda.graph and replayed gives the eager step's bits."""
    from fft_conv_pytorch_amd import FFTConv1d
    torch.manual_seed(2)
    layer = FFTConv1d(8, 8, 65, padding=32, bias=True).to(DEV).to(torch.bfloat16).train()
    x = torch.randn(4, 8, 9000, device=DEV).to(torch.bfloat16).requires_grad_()
    gy = torch.randn(4, 8, 9000, device=DEV).to(torch.bfloat16)

    def step():
        y = layer(x)
        y.backward(gy)
        return y

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                       # warm: plans, twiddles, work lists, allocator pools
            layer.zero_grad(set_to_none=True)
            x.grad = None
            want_y = step().detach().clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want = (want_y, x.grad.clone(), layer.weight.grad.clone(), layer.bias.grad.clone())
    layer.zero_grad(set_to_none=True)
    x.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = step()
    g.replay()
    torch.cuda.synchronize()
    for part, g_, w_ in zip(("y", "dX", "dW", "db"), (y, x.grad, layer.weight.grad, layer.bias.grad), want):
        _same_bits(g_.detach(), w_, f"graph replay {part}")
