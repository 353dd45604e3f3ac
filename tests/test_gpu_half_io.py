"""float16 / bfloat16 signals read and outputs written by the forward kernels themselves (fc_dtype FC_F16 / FC_BF16).

The kernels widen x exactly as they load it and round y once as they store it, so every result must have the bits of the
cast path: x.float() through the float32 plan of the same descriptor, then .to(dtype).  Checked for every float32 route of
tests/route_util.py that a half plan may take (same route and spectrum signature as the float32 plan), for the routes it
refuses (named, and fft_conv falls back to the cast path), for the memory a call holds, for unaligned and odd-sized
tensors, for special values and for the modules."""
import math

import pytest
import torch

from tests import route_util as ru

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HALF = (torch.float16, torch.bfloat16)
KNOBS = ("FFTCONV_PERS", "FFTCONV_PH2", "FFTCONV_TILE", "FFTCONV_DENSE", "FFTCONV_DENSE_SLAB", "FFTCONV_PLANES",
         "FFTCONV_WIDE", "FFTCONV_DIAG", "FFTCONV_XTILE", "FFTCONV_YTILE", "FFTCONV_F64_FFT", "FFTCONV_ZEROWRAP",
         "FFTCONV_NDSEG", "FFTCONV_HALF_IO")
REFUSED_ROUTES = ("1d-chunk-launches", "1d-segments", "1d-segments-depthwise")
NATIVE_ROUTES = [r for r in ru.ROUTES if r.name not in REFUSED_ROUTES and any(not c.f64 for c in r.cases)]


@pytest.fixture(autouse=True)
def _no_knob_plans_afterwards():
    """The plan cache key does not hold the knobs: plans built under them must not outlive the test."""
    yield
    from fft_conv_pytorch_amd import _native, functional
    _native.clear_plan_cache()
    functional._REFUSED_HALF.clear()


def _knobs(monkeypatch, *envs):
    from fft_conv_pytorch_amd import _native, functional
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for env in envs:
        for k, v in env.items():
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, v)
    _native.clear_plan_cache()
    functional._REFUSED_HALF.clear()


def _kw(c):
    if c.tr:
        return dict(stride=c.tup(c.s), padding=c.tup(c.p), output_padding=c.tup(c.op), dilation=c.tup(c.d), groups=c.g)
    return dict(stride=c.tup(c.s), padding=c.tup(c.p), dilation=c.tup(c.d), groups=c.g, padding_mode=c.mode)


def _plan(c, x, w, b):
    from fft_conv_pytorch_amd import functional as fc
    kw = _kw(c)
    return fc._plan_for(x, w, b, kw["stride"], kw["padding"], kw["dilation"], c.g, "constant" if c.tr else c.mode,
                        transposed=c.tr, output_padding=kw.get("output_padding", 0))


def _plan_forward(plan, x, spec, b):
    """Plan.forward into an output filled with NaN: a sample the kernels never store stays NaN."""
    from fft_conv_pytorch_amd import functional as fc
    out = torch.full((x.shape[0], plan.key[3]) + plan.out_spatial, float("nan"), dtype=plan.dtype, device=DEV)
    ws = fc.new_workspace(plan, x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    plan.forward(x.data_ptr(), spec.buf.data_ptr(), b.data_ptr() if b is not None else None, out.data_ptr(),
                 ws.data_ptr() if ws is not None else None, stream)
    return out


def _tensors(c, dtype, seed=0, scale=1.0):
    gen = torch.Generator(device=DEV).manual_seed(sum(c.size) + 7 * c.B + c.cin + seed)
    x = (torch.randn((c.B, c.cin) + tuple(c.size), generator=gen, device=DEV) * scale).to(dtype)
    w = (torch.randn(c.wshape, generator=gen, device=DEV) / math.sqrt(math.prod(c.wshape[1:]))).to(dtype)
    b = torch.randn(c.cout, generator=gen, device=DEV).to(dtype)
    return x, w, b


def _cast_path(c, x, w, b):
    """Today's float16 / bfloat16 result: float32 tensors through the float32 plan, rounded once."""
    from fft_conv_pytorch_amd import functional as fc
    x32, w32, b32 = x.float(), w.float(), b.float() if b is not None else None
    plan = _plan(c, x32, w32, b32)
    return _plan_forward(plan, x32, fc.transform_kernel(plan, w32), b32).to(x.dtype), plan


def _same_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = got.view(torch.int16) != want.view(torch.int16)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {got.numel()} samples differ from the cast path's bits"


def _public(c, x, w, b):
    from fft_conv_pytorch_amd.functional import fft_conv, fft_conv_transpose
    return (fft_conv_transpose if c.tr else fft_conv)(x, w, b, **_kw(c))


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("route", NATIVE_ROUTES, ids=[r.name for r in NATIVE_ROUTES])
def test_native_route_bits(route, dtype, monkeypatch):
    from fft_conv_pytorch_amd import functional as fc
    cases = [c for c in route.cases if not c.f64]
    for c in cases:
        _knobs(monkeypatch, route.env, c.env)
        x, w, b = _tensors(c, dtype)
        want, plan32 = _cast_path(c, x, w, b)
        plan = _plan(c, x, w, b)
        what = f"{route.name} / {c.ident()} / {dtype}"
        assert plan.dtype == dtype and plan.weight_dtype == torch.float32, what
        assert plan.route == plan32.route, f"{what}: half plan route {plan.route} != float32 {plan32.route}"
        assert plan.signature() == plan32.signature(), what
        assert plan.workspace_bytes == plan32.workspace_bytes, what
        got = _plan_forward(plan, x, fc.transform_kernel(plan, w), b.float())
        assert not torch.isnan(got).any() or torch.isnan(want).any(), f"{what}: samples not written"
        _same_bits(got, want, what)
        if c.public:
            _same_bits(_public(c, x, w, b), want, what + " (public op)")
        torch.cuda.synchronize()


REFUSED = [
    ("chunk launches", {}, ru.C(2, 20, 6, (5317,), (700,), p=100, d=3)),
    ("segments of taps", {}, ru.C(2, 8, 8, (20000,), (5000,))),
    ("segments of taps", {"FFTCONV_NDSEG": "4", "FFTCONV_PLANES": "0"}, ru.C(2, 3, 4, (40, 60), (9, 11), p=2)),
]


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("name,env,c", REFUSED, ids=["1d-chunk", "1d-segments", "2d-ndseg"])
def test_refused_route_falls_back(name, env, c, dtype, monkeypatch):
    _knobs(monkeypatch, env)
    x, w, b = _tensors(c, dtype)
    with pytest.raises(NotImplementedError, match=name):
        _plan(c, x, w, b)
    want, _ = _cast_path(c, x, w, b)
    _same_bits(_public(c, x, w, b), want, f"{name} public op")
    _same_bits(_public(c, x, w, b), want, f"{name} public op, refusal remembered")


def _peak_increase(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


@pytest.mark.parametrize("c", [ru.C(32, 8, 8, (32768,), (512,)), ru.C(8, 8, 8, (256, 256), (9, 9), p=4)],
                         ids=["cfgA", "2d"])
def test_peak_memory(c, monkeypatch):
    from fft_conv_pytorch_amd.functional import fft_conv
    _knobs(monkeypatch)
    x, w, b = _tensors(c, torch.bfloat16)
    fft_conv(x, w, b, **_kw(c))                 # warm plan (and allocator)
    plan = _plan(c, x, w, b)
    grow, y = _peak_increase(lambda: fft_conv(x, w, b, **_kw(c)))
    bound = y.numel() * y.element_size() + plan.spectrum_bytes + plan.workspace_bytes + (8 << 20)
    assert grow <= bound, f"native call grew the peak by {grow} bytes > {bound}"
    del y
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    fft_conv(x, w, b, **_kw(c))
    grow_cast, y = _peak_increase(lambda: fft_conv(x, w, b, **_kw(c)))
    assert grow_cast > bound, f"cast path grew the peak by only {grow_cast} bytes (bound {bound})"


ODD = [
    ("odd L, odd Lout", {}, ru.C(3, 8, 8, (5001,), (130,), p=3)),
    ("odd L 2-D", {"FFTCONV_PLANES": "0"}, ru.C(2, 3, 5, (37, 101), (4, 7), p=(1, 2))),
    ("odd L transposed", {}, ru.C(2, 4, 6, (1001,), (33,), s=3, p=5, op=1, tr=True)),
    ("phase quads", {"FFTCONV_PERS": "4"}, ru.C(4, 8, 8, (30002,), (250,), d=4, p=31, mode="reflect")),
    ("phase pairs", {"FFTCONV_PERS": "4", "FFTCONV_PH2": "1"}, ru.C(5, 8, 8, (9001,), (200,), d=4, p=4)),
    ("3-D planes", {}, ru.C(2, 3, 4, (17, 19, 23), (3, 5, 3), p=1)),
]


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd-start"])
@pytest.mark.parametrize("name,env,c", ODD, ids=[o[0].replace(" ", "-").replace(",", "") for o in ODD])
def test_alignment_and_odd_sizes(name, env, c, offset, dtype, monkeypatch):
    _knobs(monkeypatch, env)
    x, w, b = _tensors(c, dtype)
    if offset:      # storage starting at an odd element
        n = x.numel()
        xs = torch.empty(n + 1, dtype=dtype, device=DEV)[1:].view(x.shape)
        xs.copy_(x)
        x = xs
    want, plan32 = _cast_path(c, x, w, b)
    if name.startswith("phase quads"):
        assert plan32.route["ph2"] == 2, plan32.route
    if name.startswith("phase pairs"):
        assert plan32.route["ph2"] == 1, plan32.route
    _same_bits(_public(c, x, w, b), want, name)


def test_special_values(monkeypatch):
    from fft_conv_pytorch_amd.functional import fft_conv
    _knobs(monkeypatch)
    # float16 outputs past 65504: inf at the same positions with the same signs
    c = ru.C(2, 8, 8, (4000,), (65,), p=32)
    x, w, b = _tensors(c, torch.float16, scale=4000.0)
    w = w * 16                              # outputs of about 64000 sigma-one
    want, _ = _cast_path(c, x, w, b)
    got = fft_conv(x, w, b, **_kw(c))
    assert torch.isinf(want).any(), "the case must overflow"
    assert torch.equal(torch.isinf(got), torch.isinf(want)) and torch.equal(got[torch.isinf(got)], want[torch.isinf(want)])
    _same_bits(got, want, "float16 overflow")
    # a bfloat16 output of 2^20+ samples: round-to-nearest-even ties occur
    c = ru.C(4, 8, 8, (40000,), (129,), p=64)
    x, w, b = _tensors(c, torch.bfloat16, seed=3)
    want, _ = _cast_path(c, x, w, b)
    assert want.numel() >= 1 << 20
    _same_bits(fft_conv(x, w, b, **_kw(c)), want, "bfloat16 ties")
    # one NaN in the input: NaN where the cast path has NaN
    for dtype in HALF:
        c = ru.C(2, 8, 8, (3000,), (33,), p=16)
        x, w, b = _tensors(c, dtype, seed=5)
        x[1, 3, 1234] = float("nan")
        want, _ = _cast_path(c, x, w, b)
        got = fft_conv(x, w, b, **_kw(c))
        assert torch.isnan(want).any()
        assert torch.equal(torch.isnan(got), torch.isnan(want)), dtype


MODULES = [
    ("FFTConv1d", dict(in_channels=8, out_channels=8, kernel_size=129, padding=64), (4, 8, 5000)),
    ("FFTConv2d", dict(in_channels=3, out_channels=4, kernel_size=5, padding=2), (2, 3, 60, 70)),
    ("FFTConv3d", dict(in_channels=2, out_channels=3, kernel_size=3, padding=1), (2, 2, 20, 21, 22)),
    ("FFTConvTranspose1d", dict(in_channels=8, out_channels=8, kernel_size=33, stride=2, padding=5, output_padding=1),
     (2, 8, 700)),
    ("FFTConvTranspose2d", dict(in_channels=3, out_channels=4, kernel_size=4, stride=2, padding=1), (2, 3, 30, 40)),
]


@pytest.mark.parametrize("name,kw,shape", MODULES, ids=[m[0] for m in MODULES])
def test_modules(name, kw, shape, monkeypatch):
    import fft_conv_pytorch_amd as pkg
    from fft_conv_pytorch_amd import functional as fc
    _knobs(monkeypatch)
    torch.manual_seed(0)
    layer = getattr(pkg, name)(bias=True, **kw).to(DEV).to(torch.bfloat16).eval()
    x = torch.randn(shape, device=DEV).to(torch.bfloat16)
    calls = []
    orig = fc.transform_kernel
    monkeypatch.setattr(fc, "transform_kernel", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    with torch.no_grad():
        y1 = layer(x)
        y2 = layer(x)
        native_calls = len(calls)
        monkeypatch.setenv("FFTCONV_HALF_IO", "0")
        want = layer(x)
    assert y1.dtype == torch.bfloat16
    _same_bits(y1, want, name)
    _same_bits(y2, want, name + " (second call)")
    assert native_calls == 1, f"{name}: the kernel was transformed {native_calls} times in two native calls"
    assert "_spectrum_cache" in layer.__dict__
