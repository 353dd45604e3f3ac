"""float64 1-D convolutions with kernels past the 2048-point tile through one long transform per row (csrc/long_f64.hip,
plan kind ``f64_fft_long``): every factor length, the planner's own choices, overlap-save tiles with a seam probe, every
argument of the public ops, modules, gradients, the direct kernel's agreement and graph capture.

The reference is torch's float64 convolution on CPU copies (``F.pad`` in the mode for a padding mode); the bound is
route_util.TOL64 = 1e-12 of the result's largest magnitude.  Forwards at C level run into an output filled with NaN, so a
sample the kernels never store fails the check."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import route_util as ru

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = ru.TOL64
KNOBS = ("FFTCONV_F64_FFT", "FFTCONV_F64_LONG", "FFTCONV_F64_LONG_N", "FFTCONV_LONG_WS_MB", "FFTCONV_ZEROWRAP", "FFTCONV_TILE")
C = ru.Case


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    """Knobs are read at plan creation and are not part of the plan cache's key: none set on entry, no plan built under
    one outlives the test."""
    from fft_conv_pytorch_amd import _native
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    _native.clear_plan_cache()
    yield
    _native.clear_plan_cache()


def _set(monkeypatch, **env):
    from fft_conv_pytorch_amd import _native
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _native.clear_plan_cache()


def _err(got, want):
    want = want.double()
    return (got.double().cpu() - want).abs().max().item() / max(want.abs().max().item(), 1e-300)


def _kw(c):
    if c.tr:
        return dict(stride=c.s, padding=c.p, output_padding=c.op, dilation=c.d, groups=c.g)
    return dict(stride=c.s, padding=c.p, dilation=c.d, groups=c.g, padding_mode=c.mode)


def _reference(c, x, w, b):
    """torch's float64 convolution of CPU tensors."""
    if c.tr:
        return F.conv_transpose1d(x, w, b, stride=c.s, padding=c.p, output_padding=c.op, groups=c.g, dilation=c.d)
    if c.mode == "constant":
        return F.conv1d(x, w, b, stride=c.s, padding=c.p, dilation=c.d, groups=c.g)
    return F.conv1d(F.pad(x, (c.p, c.p), mode=c.mode), w, b, stride=c.s, dilation=c.d, groups=c.g)


def _tensors(c, bias=True):
    gen = torch.Generator().manual_seed(c.size[0] + 7 * c.B + c.cin + c.k[0])
    x = torch.randn((c.B, c.cin) + tuple(c.size), generator=gen, dtype=torch.float64)
    w = torch.randn(c.wshape, generator=gen, dtype=torch.float64) / math.sqrt(math.prod(c.wshape[1:]))
    b = torch.randn(c.cout, generator=gen, dtype=torch.float64) if bias else None
    return x, w, b


def _plan(c, x, w, b):
    from fft_conv_pytorch_amd import functional as fc
    return fc._plan_for(x, w, b, c.s, c.p, c.d, c.g, "constant" if c.tr else c.mode, transposed=c.tr,
                        output_padding=c.op if c.tr else 0)


def _plan_forward(plan, x, spec, b):
    """Plan.forward into an output filled with NaN: a sample the kernels never store stays NaN."""
    from fft_conv_pytorch_amd import functional as fc
    out = torch.full((x.shape[0], plan.key[3]) + plan.out_spatial, float("nan"), dtype=plan.dtype, device=DEV)
    ws = fc.new_workspace(plan, x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    plan.forward(x.data_ptr(), spec.buf.data_ptr(), b.data_ptr() if b is not None else None, out.data_ptr(),
                 ws.data_ptr() if ws is not None else None, stream)
    torch.cuda.synchronize()
    return out


def _check(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = int((~torch.isfinite(got)).sum())
    assert bad == 0, f"{what}: {bad} output samples not written / not finite"
    err = _err(got, want)
    print(f"{what}: max|got - want| / max|want| = {err:.3e}")
    assert err < TOL, f"{what}: element-wise error {err:.3e} >= {TOL}"


def _run_c_level(c, bias=True, expect=None):
    """The plan's forward at C level against the reference; returns (plan, x, w, b, want) with x, w, b on the GPU."""
    from fft_conv_pytorch_amd import functional as fc
    xc, wc, bc = _tensors(c, bias)
    x, w, b = xc.to(DEV), wc.to(DEV), bc.to(DEV) if bias else None
    plan = _plan(c, x, w, b)
    r = plan.route
    assert r["kind"] == "f64_fft_long", r
    assert plan.tile == r["N2"]
    if expect is not None:
        assert expect(r), f"case not sized as intended: {r}"
    spec = fc.transform_kernel(plan, w)
    want = _reference(c, xc, wc, bc)
    _check(_plan_forward(plan, x, spec, b), want, f"{c.ident()} {r}")
    return plan, spec, (x, w, b), (xc, wc, bc), want


# ------------------------------------------------------------------ every N1 and every N2 length
FACTORS = ["64x64", "128x64", "256x64", "512x64", "1024x64", "2048x64", "64x128", "64x256", "64x512", "64x1024", "64x2048",
           "256x256"]


@pytest.mark.parametrize("fac", FACTORS)
def test_forced_factorisation(fac, monkeypatch):
    n1, n2 = (int(v) for v in fac.split("x"))
    _set(monkeypatch, FFTCONV_F64_LONG_N=fac, FFTCONV_F64_LONG="2")
    L = 2500 if n1 * n2 == 4096 else 3000           # (one transform: the row and its 1100 taps inside 4096 points)
    c = C(3, 4, 6, (L,), (1100,), g=2, f64=True)
    _run_c_level(c, expect=lambda r: (r["N1"], r["N2"], r["ntiles"]) == (n1, n2, 1))


# ------------------------------------------------------------------ the planner's own choice
OWN = [
    C(2, 3, 5, (5000,), (1026,), f64=True),
    C(1, 2, 2, (20000,), (20000,), g=2, p=10000, f64=True),
    C(5, 2, 3, (4000,), (1500,), p=750, f64=True, note="odd-batch"),
]


@pytest.mark.parametrize("c", OWN, ids=[c.ident() for c in OWN])
def test_planner_choice(c):
    _run_c_level(c, expect=lambda r: r["ntiles"] == 1 and r["N1"] <= r["N2"])


# ------------------------------------------------------------------ overlap-save tiles
def _seam_probe(c, seams):
    """Zeros plus unit impulses, on every channel, at the first and last samples, at the padding boundary and at the input
    samples that meet both sides of every tile seam (the first and the last tap of the outputs around it)."""
    kd = (c.k[0] - 1) * c.d + 1
    S, p = c.size[0], c.p
    pos = {0, 1, S - 2, S - 1, p - 1, p, p + 1, S - 1 - p, S - p}
    for o in seams:
        for q in (o - 1, o, o + 1):
            if c.tr:
                padl = kd - 1 - p
                pos.update({(q - padl) // c.s, (q + kd - 1 - padl) // c.s})
            else:
                pos.update({q - p, q - p + kd - 1})
    x = torch.zeros((c.B, c.cin, S), dtype=torch.float64)
    x[:, :, [v for v in pos if 0 <= v < S]] = 1.0
    return x


TILED = [
    C(2, 4, 4, (10000,), (1100,), f64=True),
    C(3, 2, 4, (9000,), (1100,), s=2, p=300, mode="reflect", f64=True),
    C(2, 4, 2, (4000,), (1100,), s=2, p=5, op=1, g=2, tr=True, f64=True),
]


@pytest.mark.parametrize("c", TILED, ids=[c.ident() for c in TILED])
def test_tiles_random_data_and_seam_probe(c, monkeypatch):
    _set(monkeypatch, FFTCONV_F64_LONG_N="64x64", FFTCONV_F64_LONG="2")
    V = 4096 - 1100 + 1
    plan, spec, (x, w, b), (xc, wc, bc), want = _run_c_level(c, expect=lambda r: (r["N1"], r["N2"]) == (64, 64) and r["ntiles"] >= 3)
    Lf = (want.shape[-1] - 1) * (1 if c.tr else c.s) + 1
    assert plan.route["ntiles"] == -(-Lf // V)
    seams = [j * V for j in range(1, plan.route["ntiles"])]
    probe = _seam_probe(c, seams)
    _check(_plan_forward(plan, probe.to(DEV), spec, b), _reference(c, probe, wc, bc), "seam probe")


# ------------------------------------------------------------------ every argument, one case each
ARGS = [
    (C(2, 3, 4, (5000,), (1100,), s=3, p=100, f64=True, note="stride3"), True),
    (C(2, 3, 4, (5000,), (300,), d=4, p=50, f64=True, note="dilation4"), True),
    (C(2, 4, 3, (4000,), (1100,), p=400, mode="reflect", f64=True), True),
    (C(3, 2, 2, (3500,), (1100,), p=300, mode="replicate", f64=True), True),
    (C(2, 2, 4, (3000,), (1100,), p=1000, mode="circular", f64=True), True),
    (C(3, 6, 6, (4000,), (1100,), g=6, p=550, f64=True, note="depthwise"), True),
    (C(2, 4, 4, (4000,), (1100,), p=10, f64=True, note="no-bias"), False),
    (C(2, 6, 4, (700,), (1100,), s=2, p=5, op=1, tr=True, f64=True), True),
]


@pytest.mark.parametrize("c,bias", ARGS, ids=[a[0].ident() for a in ARGS])
def test_every_argument(c, bias):
    _run_c_level(c, bias)


# ------------------------------------------------------------------ public ops and modules
def test_public_ops_match_torch():
    from fft_conv_pytorch_amd.functional import fft_conv, fft_conv_transpose
    c = C(2, 4, 6, (4000,), (1100,), s=2, p=500, g=2, mode="circular", f64=True)
    xc, wc, bc = _tensors(c)
    x, w, b = xc.to(DEV), wc.to(DEV), bc.to(DEV)
    assert _plan(c, x, w, b).route["kind"] == "f64_fft_long"
    _check(fft_conv(x, w, b, **_kw(c)), _reference(c, xc, wc, bc), "fft_conv")
    c = C(2, 6, 4, (700,), (1100,), s=2, p=5, op=1, g=2, tr=True, f64=True)
    xc, wc, bc = _tensors(c)
    x, w, b = xc.to(DEV), wc.to(DEV), bc.to(DEV)
    assert _plan(c, x, w, b).route["kind"] == "f64_fft_long"
    _check(fft_conv_transpose(x, w, b, **_kw(c)), _reference(c, xc, wc, bc), "fft_conv_transpose")


def test_module_cached_spectrum_equals_uncached():
    from fft_conv_pytorch_amd import FFTConv1d
    torch.manual_seed(2)
    layer = FFTConv1d(4, 4, 1100, padding=550, bias=True).to(DEV).double()
    x = torch.randn(2, 4, 3000, dtype=torch.float64, device=DEV)
    with torch.no_grad():
        layer.cache_kernel_spectrum = False
        uncached = layer(x)                  # transforms the weight in the call
        layer.cache_kernel_spectrum = True
        layer.eval()
        first = layer(x)
        cached = layer(x)                    # eval: the kernel spectrum of the first call
    assert layer.__dict__["_spectrum_cache"][1].plan.route["kind"] == "f64_fft_long"
    assert torch.equal(first, cached) and torch.equal(uncached, cached)
    _check(cached, F.conv1d(x.cpu(), layer.weight.detach().cpu(), layer.bias.detach().cpu(), padding=550), "FFTConv1d")


def test_gradients_match_cpu_autograd():
    """dX (a transposed plan on the long route), dW (chunks of dY on the tiled route) and db at B2 4->4 L 3000 K 1100."""
    from fft_conv_pytorch_amd import fft_conv
    from fft_conv_pytorch_amd.functional import _plan_for
    c = C(2, 4, 4, (3000,), (1100,), p=550, f64=True)
    xc, wc, bc = _tensors(c)
    x, w, b = (t.to(DEV).requires_grad_() for t in (xc, wc, bc))
    y = fft_conv(x, w, b, padding=550)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    y.backward(gy.to(DEV))
    xr, wr, br = (t.clone().requires_grad_() for t in (xc, wc, bc))
    want = F.conv1d(xr, wr, br, padding=550)
    want.backward(gy)
    _check(y.detach(), want.detach(), "y")
    for name, got_, want_ in (("dX", x.grad, xr.grad), ("dW", w.grad, wr.grad), ("db", b.grad, br.grad)):
        _check(got_, want_, name)
    dx_plan = _plan_for(gy.to(DEV), w.detach(), None, 1, 550, 1, 1, "constant", transposed=True, output_padding=0)
    assert dx_plan.route["kind"] == "f64_fft_long"          # the plan autograd ran for dX


# ------------------------------------------------------------------ the direct kernel agrees
def test_direct_kernel_agrees(monkeypatch):
    from fft_conv_pytorch_amd import fft_conv
    c = C(3, 4, 6, (3000,), (1100,), s=2, p=200, g=2, mode="reflect", f64=True)
    xc, wc, bc = _tensors(c)
    x, w, b = xc.to(DEV), wc.to(DEV), bc.to(DEV)
    outs = {}
    for knob, kind in (("1", "f64_fft_long"), ("0", "f64_direct")):
        _set(monkeypatch, FFTCONV_F64_LONG=knob)            # (read at plan creation)
        assert _plan(c, x, w, b).route["kind"] == kind
        outs[knob] = fft_conv(x, w, b, **_kw(c))
    assert _err(outs["1"], outs["0"].cpu()) < TOL
    _check(outs["1"], _reference(c, xc, wc, bc), "long route")


# ------------------------------------------------------------------ graph capture
def test_warm_forward_is_capturable_and_replays_bit_for_bit():
    from fft_conv_pytorch_amd import FFTConv1d
    torch.manual_seed(4)
    layer = FFTConv1d(4, 4, 1100, padding=550, bias=True).to(DEV).double().eval()
    x = torch.randn(3, 4, 3000, dtype=torch.float64, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        eager = layer(x)                     # warm: plan and kernel spectrum exist before the capture
        eager = layer(x)
    torch.cuda.current_stream().wait_stream(s)
    assert layer.__dict__["_spectrum_cache"][1].plan.route["kind"] == "f64_fft_long"
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        out = layer(x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    _check(eager, F.conv1d(x.cpu(), layer.weight.detach().cpu(), layer.bias.detach().cpu(), padding=550), "captured forward")
