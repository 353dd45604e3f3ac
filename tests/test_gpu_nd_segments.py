"""Float32 2-D / 3-D kernels run in segments of taps (csrc/host_nd.cpp plan_nd_segments).

An axis whose dilated kernel extent no FFT tile holds is cut into segments of C taps; segment j reads the padded axis
from position j*C*dilation on against its own spectrum, and the later segments add into y.  Every case asserts its route
(segments > 1 on the intended axis) and runs ``Plan.forward`` into an output filled with NaN, so that a sample no
segment stores, or a first segment that adds instead of storing, shows.  Results are compared with torch's float64
convolution element-wise at route_util.TOL32; a seam probe puts impulses at both sides of every segment boundary and
every tile seam."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import route_util as ru
from tests.test_gpu_routes import _sample_idx, _sampled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOBS = ("FFTCONV_NDSEG", "FFTCONV_PLANES", "FFTCONV_XTILE", "FFTCONV_YTILE", "FFTCONV_ZEROWRAP", "FFTCONV_TILE")
C = ru.Case


@pytest.fixture(autouse=True)
def _clean_knobs(monkeypatch):
    """No planner knob from the environment; plans built under a knob do not outlive the test."""
    from fft_conv_pytorch_amd import _native
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    _native.clear_plan_cache()
    yield
    _native.clear_plan_cache()


def _set_seg(monkeypatch, taps):
    from fft_conv_pytorch_amd import _native
    if taps is None:
        monkeypatch.delenv("FFTCONV_NDSEG", raising=False)
    else:
        monkeypatch.setenv("FFTCONV_NDSEG", str(taps))
    _native.clear_plan_cache()


def _err(got, want):
    return (got.double() - want.double()).abs().max().item() / max(want.double().abs().max().item(), 1e-300)


def _kw(c):
    if c.tr:
        return dict(stride=c.tup(c.s), padding=c.tup(c.p), output_padding=c.tup(c.op), dilation=c.tup(c.d), groups=c.g)
    return dict(stride=c.tup(c.s), padding=c.tup(c.p), dilation=c.tup(c.d), groups=c.g, padding_mode=c.mode)


def _reference(c, x, w, b):
    """torch's float64 convolution (forward or transposed)."""
    x, w, b = x.double(), w.double(), None if b is None else b.double()
    if c.tr:
        fn = (F.conv_transpose1d, F.conv_transpose2d, F.conv_transpose3d)[c.nd - 1]
        return fn(x, w, b, stride=c.tup(c.s), padding=c.tup(c.p), output_padding=c.tup(c.op), groups=c.g,
                  dilation=c.tup(c.d))
    conv = (F.conv1d, F.conv2d, F.conv3d)[c.nd - 1]
    if c.mode == "constant":
        return conv(x, w, b, stride=c.tup(c.s), padding=c.tup(c.p), dilation=c.tup(c.d), groups=c.g)
    flat = [q for p in reversed(c.tup(c.p)) for q in (p, p)]
    return conv(F.pad(x, flat, mode=c.mode), w, b, stride=c.tup(c.s), dilation=c.tup(c.d), groups=c.g)


def _plan(c, x, w, b):
    from fft_conv_pytorch_amd import functional as fc
    kw = _kw(c)
    return fc._plan_for(x, w, b, kw["stride"], kw["padding"], kw["dilation"], c.g, "constant" if c.tr else c.mode,
                        transposed=c.tr, output_padding=kw.get("output_padding", 0))


def _plan_forward(plan, x, spec, b):
    """Plan.forward into an output filled with NaN."""
    from fft_conv_pytorch_amd import functional as fc
    out = torch.full((x.shape[0], plan.key[3]) + plan.out_spatial, float("nan"), dtype=torch.float32, device=DEV)
    ws = fc.new_workspace(plan, x.device)
    plan.forward(x.data_ptr(), spec.buf.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr() if ws is not None else None,
                 torch.cuda.current_stream(x.device).cuda_stream)
    return out


def _geometry(c, r, ax):
    """(padded left pad, spread step, stride-1 outputs, dilated extent of one segment, segment starts (padded
    coordinates), stride-1 output seams of the axis' overlap-save tiles)."""
    k, d, s, p = c.k[ax], c.tup(c.d)[ax], c.tup(c.s)[ax], c.tup(c.p)[ax]
    kd = (k - 1) * d + 1
    if c.tr:
        padl, up = kd - 1 - p, s
        Lf = (c.size[ax] - 1) * s - 2 * p + kd - 1 + c.tup(c.op)[ax] + 1
    else:
        padl, up = p, 1
        Lf = c.size[ax] + 2 * p - kd + 1
    nseg, taps = r[f"nseg{ax}"], r[f"seg_taps{ax}"]
    kds = (taps - 1) * d + 1
    starts = [j * taps * d for j in range(nseg)]
    T, n = {0: (r["T"], r["ntiles"]), c.nd - 1: (r["Tx"], r["nxt"])}.get(ax, (r["Tm"], r["nyt"]))
    seams = [j * (T - kds + 1) for j in range(1, n)]
    return padl, up, Lf, kds, starts, seams


def seam_probe(c, r):
    """Zeros plus unit impulses (every channel) at the row ends, at both sides of every segment boundary and at the
    input samples that meet both sides of every tile seam of every segment (its first and its last tap)."""
    masks = []
    for ax in range(c.nd):
        S = c.size[ax]
        padl, up, Lf, kds, starts, seams = _geometry(c, r, ax)
        padded = set()
        for b0 in starts:
            padded.update({b0 - 1, b0, b0 + 1})
            for o in [0, 1, Lf - 2, Lf - 1] + [q for sm in seams for q in (sm - 1, sm, sm + 1)]:
                padded.update({b0 + o, b0 + o + kds - 1})
        pos = {0, 1, S - 2, S - 1}
        for q in padded:
            if (q - padl) % up == 0:
                pos.add((q - padl) // up)
        m = torch.zeros(S, dtype=torch.bool)
        m[[v for v in pos if 0 <= v < S]] = True
        shape = [1] * c.nd
        shape[ax] = S
        masks.append(m.view(shape))
    mask = masks[0]
    for m in masks[1:]:
        mask = mask & m
    x = torch.zeros((c.B, c.cin) + tuple(c.size), device=DEV)
    x[:, :] = mask.float().to(DEV)
    return x


def _check(c, r, got, x, w, b, what):
    """got against float64: torch's convolution while its column buffer stays under 4 GiB, else sampled dot products
    (route_util's rule for large outputs) at random positions, the row ends and both sides of every tile seam."""
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} output samples not written"
    cols = math.prod(got.shape[2:]) * math.prod(w.shape[1:]) * 8
    if c.tr or cols < (4 << 30):
        want = _reference(c, x, w, b)
        assert got.shape == want.shape, (got.shape, want.shape)
        err = _err(got, want)
    else:
        seams = [_geometry(c, r, ax)[5] for ax in range(c.nd)]
        idx = _sample_idx(c, tuple(got.shape), seams)
        err = _err(got[tuple(idx.t().to(DEV))], _sampled(c, x, w, b, idx))
    assert err <= ru.TOL32, f"{what}: element-wise error {err:.3e} > {ru.TOL32}"
    return err


def _tensors(c, bias_scale=1.0):
    gen = torch.Generator(device=DEV).manual_seed(sum(c.size) + 7 * c.B + c.cin)
    x = torch.randn((c.B, c.cin) + tuple(c.size), generator=gen, device=DEV)
    w = torch.randn(c.wshape, generator=gen, device=DEV) / math.sqrt(math.prod(c.wshape[1:]))
    b = torch.randn(c.cout, generator=gen, device=DEV) * bias_scale
    return x, w, b


def _run(c, seg_axes, bias_scale=1.0, probe=True):
    """Route, NaN-filled forward, seam probe and the public op of one case; returns the worst error."""
    from fft_conv_pytorch_amd import functional as fc
    from fft_conv_pytorch_amd.functional import fft_conv, fft_conv_transpose
    x, w, b = _tensors(c, bias_scale)
    plan = _plan(c, x, w, b)
    r = plan.route
    assert r["kind"] == "f32_nd" and (r["planes"] == 0 or not seg_axes), r
    for ax in range(c.nd):
        want_seg = ax in seg_axes
        assert (r[f"nseg{ax}"] > 1) == want_seg, (ax, r)
        assert plan.layout[4 + ax] == (r[f"seg_taps{ax}"] if want_seg else 0), (plan.layout, r)
        assert r[f"nseg{ax}"] == -(-c.k[ax] // r[f"seg_taps{ax}"]), r
    spec = fc.transform_kernel(plan, w)
    worst = _check(c, r, _plan_forward(plan, x, spec, b), x, w, b, "forward")
    if probe:
        # (no bias: an impulse answer far below the bias would pass any error bound relative to it)
        zb = torch.zeros_like(b)
        xp = seam_probe(c, r)
        worst = max(worst, _check(c, r, _plan_forward(plan, xp, spec, zb), xp, w, zb, "seam probe"))
    op = fft_conv_transpose if c.tr else fft_conv
    return max(worst, _check(c, r, op(x, w, b, **_kw(c)), x, w, b, "public op"))


# ------------------------------------------------------------------------------------------ 1. kernels past 4096
LONG = [
    (C(1, 3, 4, (12, 9000), (3, 5000), p=(1, 2000)), {1}),
    (C(1, 2, 2, (10, 6000), (3, 1100), p=(1, 300), d=(1, 4), mode="reflect", note="kd4397"), {1}),
    (C(1, 2, 2, (5000, 16), (4500, 3), s=(2, 1), p=(0, 1)), {0}),
    (C(1, 2, 2, (3, 4500, 4), (2, 4200, 3), p=(0, 100, 1), mode="replicate"), {1}),
    (C(1, 18, 4, (6, 5000), (2, 4300), g=2, p=(0, 2), note="cig9"), {1}),
    (C(1, 2, 6, (4, 600), (3, 4500), s=(1, 2), p=(1, 3), tr=True), {1}),
]


@pytest.mark.parametrize("case,axes", LONG, ids=[c.ident() for c, _ in LONG])
def test_kernels_longer_than_4096(case, axes):
    print(f"\n{case.ident()}: worst {_run(case, axes):.2e}")


def test_large_bias_is_added_once():
    """A bias 1000x the output scale: added by every segment, it would be off by whole multiples of itself."""
    c = C(1, 2, 3, (4, 5000), (3, 4400), p=(1, 0))
    _run(c, {1}, bias_scale=1000.0, probe=False)


# ------------------------------------------------------------------------------------------ 2. forced segments
FORCED = [
    (C(2, 3, 4, (20, 30), (5, 7), p=(2, 3)), 3, {0, 1}),
    (C(2, 3, 4, (20, 30), (2, 7), p=(1, 3)), 3, {1}),
    (C(1, 2, 3, (40, 18), (7, 3), p=(3, 1)), 3, {0}),
    (C(2, 3, 4, (25, 33), (5, 7), s=(2, 3), p=(2, 1)), 2, {0, 1}),
    (C(1, 3, 2, (30, 40), (4, 5), d=(2, 3), p=(3, 4), mode="reflect"), 2, {0, 1}),
    (C(1, 3, 2, (30, 40), (4, 5), p=(2, 2), mode="replicate"), 3, {0, 1}),
    (C(1, 3, 2, (30, 40), (4, 5), s=(1, 2), p=(3, 4), mode="circular"), 2, {0, 1}),
    (C(2, 3, 4, (12, 15), (5, 6), s=(2, 1), p=(1, 2), op=(1, 0), tr=True), 2, {0, 1}),
    (C(2, 3, 2, (9, 10), (3, 5), d=(2, 1), s=(1, 3), p=(2, 0), op=(0, 2), tr=True), 2, {0, 1}),
    (C(1, 2, 3, (10, 12, 14), (4, 5, 3), p=(1, 2, 1)), 2, {0, 1, 2}),
    (C(2, 2, 3, (9, 20, 11), (2, 6, 3), s=(1, 2, 1), p=(0, 2, 1), mode="reflect"), 3, {1}),
    (C(1, 3, 2, (8, 9, 10), (3, 4, 5), s=(2, 1, 1), p=(1, 1, 2), op=(1, 0, 0), tr=True), 2, {0, 1, 2}),
]


@pytest.mark.parametrize("case,taps,axes", FORCED, ids=[c.ident() for c, _, _ in FORCED])
def test_forced_segments(case, taps, axes, monkeypatch):
    """FFTCONV_NDSEG=<taps>: segments on small shapes (every axis, two at once, stride, dilation, every padding mode,
    transposed), and the same shape unsegmented against the same reference."""
    _set_seg(monkeypatch, taps)
    seg = _run(case, axes)
    _set_seg(monkeypatch, None)
    whole = _run(case, set())
    print(f"\n{case.ident()}: segmented {seg:.2e}, whole {whole:.2e}")


# ------------------------------------------------------------------------------------------ 3. training on long signals
def _train(layer, x):
    """dX, dW and db of a module against float64 autograd."""
    torch.manual_seed(3)
    layer = layer.to(DEV)
    ref = next(k for k in type(layer).__mro__ if k.__module__.startswith("torch.nn"))   # nn.Conv2d, ...
    xg = x.clone().requires_grad_()
    y = layer(xg)
    gy = torch.randn(y.shape, generator=torch.Generator(device=DEV).manual_seed(9), device=DEV)
    y.backward(gy)
    xr = x.double().requires_grad_()
    wr = layer.weight.detach().double().requires_grad_()
    br = layer.bias.detach().double().requires_grad_()
    conv = {"Conv2d": F.conv2d, "Conv3d": F.conv3d, "ConvTranspose2d": F.conv_transpose2d}[ref.__name__]
    if "Transpose" in ref.__name__:
        want = conv(xr, wr, br, stride=layer.stride, padding=layer.padding, output_padding=layer.output_padding,
                    dilation=layer.dilation, groups=layer.groups)
    else:
        want = conv(xr, wr, br, stride=layer.stride, padding=layer.padding, dilation=layer.dilation, groups=layer.groups)
    assert _err(y.detach(), want.detach()) <= ru.TOL32
    want.backward(gy.double())
    for name, got, ref_ in (("dX", xg.grad, xr.grad), ("dW", layer.weight.grad, wr.grad), ("db", layer.bias.grad, br.grad)):
        assert torch.isfinite(got).all(), name
        e = _err(got, ref_)
        assert e <= ru.TOL32, f"{name}: element-wise error {e:.3e}"


def _wgrad_route(layer, x):
    """Route of the weight-gradient plan of a forward module (fc_wgrad_nd_plan_create)."""
    from fft_conv_pytorch_amd import _native
    n = x.ndim - 2
    desc = _native.conv_desc(n, x.shape[0], x.shape[1], layer.weight.shape[0], layer.groups, tuple(x.shape[2:]),
                             tuple(layer.weight.shape[2:]), layer.stride, layer.padding, layer.dilation, 0)
    plan = _native.WgradPlan(desc)
    return _native.read_route(plan._lib, plan._h)


def test_train_conv2d_on_rows_of_8192():
    from fft_conv_pytorch_amd import FFTConv2d
    torch.manual_seed(0)
    layer = FFTConv2d(3, 4, 3, padding=1)
    x = torch.randn(2, 3, 16, 8192, device=DEV)
    r = _wgrad_route(layer, x)
    assert r["nseg1"] > 1 and r["nseg0"] == 1, r
    _train(layer, x)


def test_train_conv3d_with_an_outer_axis_of_4500():
    from fft_conv_pytorch_amd import FFTConv3d
    torch.manual_seed(0)
    layer = FFTConv3d(2, 3, 3, padding=1)
    x = torch.randn(1, 2, 4500, 4, 5, device=DEV)
    r = _wgrad_route(layer, x)
    assert r["nseg0"] > 1 and r["nseg1"] == r["nseg2"] == 1, r
    _train(layer, x)


def test_train_conv2d_with_a_kernel_of_4500_taps():
    from fft_conv_pytorch_amd import FFTConv2d
    from fft_conv_pytorch_amd import functional as fc
    torch.manual_seed(0)
    layer = FFTConv2d(2, 3, (3, 4500), padding=(1, 0)).to(DEV)
    x = torch.randn(2, 2, 4, 5000, device=DEV)
    r = fc._plan_for(x, layer.weight, layer.bias, layer.stride, layer.padding, layer.dilation, 1, "constant").route
    assert r["nseg1"] > 1, r
    _train(layer, x)


def test_train_conv_transpose2d_on_a_long_row():
    from fft_conv_pytorch_amd import FFTConvTranspose2d
    torch.manual_seed(0)
    layer = FFTConvTranspose2d(3, 2, 3, stride=(1, 2), padding=1)
    _train(layer, torch.randn(2, 3, 8, 5000, device=DEV))


# ------------------------------------------------------------------------------------------ 4. nothing else moved
def test_unsegmented_routes_report_one_segment_per_axis(monkeypatch):
    """Every float32 N-d case of the route table plans as before: one segment per axis, layout words 4-6 zero."""
    from fft_conv_pytorch_amd import _native
    seen = 0
    for route in ru.ROUTES:
        for c in route.cases:
            if c.f64 or c.nd == 1:
                continue
            for k in ("FFTCONV_PLANES", "FFTCONV_XTILE", "FFTCONV_YTILE"):
                monkeypatch.delenv(k, raising=False)
            for k, v in {**route.env, **c.env}.items():
                if v is None:
                    monkeypatch.delenv(k, raising=False)
                else:
                    monkeypatch.setenv(k, v)
            _native.clear_plan_cache()
            kd = [(k - 1) * d + 1 for k, d in zip(c.k, c.tup(c.d))]
            x = torch.empty((c.B, c.cin) + tuple(c.size), device=DEV)
            plan = _plan(c, x, torch.empty(c.wshape, device=DEV), torch.empty(c.cout, device=DEV))
            r = plan.route
            assert r["kind"] == "f32_nd", (c.ident(), r)
            for ax in range(c.nd):
                assert r[f"nseg{ax}"] == 1 and r[f"seg_taps{ax}"] == c.k[ax], (c.ident(), r)
            assert plan.layout[4:7] == (0, 0, 0), (c.ident(), plan.layout)
            assert max(kd) <= 4096
            seen += 1
    assert seen >= 20, seen


# ------------------------------------------------------------------------------------------ 5. refusal
def test_more_than_64_segments_is_refused(monkeypatch):
    from fft_conv_pytorch_amd import _native
    # dilated extent 299,901: at most 41 taps of dilation 100 fit a 4096-point tile -> 74 segments
    key = (2, 1, 1, 1, 1, (4, 300000), (1, 3000), (1, 1), (0, 0), (1, 100), 0, False, 0, False, (0, 0), 0)
    with pytest.raises(NotImplementedError, match=r"\b74 segments"):
        _native.Plan(key)
    # the count is the product over the axes: 9 x 9 one-tap segments
    _set_seg(monkeypatch, 1)
    key = (2, 1, 1, 1, 1, (20, 20), (9, 9), (1, 1), (0, 0), (1, 1), 0, False, 0, False, (0, 0), 0)
    with pytest.raises(NotImplementedError, match=r"\b81 segments"):
        _native.Plan(key)


# ------------------------------------------------------------------------------------------ 6. capture and cache
def test_segmented_plan_replays_from_a_hip_graph():
    from fft_conv_pytorch_amd import FFTConv2d
    torch.manual_seed(0)
    layer = FFTConv2d(2, 3, (3, 4400), padding=(1, 10)).to(DEV).eval()
    x = torch.randn(2, 2, 10, 7000, device=DEV)
    with torch.no_grad():
        want = layer(x).clone()                 # warm: plan, tables, spectrum
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = layer(x)
        y.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(y, want)


def test_cached_spectrum_of_a_segmented_module_gives_the_uncached_result():
    from fft_conv_pytorch_amd import FFTConv2d
    torch.manual_seed(0)
    layer = FFTConv2d(2, 3, (3, 4400), padding=(1, 10)).to(DEV)
    x = torch.randn(2, 2, 10, 7000, device=DEV)
    with torch.no_grad():
        uncached = layer(x)                      # training mode, weight requires grad: transformed on every call
        layer.eval()
        first = layer(x)
        second = layer(x)                        # from the cached spectrum
    assert torch.equal(first, uncached) and torch.equal(second, uncached)
