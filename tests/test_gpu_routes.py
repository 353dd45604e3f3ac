"""Every kernel route the planners pick (tests/route_util.py), each checked against float64.

For every case of a route: the plan reports that route (``Plan.route``, fc_debug_route); its forward, run through
``transform_kernel`` and ``Plan.forward`` into an output filled with NaN, writes every sample and matches torch's float64
convolution element-wise (max|got - want| / max|want|: 1e-4 for float32 plans, 1e-12 for float64 ones); a seam probe --
unit impulses at the row ends, the padding boundary and both sides of every tile seam -- matches too, so that a wrong tap
row at a seam cannot hide in a large output.  Cases marked ``public`` also run through fft_conv / fft_conv_transpose, and
cases marked ``grads`` check dX (transposed plan), dW and db through autograd.  Outputs past route_util.FULL_REF_MAX
samples are checked on sampled float64 dot products.  One line per route reports the cases run and the worst error."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import route_util as ru

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOBS = ("FFTCONV_PERS", "FFTCONV_PH2", "FFTCONV_TILE", "FFTCONV_DENSE", "FFTCONV_DENSE_SLAB", "FFTCONV_PLANES",
         "FFTCONV_WIDE", "FFTCONV_DIAG", "FFTCONV_XTILE", "FFTCONV_YTILE", "FFTCONV_F64_FFT", "FFTCONV_ZEROWRAP")


@pytest.fixture(autouse=True)
def _no_knob_plans_afterwards():
    """The plan cache key does not hold the knobs: plans built under them must not outlive the test, failed or not."""
    yield
    from fft_conv_pytorch_amd import _native
    _native.clear_plan_cache()


def _knobs(monkeypatch, *envs):
    from fft_conv_pytorch_amd import _native
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for env in envs:
        for k, v in env.items():
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, v)
    _native.clear_plan_cache()


def _err(got, want):
    return (got.double() - want.double()).abs().max().item() / max(want.double().abs().max().item(), 1e-300)


def _kw(c):
    if c.tr:
        return dict(stride=c.tup(c.s), padding=c.tup(c.p), output_padding=c.tup(c.op), dilation=c.tup(c.d), groups=c.g)
    return dict(stride=c.tup(c.s), padding=c.tup(c.p), dilation=c.tup(c.d), groups=c.g, padding_mode=c.mode)


def _reference(c, x, w, b):
    """torch's float64 convolution (forward or transposed) of float64 tensors."""
    nd = c.nd
    if c.tr:
        fn = (F.conv_transpose1d, F.conv_transpose2d, F.conv_transpose3d)[nd - 1]
        return fn(x, w, b, stride=c.tup(c.s), padding=c.tup(c.p), output_padding=c.tup(c.op), groups=c.g,
                  dilation=c.tup(c.d))
    conv = (F.conv1d, F.conv2d, F.conv3d)[nd - 1]
    pads = c.tup(c.p)
    if c.mode == "constant":
        return conv(x, w, b, stride=c.tup(c.s), padding=pads, dilation=c.tup(c.d), groups=c.g)
    flat = [q for p in reversed(pads) for q in (p, p)]
    return conv(F.pad(x, flat, mode=c.mode), w, b, stride=c.tup(c.s), dilation=c.tup(c.d), groups=c.g)


def _sampled(c, x, w, b, idx):
    """float64 dot products of a forward (not transposed) convolution at the output positions idx (n, 2 + nd)."""
    pads = c.tup(c.p)
    flat = [q for p in reversed(pads) for q in (p, p)]
    xp = F.pad(x.double(), flat, mode=c.mode) if c.mode != "constant" else F.pad(x.double(), flat)
    w, b = w.double(), None if b is None else b.double()
    s, d, k = c.tup(c.s), c.tup(c.d), c.k
    cig, cog = c.cin // c.g, c.cout // c.g
    vals = []
    for row in idx.tolist():
        bi, o, pos = row[0], row[1], row[2:]
        g = o // cog
        win = xp[bi, g * cig:(g + 1) * cig]
        sl = tuple(slice(pos[a] * s[a], pos[a] * s[a] + (k[a] - 1) * d[a] + 1, d[a]) for a in range(c.nd))
        v = (win[(slice(None),) + sl] * w[o]).sum()
        vals.append(v + (b[o] if b is not None else 0.0))
    return torch.stack(vals)


def _seams(c, r, seg_taps):
    """Output seams (stride-1 output coordinates) of every tiled axis of the plan, per axis (seg_taps: taps per segment
    of a segmented 1-D plan, its layout word 3)."""
    nd, kd = c.nd, [(k - 1) * d + 1 for k, d in zip(c.k, c.tup(c.d))]
    seams = [[] for _ in range(nd)]
    kind = r["kind"]
    if kind == "f32_1d":
        ph, d0 = r["ph"], c.tup(c.d)[0]
        if ph > 1:
            kt = c.k[0]
        elif r["nseg"] > 1:
            kt = (seg_taps - 1) * d0 + 1
        else:
            kt = kd[0]
        V = r["T"] - kt + 1
        seams[0] = [j * V * ph for j in range(1, r["ntiles"])]
    elif kind == "f32_nd":
        tiled = [(0, r["T"], r["ntiles"]), (nd - 1, r["Tx"], r["nxt"])] + ([(1, r["Tm"], r["nyt"])] if nd == 3 else [])
        for ax, T, n in tiled:
            seams[ax] = [j * (T - kd[ax] + 1) for j in range(1, n)]
    elif kind == "f64_fft_1d":
        seams[0] = [j * (r["T"] - kd[0] + 1) for j in range(1, r["ntiles"])]
    elif kind == "f64_fft_nd":
        for ax in range(nd):
            T, n = r[f"t{ax}"], r[f"nt{ax}"]
            seams[ax] = [j * (T - kd[ax] + 1) for j in range(1, n)]
    return seams


def seam_probe(c, seams, dtype):
    """Zeros plus unit impulses, on every channel, at the first and last samples, at the padding boundary and at the
    input samples that meet both sides of every tile seam (the first and the last tap of the outputs around it)."""
    kd = [(k - 1) * d + 1 for k, d in zip(c.k, c.tup(c.d))]
    x = torch.zeros((c.B, c.cin) + tuple(c.size), dtype=dtype, device=DEV)
    masks = []
    for ax in range(c.nd):
        S, p, s = c.size[ax], c.tup(c.p)[ax], c.tup(c.s)[ax]
        pos = {0, 1, S - 2, S - 1, p - 1, p, p + 1, S - 1 - p, S - p}
        for o in seams[ax]:
            for q in (o - 1, o, o + 1):
                if c.tr:
                    padl = kd[ax] - 1 - p
                    pos.update({(q - padl) // s, (q + kd[ax] - 1 - padl) // s})
                else:
                    pos.update({q - p, q - p + kd[ax] - 1})
        m = torch.zeros(S, dtype=torch.bool)
        m[[v for v in pos if 0 <= v < S]] = True
        shape = [1] * c.nd
        shape[ax] = S
        masks.append(m.view(shape))
    mask = masks[0]
    for m in masks[1:]:
        mask = mask & m
    x[:, :] = mask.to(dtype).to(DEV)
    return x


def _plan_forward(plan, x, spec, b):
    """Plan.forward into an output filled with NaN: a sample the kernels never store stays NaN."""
    from fft_conv_pytorch_amd import functional as fc
    out = torch.full((x.shape[0], plan.key[3]) + plan.out_spatial, float("nan"), dtype=plan.dtype, device=DEV)
    ws = fc.new_workspace(plan, x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    plan.forward(x.data_ptr(), spec.buf.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr() if ws is not None else None,
                 stream)
    return out


def _sample_idx(c, shape, seams, n=1500):
    """Random output positions plus every row end and every tile seam (both sides) of each axis."""
    gen = torch.Generator().manual_seed(5)
    cols = [torch.randint(0, shape[i], (n,), generator=gen) for i in range(len(shape))]
    extra = []
    for ax in range(c.nd):
        L = shape[2 + ax]
        s = c.tup(c.s)[ax]
        for o in [0, 1, L - 2, L - 1] + [q // s for j in seams[ax] for q in (j - 1, j, j + 1)]:
            if 0 <= o < L:
                for _ in range(4):
                    row = [int(torch.randint(0, shape[i], (1,), generator=gen)) for i in range(len(shape))]
                    row[2 + ax] = o
                    extra.append(row)
    idx = torch.stack(cols, 1)
    if extra:
        idx = torch.cat([idx, torch.tensor(extra)], 0)
    return idx


def _check(c, seams, got, x, w, b, tol, what):
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} output samples not written / not finite"
    if got.numel() <= ru.FULL_REF_MAX:
        want = _reference(c, x.double(), w.double(), b.double())
        assert got.shape == want.shape, (got.shape, want.shape)
        err = _err(got, want)
    else:
        idx = _sample_idx(c, tuple(got.shape), seams)
        want = _sampled(c, x, w, b, idx)
        g = got[tuple(idx.t().to(DEV))]
        err = _err(g, want)
    assert err <= tol, f"{what}: element-wise error {err:.3e} > {tol}"
    return err


def _grads(c, x, w, b, tol, only_dx):
    """dX / dW / db through autograd (transposed plan, fc_wgrad1d* / fc_wgrad_nd) against float64 autograd."""
    from fft_conv_pytorch_amd.functional import fft_conv, fft_conv_transpose
    op = fft_conv_transpose if c.tr else fft_conv
    xg = x.clone().requires_grad_()
    wg, bg = (w.clone().requires_grad_(), b.clone().requires_grad_()) if not only_dx else (w, b)
    y = op(xg, wg, bg, **_kw(c))
    gy = torch.randn(y.shape, generator=torch.Generator(device=DEV).manual_seed(9), device=DEV, dtype=y.dtype)
    y.backward(gy)
    worst = 0.0
    if only_dx:
        # stride 1, groups 1: dX is the convolution of dY with the flipped, channel-swapped kernel, padding kd - 1 - p
        assert not c.tr and c.g == 1 and all(s == 1 for s in c.tup(c.s)) and c.mode == "constant"
        wt = w.flip(list(range(2, 2 + c.nd))).transpose(0, 1).contiguous()
        cd = ru.Case(c.B, c.cout, c.cin, tuple(y.shape[2:]), c.k, p=tuple((k - 1) * d - p for k, d, p in
                                                                         zip(c.k, c.tup(c.d), c.tup(c.p))), d=c.d)
        no_seams = [[] for _ in range(c.nd)]
        return _check(cd, no_seams, xg.grad, gy, wt, torch.zeros(c.cin, device=DEV, dtype=x.dtype), tol, "dX")
    xr, wr, br = (t.double().clone().requires_grad_() for t in (x, w, b))
    want = _reference(c, xr, wr, br)
    want.backward(gy.double())
    for name, got_, want_ in (("dX", xg.grad, xr.grad), ("dW", wg.grad, wr.grad), ("db", bg.grad, br.grad)):
        assert torch.isfinite(got_).all(), name
        e = _err(got_, want_)
        assert e <= tol, f"{name}: element-wise error {e:.3e} > {tol}"
        worst = max(worst, e)
    return worst


def _run_case(route, c, monkeypatch):
    from fft_conv_pytorch_amd import functional as fc
    from fft_conv_pytorch_amd.functional import fft_conv, fft_conv_transpose
    _knobs(monkeypatch, route.env, c.env)
    dtype = torch.float64 if c.f64 else torch.float32
    tol = ru.TOL64 if c.f64 else ru.TOL32
    gen = torch.Generator(device=DEV).manual_seed(sum(c.size) + 7 * c.B + c.cin)
    x = torch.randn((c.B, c.cin) + tuple(c.size), generator=gen, device=DEV, dtype=dtype)
    w = torch.randn(c.wshape, generator=gen, device=DEV, dtype=dtype) / math.sqrt(math.prod(c.wshape[1:]))
    b = torch.randn(c.cout, generator=gen, device=DEV, dtype=dtype)
    kw = _kw(c)
    plan = fc._plan_for(x, w, b, kw["stride"], kw["padding"], kw["dilation"], c.g, "constant" if c.tr else c.mode,
                        transposed=c.tr, output_padding=kw.get("output_padding", 0))
    r = plan.route
    assert route.pred(r), f"plan is on another route: {r}"
    seams = _seams(c, r, plan.layout[3])
    spec = fc.transform_kernel(plan, w)
    worst = _check(c, seams, _plan_forward(plan, x, spec, b), x, w, b, tol, "forward")
    probe = seam_probe(c, seams, dtype)
    worst = max(worst, _check(c, seams, _plan_forward(plan, probe, spec, b), probe, w, b, tol, "seam probe"))
    if c.public:
        op = fft_conv_transpose if c.tr else fft_conv
        worst = max(worst, _check(c, seams, op(x, w, b, **kw), x, w, b, tol, "public op"))
    if c.grads:
        only_dx = math.prod(c.size) * c.B * max(c.cin, c.cout) > ru.FULL_REF_MAX
        worst = max(worst, _grads(c, x, w, b, tol, only_dx))
    torch.cuda.synchronize()
    # (after the values: a work list that loses items shows as unwritten samples first)
    if c.expect is not None:
        assert c.expect(r), f"case not sized as intended: {r}"
    return worst


@pytest.mark.parametrize("route", ru.ROUTES, ids=[r.name for r in ru.ROUTES])
def test_route(route, monkeypatch):
    assert route.cases, f"{route.name}: no cases"
    worst = 0.0
    for c in route.cases:
        try:
            worst = max(worst, _run_case(route, c, monkeypatch))
        except AssertionError as e:
            raise AssertionError(f"{route.name} / {c.ident()}: {e}") from None
    print(f"\nroute {route.name}: {len(route.cases)} cases, worst element-wise error {worst:.2e}")


def test_refused_block_layout_leaves_no_trace(monkeypatch):
    """Depthwise channels and groups of 2 channels are first planned as 8 x 8 blocks for the batch-sharing kernel.  Under
    FFTCONV_PERS=0 that kernel refuses them, and the plan must be the one the plain grouped layout gets when the blocks
    are never tried (FFTCONV_DIAG=0): same route, layout and sizes, and a forward that matches float64."""
    from fft_conv_pytorch_amd import functional as fc
    for c in (ru.Case(2, 16, 16, (4096,), (33,), g=16, note="depthwise"), ru.Case(2, 16, 16, (4096,), (33,), g=8, note="gs2")):
        gen = torch.Generator(device=DEV).manual_seed(11)
        x = torch.randn((c.B, c.cin) + c.size, generator=gen, device=DEV)
        w = torch.randn(c.wshape, generator=gen, device=DEV) / math.sqrt(math.prod(c.wshape[1:]))
        b = torch.randn(c.cout, generator=gen, device=DEV)
        seen = []
        for env in ({"FFTCONV_PERS": "0"}, {"FFTCONV_PERS": "0", "FFTCONV_DIAG": "0"}):
            _knobs(monkeypatch, env)
            plan = fc._plan_for(x, w, b, 1, 0, 1, c.g, "constant")
            seen.append((plan.route, plan.layout, plan.tile, plan.spectrum_bytes, plan.workspace_bytes, plan.out_spatial,
                         plan.debug_grid()))
        assert seen[0] == seen[1], f"{c.ident()}: a refused block layout shows in the plan: {seen}"
        assert ru.GENERAL_1D(seen[0][0]), f"{c.ident()}: {seen[0][0]}"
        _knobs(monkeypatch, {"FFTCONV_PERS": "0"})
        plan = fc._plan_for(x, w, b, 1, 0, 1, c.g, "constant")
        err = _check(c, [[]], _plan_forward(plan, x, fc.transform_kernel(plan, w), b), x, w, b, ru.TOL32, "forward")
        print(f"\n{c.ident()}: element-wise error {err:.2e}")
