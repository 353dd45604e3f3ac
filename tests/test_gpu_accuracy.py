"""The arithmetic of every kernel route against what float32 (float64) can deliver (tests/accuracy_util.py).

The route tables of test_gpu_routes.py, test_gpu_backward_routes.py and the fft_long_conv tests run once more, on integer
inputs whose float64 convolution is exact, in two input classes (centred, and offset by 64 so that the DC and Nyquist
bins carry energy).  Each result is measured as e_rms = rms(got - want) / rms(want) and e_max = max|got - want| / rms(want)
and held against the same measures of the model project's rfftn formulation, run in the case's precision on the same
tensors and device:  e_rms <= max(2 x baseline, 4 eps),  e_max <= max(3 x baseline, 16 eps).  A plan of kind f64_direct
runs no transform: its forward must be exact.  The old bounds (route_util.TOL32 / TOL64 on max/max) stay where they are, in the
files that prove where every sample goes; this file proves that the arithmetic is as good as it was.

Not measured: the 16-bit cases (their rounding is the store's; they are bit-compared with the cast path elsewhere), gradients
at N = 2**20 and 2**22 (forward only, on sampled dot products), and gradients of float32 rows at 64 x 64 points, which the
functional hands to fft_conv (the primitive's forward is measured; complex64 rows train at 64 x 64).

Every measurement is appended to ROWS (scripts/accuracy_report.py writes them out); one line per route, family or
factorisation reports the worst ratios, and the last test fails a table entry that was not measured."""
import math
import types

import pytest
import torch
import torch.nn.functional as F

from tests import accuracy_util as au
from tests import backward_util as bu
from tests import route_util as ru
from tests import test_gpu_backward_routes as tb
from tests import test_gpu_f64_long as t64
from tests import test_gpu_long_general as tl
from tests import test_gpu_nd_segments as ts
from tests import test_gpu_routes as tr

pytestmark = pytest.mark.gpu
DEV = tr.DEV
C = ru.Case
ROWS = []               # dict(family, route, case, quantity, cls, e_rms, base_e_rms, rms_ratio, e_max, base_e_max, max_ratio)
KNOBS = tuple(dict.fromkeys(tr.KNOBS + tl.KNOBS + t64.KNOBS + ("FFTCONV_LONG_NLC", "FFTCONV_NDSEG")))


def _clear():
    from fft_conv_pytorch_amd import _native, autograd as A, functional as fc
    _native.clear_plan_cache()
    A._BWD_PLANS.clear()
    fc._REFUSED_HALF.clear()


@pytest.fixture(autouse=True)
def _no_knob_plans_afterwards():
    """Neither the plan cache nor autograd's backward plans hold the knobs in their keys."""
    yield
    _clear()


def _knobs(monkeypatch, *envs):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    tr._knobs(monkeypatch, *envs)
    _clear()


def rms_margin(route_words):
    """The e_rms margin of a route: accuracy_util.RMS_MARGIN.  A route whose design performs more roundings than the
    baseline gets its own here, as a formula of its route words (never above accuracy_util.RMS_MARGIN_CAP)."""
    return au.RMS_MARGIN


def _chk(family, route, c, quantity, cls, got, want, base, dtype, exact=False, margin=au.RMS_MARGIN):
    assert got.shape == want.shape == base.shape, (quantity, tuple(got.shape), tuple(want.shape), tuple(base.shape))
    assert au.finite(got), f"{quantity}: {route} result not finite"
    m = au.measure(got, want, base, dtype)
    ROWS.append(dict(family=family, route=route, case=c if isinstance(c, str) else c.ident(), quantity=quantity, cls=cls, **m))
    au.assert_bound(f"{quantity} [{cls}]", m, margin, exact)
    return m


def _report(kind, name, first_row):
    rows = ROWS[first_row:]
    assert rows, f"{name}: nothing measured"
    print(f"\n{kind} {name}: {len(rows)} measurements, worst e_rms ratio {max(r['rms_ratio'] for r in rows):.2f}, "
          f"worst e_max ratio {max(r['max_ratio'] for r in rows):.2f}")


def _each(kind, name, cases, fn):
    first = len(ROWS)
    for c in cases:
        for cls in au.CLASSES:
            print(f"  {name} / {c.ident()} [{cls}]")
            try:
                fn(c, cls)
            except AssertionError as e:
                raise AssertionError(f"{name} / {c.ident()} [{cls}]: {e}") from None
    torch.cuda.synchronize()
    _report(kind, name, first)


# ------------------------------------------------------------------------------------------------ forward routes
def _route_case(family, route, c, cls, monkeypatch):
    from fft_conv_pytorch_amd import functional as fc
    from fft_conv_pytorch_amd.functional import fft_conv, fft_conv_transpose
    _knobs(monkeypatch, route.env, c.env)
    au.assert_exact(c, cls)
    dtype = au.case_dtype(c)
    x, w, b = au.inputs(c, cls, DEV)
    kw = tr._kw(c)
    plan = fc._plan_for(x, w, b, kw["stride"], kw["padding"], kw["dilation"], c.g, "constant" if c.tr else c.mode,
                        transposed=c.tr, output_padding=kw.get("output_padding", 0))
    r = plan.route
    assert route.pred(r), f"plan is on another route: {r}"
    assert c.expect is None or c.expect(r), f"case not sized as intended: {r}"
    exact, margin = r["kind"] == "f64_direct", rms_margin(r)
    seams = tr._seams(c, r, plan.layout[3])
    spec = fc.transform_kernel(plan, w)
    got = tr._plan_forward(plan, x, spec, b)
    assert au.finite(got), f"forward: {int((~torch.isfinite(got)).sum())} output samples not written / not finite"
    base = au.baseline(c, x, w, b)
    if got.numel() <= ru.FULL_REF_MAX:
        want = au.truth(c, x, w, b, seams)
    else:
        idx = tr._sample_idx(c, tuple(got.shape), seams)
        want = au.sampled(c, x, w, b, idx)
        assert au.is_whole(want)
        at = tuple(idx.t().to(DEV))
        got, base = got[at], base[at]
    _chk(family, route.name, c, "y", cls, got, want, base, dtype, exact, margin)
    if not c.grads:
        return
    only_dx = math.prod(c.size) * c.B * max(c.cin, c.cout) > ru.FULL_REF_MAX
    xg = x.clone().requires_grad_()
    wg, bg = (t.clone().requires_grad_(not only_dx) for t in (w, b))
    y = (fft_conv_transpose if c.tr else fft_conv)(xg, wg, bg, **kw)
    gy = au.grad_output(y.shape, dtype, DEV)
    y.backward(gy)
    want_g = au.truth_grads(c, x, w, b, gy, only_dx=only_dx)
    base_g = au.baseline_grads(c, x, w, b, gy, only_dx=only_dx)[1:]
    # (the gradients run plans of their own -- a transposed plan, role-swapped forward plans, fc_wgrad* -- whose kind this
    #  plan's route does not tell: they are held to the bound, "exact" is the forward plan's)
    for name, got_, want_, base_ in zip(("dX", "dW", "db"), (xg.grad, wg.grad, bg.grad), want_g, base_g):
        if want_ is not None:
            _chk(family, route.name, c, name, cls, got_, want_, base_, dtype, False, margin)


@pytest.mark.parametrize("route", ru.ROUTES, ids=[r.name for r in ru.ROUTES])
def test_route(route, monkeypatch):
    assert route.cases, f"{route.name}: no cases"
    _each("route", route.name, route.cases, lambda c, cls: _route_case("forward", route, c, cls, monkeypatch))


@pytest.mark.parametrize("route", ru.TRANSPOSED_ROUTES, ids=[r.name for r in ru.TRANSPOSED_ROUTES])
def test_transposed_route(route, monkeypatch):
    assert route.cases, f"{route.name}: no cases"
    _each("route", "T:" + route.name, route.cases,
          lambda c, cls: _route_case("transposed", types.SimpleNamespace(name="T:" + route.name, env=route.env, pred=route.pred),
                                     c, cls, monkeypatch))


# ------------------------------------------------------------------------------------------------ backward routes
def _wgrad_inputs(c, cls, dtype=torch.float32):
    au.assert_exact(c, cls)
    x, w, b = au.inputs(c, cls, DEV)
    gy = au.grad_output((c.B, c.cout) + au.out_spatial(c), dtype, DEV)
    return x, w, b, gy


def _wgrad_chk(family, name, c, cls, x, w, b, gy, dw, db):
    want = au.truth_grads(c, x, w, b, gy)
    base = au.baseline_grads(c, x, w, b, gy)[1:]
    _chk(family, name, c, "dW", cls, dw, want[1], base[1], x.dtype)
    if db is not None:
        _chk(family, name, c, "db", cls, db, want[2], base[2], x.dtype)


def _wgrad1d_case(family, c, cls, monkeypatch):
    from fft_conv_pytorch_amd import _native, autograd as A
    _knobs(monkeypatch, family.env, c.env)
    geo = bu.wgrad_geometry(c, tb._cus())
    assert geo is not None, "the restated geometry refuses the case"
    assert _native.wgrad1d_slices(tb._desc(c)) == geo["slices"], f"the library's slices differ from {geo}"
    assert family.pred(geo), f"case is outside its family: {geo}"
    assert c.expect is None or c.expect(geo), f"case not sized as intended: {geo}"
    x, w, b, gy = _wgrad_inputs(c, cls)
    got = A._grad_weight_native(x, gy, *tb._args(c), want_db=True)
    assert got is not None, "fc_wgrad1d refused the case"
    assert (got[1] is None) == geo["diag"], "db rides the dense kernel's launch only"
    _wgrad_chk("wgrad1d", family.name, c, cls, x, w, b, gy, *got)


@pytest.mark.parametrize("family", bu.WGRAD1D_FAMILIES, ids=[f.name for f in bu.WGRAD1D_FAMILIES])
def test_wgrad1d_family(family, monkeypatch):
    assert family.cases, f"{family.name}: no cases"
    _each("family", family.name, family.cases, lambda c, cls: _wgrad1d_case(family, c, cls, monkeypatch))


def _refusal_case(name, c, cls, chunked, monkeypatch):
    from fft_conv_pytorch_amd import _native, autograd as A
    _knobs(monkeypatch, c.env)
    assert bu.wgrad_geometry(c, tb._cus()) is None and _native.wgrad1d_slices(tb._desc(c)) == 0, "fc_wgrad1d covers the shape"
    assert bu.chunk_plan(c)[0] == chunked
    x, w, b, gy = _wgrad_inputs(c, cls)
    _wgrad_chk("wgrad-forward-plans", name, c, cls, x, w, b, gy, A._grad_weight_plans(x, gy, *tb._args(c)), None)


@pytest.mark.parametrize("name,c,chunked,sized", bu.REFUSALS, ids=[r[0] for r in bu.REFUSALS])
def test_forward_plan_dw(name, c, chunked, sized, monkeypatch):
    _each("family", name, [c], lambda c_, cls: _refusal_case(name, c_, cls, chunked, monkeypatch))


def _transposed_dw_case(name, c, cls, monkeypatch):
    _knobs(monkeypatch, c.env)
    au.assert_exact(c, cls)
    dtype = au.case_dtype(c)
    x, w, b = au.inputs(c, cls, DEV)
    gy = au.grad_output((c.B, c.cout) + au.out_spatial(c), dtype, DEV)
    spies = tb._Spies(monkeypatch)
    y, dx, dw, db, _ = tb._step(c, x, w, b, gy)
    assert (spies.plans == [True] and not spies.w1d) if c.f64 else (len(spies.w1d) == 1 and not spies.plans), \
        f"the step launched {spies}"
    want = (au.truth(c, x, w, b),) + au.truth_grads(c, x, w, b, gy)
    base = au.baseline_grads(c, x, w, b, gy)
    for q, got_, want_, base_ in zip(("y", "dX", "dW", "db"), (y, dx, dw, db), want, base):
        _chk("transposed-dw", name, c, q, cls, got_, want_, base_, dtype)


@pytest.mark.parametrize("name,c", bu.TRANSPOSED_DW, ids=[t[0] for t in bu.TRANSPOSED_DW])
def test_transposed_dw(name, c, monkeypatch):
    _each("family", name, [c], lambda c_, cls: _transposed_dw_case(name, c_, cls, monkeypatch))


def _wgrad_nd_case(name, env, c, cls, pred, monkeypatch):
    from fft_conv_pytorch_amd import autograd as A
    _knobs(monkeypatch, env, c.env)
    x, w, b, gy = _wgrad_inputs(c, cls)
    layer = types.SimpleNamespace(weight=w, groups=c.g, stride=c.tup(c.s), padding=c.tup(c.p), dilation=c.tup(c.d))
    route = ts._wgrad_route(layer, x)
    assert pred is None or pred(route), f"case not sized as intended: {route}"
    dw = A._grad_weight_nd_native(x, gy, *tb._args(c))
    assert dw is not None, "fc_wgrad_nd refused the case"
    _wgrad_chk("wgrad-nd", name, c, cls, x, w, b, gy, dw, None)


@pytest.mark.parametrize("name,env,c,pred", bu.WGRAD_ND, ids=[n[0] for n in bu.WGRAD_ND])
def test_wgrad_nd(name, env, c, pred, monkeypatch):
    _each("family", name, [c], lambda c_, cls: _wgrad_nd_case(name, env, c_, cls, pred, monkeypatch))


# ------------------------------------------------------------------------------------------------ fft_long_conv
LONG_FACTORS = tl.COLUMN_GEOMETRIES + [(64, 64)]
LONG_KINDS = ("float32", "complex64", "channels-last")


@pytest.fixture
def long_ran(monkeypatch):
    """(N1, N2) of every long plan whose forward ran."""
    from fft_conv_pytorch_amd import _native
    seen = []
    for attr in ("forward", "forward_lay"):
        real = getattr(_native.LongPlan, attr)

        def spy(plan, *a, _real=real, **k):
            seen.append((plan.info["N1"], plan.info["N2"]))
            return _real(plan, *a, **k)
        monkeypatch.setattr(_native.LongPlan, attr, spy)
    return seen


def _long_case(N1, N2, g):
    """The smallest row that fills the transform: L + K - 1 = N1 N2 - 1, a quarter of it taps."""
    N = N1 * N2
    K = N // 4 + 1
    return C(2, 4, 4, (N - K,), (K,), g=g, note=f"{N1}x{N2}")


def _long_run(c, cls, kind, long_ran):
    """y (and gradients where the functional reaches this factorisation) of one fft_long_conv case."""
    from fft_conv_pytorch_amd import fft_long_conv
    from fft_conv_pytorch_amd import functional as fc
    cx = kind == "complex64"
    dtype = torch.complex64 if cx else torch.float32
    au.assert_exact(c, cls, cx)
    x, w, b = au.inputs(c, cls, DEV, complex_=cx)
    if kind == "channels-last":
        x = x.transpose(1, 2).contiguous().transpose(1, 2)
        assert fc._long_layout(x) == "nlc" and tuple(x.stride()) == (c.size[0] * c.cin, 1, c.cin)
    want = au.truth_by_fft(c, x, w, b)
    del long_ran[:]
    primitive = c.size[0] <= fc.LONG_HANDOFF_POINTS and not cx
    if primitive:
        # a real row of at most 4096 points goes to fft_conv in the functional: the primitive itself, forward only
        y = fc._long_run(x, w, b, 0, 0, False, 0, c.g)
        grads = None
    else:
        xg, wg, bg = (t.clone().requires_grad_() for t in (x, w, b))
        if kind == "channels-last":
            xg = x.detach().requires_grad_()
        y = fft_long_conv(xg, wg, bg, groups=c.g)
        gy = au.grad_output(y.shape, dtype, DEV)
        y.backward(gy)
        grads = (xg.grad, wg.grad, bg.grad)
        y = y.detach()
    torch.cuda.synchronize()
    base = au.baseline_grads(c, x.contiguous(), w, b, gy) if grads else (au.baseline(c, x.contiguous(), w, b),)
    return dtype, (y,) + (grads or ()), (want,) + (au.truth_grads(c, x, w, b, gy, by_fft=True) if grads else ()), base


@pytest.mark.parametrize("N1,N2", LONG_FACTORS, ids=[f"{a}x{b}" for a, b in LONG_FACTORS])
def test_long_conv_factorisation(N1, N2, monkeypatch, long_ran):
    name = f"long-{N1}x{N2}"
    first = len(ROWS)
    for g in (1, 4):
        c = _long_case(N1, N2, g)
        for kind in LONG_KINDS:
            for cls in au.CLASSES:
                _knobs(monkeypatch, {"FFTCONV_LONG_N": f"{N1}x{N2}"})
                print(f"  {name} / {c.ident()} {kind} [{cls}]")
                dtype, got, want, base = _long_run(c, cls, kind, long_ran)
                assert long_ran and set(long_ran) == {(N1, N2)}, f"the plans that ran: {long_ran}"
                assert len(long_ran) >= (1 if len(got) == 1 else 3), long_ran       # (y, then dX and dW)
                for q, got_, want_, base_ in zip(("y", "dX", "dW", "db"), got, want, base):
                    _chk("fft_long_conv", name, f"{c.ident()}-{kind}", q, cls, got_, want_, base_, dtype)
    _report("factorisation", name, first)


@pytest.mark.parametrize("lg", [20, 22])
def test_largest_transforms(lg, monkeypatch, long_ran):
    """One causal row of K = L = N / 2 samples, one channel: where the two-table twiddle thi[m >> 12] * tlo[m & 4095] of the
    long transforms matters.  No direct convolution reaches this size: the truth is explicit float64 dot products at 1500
    positions plus the row ends, and kernel and baseline are measured there."""
    from fft_conv_pytorch_amd import fft_long_conv
    _knobs(monkeypatch)
    N = 1 << lg
    L = K = N // 2
    name = f"long-2^{lg}"
    first = len(ROWS)
    # the causal form as a forward case: K - 1 zeros in front of the row, the taps flipped
    c = C(1, 1, 1, (L + K - 1,), (K,), note="causal")
    for cls in au.CLASSES:
        au.assert_exact(c, cls)
        x, w, b = au.inputs(C(1, 1, 1, (L,), (K,)), cls, DEV)
        del long_ran[:]
        y = fft_long_conv(x, w, b, causal=True)
        torch.cuda.synchronize()
        assert len(long_ran) == 1 and long_ran[0][0] * long_ran[0][1] == N, long_ran
        xp, wf = F.pad(x, (K - 1, 0)), w.flip(-1)
        idx = tr._sample_idx(c, (1, 1, L), [[]], 1500)
        want = au.sampled(c, xp, wf, b, idx)
        assert au.is_whole(want)
        at = tuple(idx.t().to(DEV))
        base = au.baseline(c, xp, wf, b)
        assert y.shape == base.shape == (1, 1, L)
        _chk("fft_long_conv", name, c, "y", cls, y[at], want, base[at], torch.float32)
    _report("transform", name, first)


# ------------------------------------------------------------------------------------------------ float64 long route
F64_LONG = [(fac, C(3, 4, 6, (2500 if fac in ("64x64",) else 3000,), (1100,), g=2, f64=True, note=fac)) for fac in t64.FACTORS]
F64_LONG += [("own", c) for c in t64.OWN]


@pytest.mark.parametrize("fac,c", F64_LONG, ids=[f"{f}-{c.ident()}" for f, c in F64_LONG])
def test_f64_long_route(fac, c, monkeypatch):
    from fft_conv_pytorch_amd import functional as fc
    name = "f64-long-" + (fac if fac != "own" else c.ident())
    first = len(ROWS)
    for cls in au.CLASSES:
        _knobs(monkeypatch, {} if fac == "own" else {"FFTCONV_F64_LONG_N": fac, "FFTCONV_F64_LONG": "2"})
        au.assert_exact(c, cls)
        x, w, b = au.inputs(c, cls, DEV)
        plan = fc._plan_for(x, w, b, c.s, c.p, c.d, c.g, c.mode)
        r = plan.route
        assert r["kind"] == "f64_fft_long" and r["ntiles"] == 1, r
        if fac == "own":
            assert r["N1"] <= r["N2"], r
        else:
            assert f"{r['N1']}x{r['N2']}" == fac, r
        got = tr._plan_forward(plan, x, fc.transform_kernel(plan, w), b)
        _chk("f64-long", name, c, "y", cls, got, au.truth(c, x, w, b), au.baseline(c, x, w, b), torch.float64)
    _report("route", name, first)


# ------------------------------------------------------------------------------------------------ the cap
def test_every_table_entry_was_measured():
    """Every route, family and factorisation of the tables has rows in this run of the file, in both input classes."""
    expected = {r.name for r in ru.ROUTES} | {"T:" + r.name for r in ru.TRANSPOSED_ROUTES}
    expected |= {f.name for f in bu.WGRAD1D_FAMILIES} | {r[0] for r in bu.REFUSALS} | {t[0] for t in bu.TRANSPOSED_DW}
    expected |= {n[0] for n in bu.WGRAD_ND} | {f"long-{a}x{b}" for a, b in LONG_FACTORS} | {"long-2^20", "long-2^22"}
    expected |= {"f64-long-" + (f if f != "own" else c.ident()) for f, c in F64_LONG}
    seen = {cls: {r["route"] for r in ROWS if r["cls"] == cls} for cls in au.CLASSES}
    for cls in au.CLASSES:
        missing = sorted(expected - seen[cls])
        assert not missing, f"not measured [{cls}]: {missing}"
