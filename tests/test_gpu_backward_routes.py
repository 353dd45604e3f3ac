"""The backward routes at the edges of their own planners (tests/backward_util.py, route_util.TRANSPOSED_ROUTES).

1. fc_wgrad1d: families of cases sized for the limits of ``wgrad_geometry`` -- slice split, stride 64, dilation 512, 64 tap
   segments, 64 channels per group, the strided depthwise kernel, the bounds of the loaders' interior path.  A spy on
   ``_native.wgrad1d_db`` proves which kernel ran and with how many slices; the geometry restated in Python must give the
   library's slice count.
2. One step past each limit: the forward-plan dW of ``_grad_weight_plans``, chunked and not, and the zero-extended weight
   gradient of fft_conv_transpose.
3. dX: strided transposed plans on every route that takes them, through ``test_gpu_routes._run_case`` (route predicate,
   NaN-filled output, float64 reference, seam probe); the 1-D kernels that refuse such plans are pinned to the general one.
4. fc_wgrad_nd: batch remainders of the contraction, stride tails, segments on the last and the outer axis, ragged groups.

Every case: y, dX, dW and db of a whole training step through fft_conv / fft_conv_transpose against torch's float64
convolution autograd (max|got - want| / max|want| <= route_util.TOL32 / TOL64), then dW and db through the entry the family
is about, on random rows and on two probes -- dY reduced to impulses around every tile start, x reduced to impulses at the
ends of every tile window -- element-wise against the same truth.  One line per family reports its cases and worst error;
the last test fails a family that ran no case."""
import math
import types

import pytest
import torch

from tests import backward_util as bu
from tests import guard_util as gu
from tests import route_util as ru
from tests import test_gpu_nd_segments as ts
from tests import test_gpu_routes as tr

pytestmark = pytest.mark.gpu
DEV = tr.DEV
RAN = set()                 # families and transposed routes whose cases passed (the last test compares it)
CODE = {torch.float32: 0, torch.float16: 2, torch.bfloat16: 3}


@pytest.fixture(autouse=True)
def _no_knob_plans_afterwards():
    """Neither the plan cache nor autograd's backward plans hold the knobs in their keys."""
    yield
    from fft_conv_pytorch_amd import _native, autograd as A
    _native.clear_plan_cache()
    A._BWD_PLANS.clear()


def _knobs(monkeypatch, *envs):
    from fft_conv_pytorch_amd import autograd as A
    tr._knobs(monkeypatch, *envs)
    A._BWD_PLANS.clear()


class _Spies:
    """What a backward launched: every fc_wgrad1d call (slices, db rider, depthwise kernel, dtype code), every fc_wgrad_nd
    run, and for every forward-plan dW whether it took the chunked branch."""

    def __init__(self, monkeypatch):
        from fft_conv_pytorch_amd import _native, autograd as A
        self.w1d, self.wnd, self.plans = [], [], []
        real_db, real_run, real_plans = _native.wgrad1d_db, _native.WgradPlan.run, A._grad_weight_plans

        def wgrad1d_db(desc, x_ptr, dy_ptr, part_ptr, db_ptr, row, slices, stream):
            # (the depthwise kernel is the one without a bias-gradient output)
            self.w1d.append(dict(slices=slices, db=db_ptr is not None, diag=not _native.wgrad1d_db_supported(desc),
                                 dtype=int(desc.dtype), stride=int(desc.stride[0])))
            return real_db(desc, x_ptr, dy_ptr, part_ptr, db_ptr, row, slices, stream)

        def run(plan, *a):
            self.wnd.append(plan)
            return real_run(plan, *a)

        def plans(x, grad, wshape, stride, *a):
            kext = (grad.shape[2] - 1) * stride[0] + 1
            kd0 = (wshape[2] - 1) * a[1][0] + 1
            self.plans.append(x.ndim == 3 and kext > max(A._DW_TILE - kd0 + 1, A._DW_TILE // 4))
            return real_plans(x, grad, wshape, stride, *a)
        monkeypatch.setattr(_native, "wgrad1d_db", wgrad1d_db)
        monkeypatch.setattr(_native.WgradPlan, "run", run)
        monkeypatch.setattr(A, "_grad_weight_plans", plans)

    def clear(self):
        del self.w1d[:], self.wnd[:], self.plans[:]

    def __repr__(self):
        return f"fc_wgrad1d {self.w1d}, fc_wgrad_nd runs {len(self.wnd)}, forward-plan dW {self.plans}"


def _tensors(c, dtype):
    gen = torch.Generator(device=DEV).manual_seed(sum(c.size) + 7 * c.B + c.cin)
    x = torch.randn((c.B, c.cin) + tuple(c.size), generator=gen, device=DEV, dtype=dtype)
    w = torch.randn(c.wshape, generator=gen, device=DEV, dtype=dtype) / math.sqrt(math.prod(c.wshape[1:]))
    b = torch.randn(c.cout, generator=gen, device=DEV, dtype=dtype)
    return x, w, b, gen


def _step(c, x, w, b, gy=None):
    """(y, dX, dW, db, dY) of one training step through fft_conv / fft_conv_transpose."""
    from fft_conv_pytorch_amd.functional import fft_conv, fft_conv_transpose
    xs, ws, bs = (t.detach().clone().requires_grad_() for t in (x, w, b))
    y = (fft_conv_transpose if c.tr else fft_conv)(xs, ws, bs, **tr._kw(c))
    if gy is None:
        gy = torch.randn(y.shape, generator=torch.Generator(device=DEV).manual_seed(9), device=DEV).to(y.dtype)
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), xs.grad, ws.grad, bs.grad, gy


def _bound(what, got, want, tol):
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} elements not finite"
    err = tr._err(got, want)
    print(f"    {what}: {err:.2e}")
    assert err <= tol, f"{what}: element-wise error {err:.3e} > {tol}"
    return err


def _step_against_float64(c, x, w, b, tol, gy=None):
    y, dx, dw, db, gy = _step(c, x, w, b, gy)
    xr, wr, br = (t.double().clone().requires_grad_() for t in (x, w, b))
    ref = tr._reference(c, xr, wr, br)
    ref.backward(gy.double())
    return max(_bound(name, got, want, tol)
               for name, got, want in (("y", y, ref.detach()), ("dX", dx, xr.grad), ("dW", dw, wr.grad), ("db", db, br.grad)))


def _probe_inputs(c, x, gen, dy_axes, x_samples):
    """(what, x, dY) of the direct checks of one forward case: random rows, the dY probe, the x probe."""
    lout = bu.out_len(c)
    gy = torch.randn((c.B, c.cout) + lout, generator=gen, device=DEV, dtype=x.dtype)
    sets = [("random rows", x, gy),
            ("dY probe", x, bu.impulses(tuple(gy.shape), dy_axes, gen, x.dtype, DEV))]
    if x_samples is not None:
        sets.append(("x probe", bu.impulses(tuple(x.shape), [x_samples], gen, x.dtype, DEV), gy))
    return sets


def _args(c):
    return (c.cout, c.cin // c.g) + tuple(c.k), c.tup(c.s), c.tup(c.p), c.tup(c.d), c.g, c.mode


def _desc(c, dtype=torch.float32):
    from fft_conv_pytorch_amd import _native
    return _native.conv_desc(c.nd, c.B, c.cin, c.cout, c.g, tuple(c.size), tuple(c.k), c.tup(c.s), c.tup(c.p), c.tup(c.d),
                             _native.PAD_MODES[c.mode], CODE[dtype])


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _each(name, cases, fn):
    worst = 0.0
    for c in cases:
        print(f"  {name} / {c.ident()}")
        try:
            worst = max(worst, fn(c))
        except AssertionError as e:
            raise AssertionError(f"{name} / {c.ident()}: {e}") from None
    print(f"\nfamily {name}: {len(cases)} cases, worst element-wise error {worst:.2e}")
    RAN.add(name)


# ------------------------------------------------------------------------------------------------ 1. fc_wgrad1d
def _wgrad1d_case(family, c, monkeypatch):
    from fft_conv_pytorch_amd import _native, autograd as A
    _knobs(monkeypatch, family.env, c.env)
    geo = bu.wgrad_geometry(c, _cus())
    assert geo is not None, "the restated geometry refuses the case"
    slices = _native.wgrad1d_slices(_desc(c))
    assert slices == geo["slices"], f"the library plans {slices} slices, the restated geometry {geo}"
    assert family.pred(geo), f"case is outside its family: {geo}"
    assert c.expect is None or c.expect(geo), f"case not sized as intended: {geo}"
    x, w, b, gen = _tensors(c, torch.float32)
    spies = _Spies(monkeypatch)
    worst = _step_against_float64(c, x, w, b, ru.TOL32)
    want_call = [dict(slices=geo["slices"], db=not geo["diag"], diag=geo["diag"], dtype=0, stride=c.tup(c.s)[0])]
    assert spies.w1d == want_call and not spies.plans and not spies.wnd, f"the step launched {spies}, expected {want_call}"
    dy_axes, x_samples = bu.probe_sets(c, _cus())
    for what, x_, gy_ in _probe_inputs(c, x, gen, dy_axes, x_samples):
        spies.clear()
        got = A._grad_weight_native(x_, gy_, *_args(c), want_db=True)
        assert got is not None and spies.w1d == want_call, f"{what}: launched {spies}"
        dw, db = got
        assert (db is None) == geo["diag"], f"{what}: db {'missing' if db is None else 'present'}"
        if db is None:
            db = A._grad_bias(gy_)
        want_w, want_b = bu.reference_dw(c, x_, gy_)
        worst = max(worst, _bound(f"{what} dW", dw, want_w, ru.TOL32), _bound(f"{what} db", db, want_b, ru.TOL32))
    return worst


@pytest.mark.parametrize("family", bu.WGRAD1D_FAMILIES, ids=[f.name for f in bu.WGRAD1D_FAMILIES])
def test_wgrad1d_family(family, monkeypatch):
    assert family.cases, f"{family.name}: no cases"
    _each(family.name, family.cases, lambda c: _wgrad1d_case(family, c, monkeypatch))


@pytest.mark.parametrize("name,dtype,c", bu.HALF_CASES, ids=[f"{n}-{str(d).split('.')[1]}" for n, d, _ in bu.HALF_CASES])
def test_wgrad1d_half_bits_match_cast_path(name, dtype, c, monkeypatch):
    """A 16-bit training step on a stride-64 and on a strided depthwise layer: fc_wgrad1d reads the 16-bit tensors (a
    descriptor of their dtype, the slices of the float32 geometry) and every gradient has the bits of the
    FFTCONV_HALF_IO=0 path."""
    from fft_conv_pytorch_amd import _native, autograd as A
    _knobs(monkeypatch, c.env)
    geo = bu.wgrad_geometry(c, _cus())
    assert geo is not None and _native.wgrad1d_slices(_desc(c, dtype)) == geo["slices"], geo
    assert geo["diag"] == (name == "depthwise-strided")
    x, w, b = (t.to(dtype) for t in _tensors(c, torch.float32)[:3])
    spies = _Spies(monkeypatch)
    got = _step(c, x, w, b)
    assert spies.w1d == [dict(slices=geo["slices"], db=not geo["diag"], diag=geo["diag"], dtype=CODE[dtype],
                              stride=c.tup(c.s)[0])] and not spies.plans, f"the step launched {spies}"
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    _native.clear_plan_cache()
    A._BWD_PLANS.clear()
    want = _step(c, x, w, b, got[4])
    for part, g_, w_ in zip(("y", "dX", "dW", "db"), got, want):
        assert torch.isfinite(g_).all(), part
        gu.same_bits(g_, w_, f"{name} {dtype} {part} against the cast path")
    RAN.add(f"{name}-{str(dtype).split('.')[1]}")


# ------------------------------------------------------------------------------------------------ 2. refusals
def _refusal_case(c, chunked, sized, monkeypatch):
    from fft_conv_pytorch_amd import _native, autograd as A
    _knobs(monkeypatch, c.env)
    assert bu.wgrad_geometry(c, _cus()) is None and _native.wgrad1d_slices(_desc(c)) == 0, "fc_wgrad1d covers the shape"
    is_chunked, c_taps, nchunk = bu.chunk_plan(c)
    assert is_chunked == chunked, f"chunked {is_chunked}: {c_taps} taps x {nchunk} chunks"
    assert sized is None or sized(c_taps, nchunk, bu.out_len(c)[0]), \
        f"case not sized as intended: {nchunk} chunks of {c_taps} taps on {bu.out_len(c)[0]} outputs"
    x, w, b, gen = _tensors(c, torch.float32)
    spies = _Spies(monkeypatch)
    worst = _step_against_float64(c, x, w, b, ru.TOL32)
    assert not spies.w1d and not spies.wnd and spies.plans == [chunked], f"the step launched {spies}"
    dy_axes, x_samples = bu.probe_sets(c, _cus())
    for what, x_, gy_ in _probe_inputs(c, x, gen, dy_axes, x_samples):
        spies.clear()
        dw = A._grad_weight_plans(x_, gy_, *_args(c))
        assert spies.plans == [chunked] and not spies.w1d, f"{what}: launched {spies}"
        worst = max(worst, _bound(f"{what} dW", dw, bu.reference_dw(c, x_, gy_)[0], ru.TOL32))
    return worst


@pytest.mark.parametrize("name,c,chunked,sized", bu.REFUSALS, ids=[r[0] for r in bu.REFUSALS])
def test_refused_shapes_take_the_forward_plan_dw(name, c, chunked, sized, monkeypatch):
    """One step past a limit of fc_wgrad1d: the library reports no slices, no fc_wgrad1d launch happens, and the forward-plan
    dW -- through the chunked gather on long rows -- matches float64 on random rows and on probes at the chunk bounds."""
    _each(name, [c], lambda c_: _refusal_case(c_, chunked, sized, monkeypatch))


@pytest.mark.parametrize("name,c", bu.TRANSPOSED_DW, ids=[t[0] for t in bu.TRANSPOSED_DW])
def test_transposed_dw_with_zero_extended_signal(name, c, monkeypatch):
    """fft_conv_transpose with output_padding >= stride: conv(dY, W) is longer than x, and backward zero-extends x before
    the weight gradient -- fc_wgrad1d in float32, the chunked forward-plan dW in float64.  The probes are those of that
    convolution: impulses in x at the first outputs of its tiles (chunks), impulses in dY at the ends of their windows."""
    _knobs(monkeypatch, c.env)
    dtype = torch.float64 if c.f64 else torch.float32
    x, w, b, _ = _tensors(c, dtype)
    s, p, d, op, k, L = c.tup(c.s)[0], c.tup(c.p)[0], c.tup(c.d)[0], c.tup(c.op)[0], c.k[0], c.size[0]
    lo = (L - 1) * s - 2 * p + d * (k - 1) + op + 1
    assert op >= s and (lo + 2 * p - d * (k - 1) - 1) // s + 1 > L, "x is not extended"

    # the weight gradient is that of conv(dY, W): dY (lo samples) is its signal, the zero-extended x its output gradient
    fwd = ru.Case(c.B, c.cout, c.cin, (lo,), c.k, s=s, p=p, d=d, g=c.g, f64=c.f64)
    geo = bu.wgrad_geometry(fwd, _cus())
    assert (bu.chunk_plan(fwd)[2] if c.f64 else geo["ntiles"]) > 2, "a row of several tiles"
    outs, samples = bu.probe_sets(fwd, _cus())
    gen = torch.Generator(device=DEV).manual_seed(21)
    probes = [("random rows", x, None),
              ("dY probe", bu.impulses(tuple(x.shape), [[v for v in outs[0] if v < L]], gen, dtype, DEV), None),
              ("x probe", x, bu.impulses((c.B, c.cout, lo), [samples], gen, dtype, DEV))]

    def run(c_):
        spies = _Spies(monkeypatch)
        worst = 0.0
        for what, x_, gy_ in probes:
            spies.clear()
            print(f"   {what}")
            worst = max(worst, _step_against_float64(c_, x_, w, b, ru.TOL64 if c_.f64 else ru.TOL32, gy_))
            if c_.f64:
                assert spies.plans == [True] and not spies.w1d, f"{what}: the step launched {spies}"
            else:
                assert len(spies.w1d) == 1 and spies.w1d[0]["slices"] == geo["slices"] > 1 and not spies.plans, \
                    f"{what}: the step launched {spies}"
        return worst
    _each(name, [c], run)


# ------------------------------------------------------------------------------------------------ 3. dX
@pytest.mark.parametrize("route", ru.TRANSPOSED_ROUTES, ids=[r.name for r in ru.TRANSPOSED_ROUTES])
def test_transposed_route(route, monkeypatch):
    assert route.cases, f"{route.name}: no cases"
    assert all(c.tr and max(c.tup(c.s)) >= 2 for c in route.cases), "a strided transposed plan in every case"
    ops = {max(c.tup(c.op)) == 0 for c in route.cases}
    assert ops == {True, False}, "output_padding both 0 and s - 1"
    _each("T:" + route.name, route.cases, lambda c: tr._run_case(route, c, monkeypatch))


@pytest.mark.parametrize("name,env,c,own", ru.TRANSPOSED_REFUSED, ids=[r[0] for r in ru.TRANSPOSED_REFUSED])
def test_refusing_1d_routes_plan_the_general_kernel(name, env, c, own, monkeypatch):
    """The batch-sharing, wide, dense, depthwise and block-diagonal 1-D kernels take stride-1 plans only: under the route's
    knobs the stride-1 transposed plan of a shape lands on the route, the strided one on a general route."""
    from fft_conv_pytorch_amd import functional as fc
    _knobs(monkeypatch, env, c.env)
    x, w, b, _ = _tensors(c, torch.float32)
    kw = tr._kw(c)
    r = fc._plan_for(x, w, b, kw["stride"], kw["padding"], kw["dilation"], c.g, "constant", transposed=True,
                     output_padding=kw["output_padding"]).route
    assert ru.GENERAL_1D(r), f"{name}: a strided transposed plan on {r}"
    one = ru.Case(**{**c.__dict__, "s": 1, "op": 0})
    kw = tr._kw(one)
    r1 = fc._plan_for(x, w, b, kw["stride"], kw["padding"], kw["dilation"], c.g, "constant", transposed=True,
                      output_padding=kw["output_padding"]).route
    assert own(r1), f"{name}: the knobs do not reach the route at stride 1: {r1}"
    RAN.add("refused:" + name)


# ------------------------------------------------------------------------------------------------ 4. fc_wgrad_nd
def _wgrad_nd_case(c, env, pred, monkeypatch):
    from fft_conv_pytorch_amd import autograd as A
    _knobs(monkeypatch, env, c.env)
    x, w, b, gen = _tensors(c, torch.float32)
    layer = types.SimpleNamespace(weight=w, groups=c.g, stride=c.tup(c.s), padding=c.tup(c.p), dilation=c.tup(c.d))
    route = ts._wgrad_route(layer, x)
    assert pred is None or pred(route), f"case not sized as intended: {route}"
    assert c.note != "tails" or all(t != 0 for t in bu.stride_tails(c)), f"no tail on some axis: {bu.stride_tails(c)}"
    spies = _Spies(monkeypatch)
    worst = _step_against_float64(c, x, w, b, ru.TOL32)
    assert len(spies.wnd) == 1 and not spies.plans and not spies.w1d, f"the step launched {spies}"
    dy_axes, _ = bu.probe_sets(c, route=route)
    for what, x_, gy_ in _probe_inputs(c, x, gen, dy_axes, None):
        spies.clear()
        dw = A._grad_weight_nd_native(x_, gy_, *_args(c))
        assert dw is not None and len(spies.wnd) == 1 and not spies.plans, f"{what}: launched {spies}"
        worst = max(worst, _bound(f"{what} dW", dw, bu.reference_dw(c, x_, gy_)[0], ru.TOL32))
    return worst


@pytest.mark.parametrize("name,env,c,pred", bu.WGRAD_ND, ids=[n[0] for n in bu.WGRAD_ND])
def test_wgrad_nd_case(name, env, c, pred, monkeypatch):
    _each(name, [c], lambda c_: _wgrad_nd_case(c_, env, pred, monkeypatch))


# ------------------------------------------------------------------------------------------------ the cap
def test_every_family_and_transposed_route_ran():
    """Every family of backward_util and every entry of route_util.TRANSPOSED_ROUTES passed its cases in this run of the
    file: one that was skipped, deselected, empty or failed is missing here."""
    expected = {f.name for f in bu.WGRAD1D_FAMILIES} | {f"{n}-{str(d).split('.')[1]}" for n, d, _ in bu.HALF_CASES}
    expected |= {r[0] for r in bu.REFUSALS} | {t[0] for t in bu.TRANSPOSED_DW} | {n[0] for n in bu.WGRAD_ND}
    expected |= {"T:" + r.name for r in ru.TRANSPOSED_ROUTES} | {"refused:" + r[0] for r in ru.TRANSPOSED_REFUSED}
    assert len(expected) == (len(bu.WGRAD1D_FAMILIES) + len(bu.HALF_CASES) + len(bu.REFUSALS) + len(bu.TRANSPOSED_DW) +
                             len(bu.WGRAD_ND) + len(ru.TRANSPOSED_ROUTES) + len(ru.TRANSPOSED_REFUSED)), "a name is used twice"
    missing, extra = sorted(expected - RAN), sorted(RAN - expected)
    assert not missing and not extra, f"not exercised: {missing}; unexpected: {extra}"
