"""What the kernels do to memory they should neither read nor write (tests/guard_util.py), over every route.

Each case runs four times: with every ``torch.empty`` buffer of the library (workspace, spectrum, outputs, the partial
sums of the weight gradients) and the surroundings of every input filled with 0x00, with 0xFF (NaN), with 0x7F (huge), and
with 0x00 again.  Every tensor sits between two 64 KiB guards.  Asserted:

* no guard of a library buffer or of an input changed, and no input changed;
* the 0xFF, 0x7F and repeated runs have the bits of the first one: a slot read before this call wrote it, or a race,
  shows as a difference (0 x NaN in a phantom channel is a NaN);
* the first run is finite and within route_util.TOL32 / TOL64 of the float64 reference (max|got - want| / max|want|),
  which anchors the bit-equal runs to the truth; 16-bit results have the bits of the cast path instead.

Cases: (a) every route of route_util.ROUTES and the float64 long transform, through the plan and the public op;
(b) one training step per backward kernel; (c) ``fft_long_conv`` over every column geometry, 16-bit, complex64 and
training; (d) inputs that start at an address that is only element-aligned.  The last test checks that all of them ran."""
import functools
import math

import pytest
import torch

from fft_conv_pytorch_amd import _native, autograd, fft_long_conv
from fft_conv_pytorch_amd import functional as fc
from fft_conv_pytorch_amd.functional import fft_conv, fft_conv_transpose
from tests import guard_util as gu
from tests import route_util as ru
from tests import test_gpu_f64_long as t64
from tests import test_gpu_half_train as th
from tests import test_gpu_long_complex as tcx
from tests import test_gpu_long_conv as tl
from tests import test_gpu_long_general as tg
from tests import test_gpu_routes as tr
from tests.test_host_long_general import MODES, _expect

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOBS = tuple(sorted(set(tr.KNOBS) | set(th.KNOBS) | set(tg.KNOBS) | set(t64.KNOBS)))
RUNS = (0x00, 0xFF, 0x7F, 0x00)
C = ru.Case
RAN = set()                        # route and family names whose case passed (the last test compares it)


def _clear():
    _native.clear_plan_cache()
    fc._REFUSED_HALF.clear()
    autograd._BWD_PLANS.clear()


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    """Knobs are read at plan creation and are not part of a cache key: none set on entry, no plan outlives the test."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    _clear()
    yield
    _clear()


def _set(monkeypatch, *envs):
    for env in envs:
        for k, v in env.items():
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, v)
    _clear()


def _runs(op, inputs, what, patterns=RUNS, offset=0, same_as=None):
    """``op(*inputs) -> tensor or tuple`` once per pattern, inputs embedded in guarded blocks of that pattern (``offset``
    elements past the aligned start), every torch.empty of the call guarded and filled with it.  Guards and inputs intact
    after every run; every run bit-equal to the first (to ``same_as`` if given).  Returns the first run's outputs."""
    first = same_as
    for n, pattern in enumerate(patterns):
        pairs = [(None, None) if t is None else gu.guarded(t, pattern, offset) for t in inputs]
        with gu.guarded_empty(pattern) as ge:
            out = op(*(p[0] for p in pairs))
        out = tuple(out) if isinstance(out, (tuple, list)) else (out,)
        tag = f"{what}, run {n} ({pattern:#04x}{', odd start' if offset else ''})"
        assert ge.served, f"{tag}: no buffer came from the guarded allocator"
        assert ge.violations() == [], f"{tag}: guard bytes of a library buffer changed: {ge.violations()}"
        for i, (_, check) in enumerate(pairs):
            if check is not None:
                found = check()
                assert found == [], f"{tag}: input {i} or its guards changed: {found}"
        if first is None:
            first = out
        else:
            assert len(out) == len(first)
            for j, (a, b) in enumerate(zip(out, first)):
                gu.same_bits(a, b, f"{tag}, output {j} against the first run")
    return first


def _err(got, want):
    got, want = got.detach(), want.detach()
    if got.is_complex():
        return ((got.cpu().to(torch.complex128) - want.cpu()).abs().max() / want.abs().max()).item()
    return (got.double().cpu() - want.double().cpu()).abs().max().item() / max(want.double().abs().max().item(), 1e-300)


def _anchor(got, want, tol, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    finite = torch.isfinite(torch.view_as_real(got) if got.is_complex() else got)
    assert finite.all(), f"{what}: {int((~finite).sum())} samples not written / not finite"
    err = _err(got, want)
    assert err <= tol, f"{what}: element-wise error {err:.3e} > {tol}"
    return err


# ------------------------------------------------------------------------------------------------ (a) every route
def _out_numel(c):
    n = c.B * c.cout
    for S, k, s, p, d, op in zip(c.size, c.k, c.tup(c.s), c.tup(c.p), c.tup(c.d), c.tup(c.op)):
        n *= (S - 1) * s - 2 * p + d * (k - 1) + op + 1 if c.tr else (S + 2 * p - d * (k - 1) - 1) // s + 1
    return n


def _pick(route):
    """The first case of the route with a full float64 reference, else its smallest one (sampled dot products)."""
    for c in route.cases:
        if _out_numel(c) <= ru.FULL_REF_MAX:
            return c
    return min(route.cases, key=_out_numel)


def _case_tensors(c):
    dtype = torch.float64 if c.f64 else torch.float32
    gen = torch.Generator(device=DEV).manual_seed(sum(c.size) + 7 * c.B + c.cin)
    x = torch.randn((c.B, c.cin) + tuple(c.size), generator=gen, device=DEV, dtype=dtype)
    w = torch.randn(c.wshape, generator=gen, device=DEV, dtype=dtype) / math.sqrt(math.prod(c.wshape[1:]))
    b = torch.randn(c.cout, generator=gen, device=DEV, dtype=dtype)
    return x, w, b


def _plan_of(c, x, w, b):
    kw = tr._kw(c)
    return fc._plan_for(x, w, b, kw["stride"], kw["padding"], kw["dilation"], c.g, "constant" if c.tr else c.mode,
                        transposed=c.tr, output_padding=kw.get("output_padding", 0))


def _plan_op(plan):
    """What test_gpu_routes._plan_forward does, with spectrum, workspaces and output from the (guarded) torch.empty."""
    def op(x, w, b):
        spec = fc.transform_kernel(plan, w)
        out = torch.empty((x.shape[0], plan.key[3]) + plan.out_spatial, dtype=plan.dtype, device=x.device)
        ws = fc.new_workspace(plan, x.device)
        plan.forward(x.data_ptr(), spec.buf.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr() if ws is not None else None,
                     torch.cuda.current_stream(x.device).cuda_stream)
        return out
    return op


def _public_op(c):
    op = fft_conv_transpose if c.tr else fft_conv
    kw = tr._kw(c)
    return lambda x, w, b: op(x, w, b, **kw)


class _Reference:
    """The float64 reference of one case, computed once: the full output, or sampled dot products for a large one."""

    def __init__(self, c, plan, x, w, b):
        if _out_numel(c) <= ru.FULL_REF_MAX:
            self.idx, self.want = None, tr._reference(c, x.double(), w.double(), b.double())
        else:
            shape = (c.B, c.cout) + plan.out_spatial
            self.idx = tr._sample_idx(c, shape, tr._seams(c, plan.route, plan.layout[3]))
            self.want = tr._sampled(c, x, w, b, self.idx)

    def check(self, got, tol, what):
        finite = torch.isfinite(got)
        assert finite.all(), f"{what}: {int((~finite).sum())} samples not written / not finite"
        if self.idx is not None:
            got = got[tuple(self.idx.t().to(got.device))]
        return _anchor(got, self.want, tol, what)


ODD_START_ROUTES = ("1d-general-single", "1d-pers-1024-nb2", "1d-dense-1024")


def _forward_case(name, c, pred, odd=False, expect=None):
    x, w, b = _case_tensors(c)
    plan = _plan_of(c, x, w, b)
    r = plan.route
    assert pred(r), f"{name} / {c.ident()}: the plan is on another route: {r}"
    for e in (c.expect, expect):
        assert e is None or e(r), f"{name} / {c.ident()}: case not sized as intended: {r}"
    tol = ru.TOL64 if c.f64 else ru.TOL32
    what = f"{name} / {c.ident()}"
    ref = _Reference(c, plan, x, w, b)
    (y0,) = _runs(_plan_op(plan), (x, w, b), what + " plan")
    worst = ref.check(y0, tol, what + " plan")
    if c.public:
        (p0,) = _runs(_public_op(c), (x, w, b), what + " public op")
        worst = max(worst, ref.check(p0, tol, what + " public op"))
    if odd:
        _runs(_plan_op(plan), (x, w, b), what + " plan", patterns=RUNS[:2], offset=1, same_as=(y0,))
    print(f"\n{what}: four bit-equal runs, guards intact, error {worst:.2e} {r}")


@pytest.mark.parametrize("route", ru.ROUTES, ids=[r.name for r in ru.ROUTES])
def test_route(route, monkeypatch):
    assert route.cases, f"{route.name}: no cases"
    c = _pick(route)
    _set(monkeypatch, route.env, c.env)
    odd = route.name in ODD_START_ROUTES
    _forward_case(route.name, c, route.pred, odd)
    RAN.add(route.name)
    if odd:
        RAN.add("odd-start:" + route.name)


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16), ids=["f16", "bf16"])
def test_sixteen_bit_persistent_route(dtype, monkeypatch):
    """The batch-sharing kernel reading 16-bit x: four samples per load from an aligned row, its per-sample fallback from a
    row that starts two bytes past an aligned address.  The bits of the cast path either way."""
    route = next(r for r in ru.ROUTES if r.name == "1d-pers-1024-nb2")
    c = route.cases[0]
    _set(monkeypatch, route.env, c.env)
    x, w, b = (t.to(dtype) for t in _case_tensors(c))
    r = _plan_of(c, x, w, b).route
    assert route.pred(r), f"the {dtype} plan is on another route: {r}"
    what = f"{route.name} {dtype}"
    (y0,) = _runs(_public_op(c), (x, w, b), what)
    _runs(_public_op(c), (x, w, b), what, patterns=RUNS[:2], offset=1, same_as=(y0,))
    assert torch.isfinite(y0).all()
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    gu.same_bits(y0, _public_op(c)(x, w, b), f"{what} against the cast path")
    RAN.add(f"odd-start:half-{route.name}-{str(dtype).split('.')[1]}")


F64_LONG = [
    # the planner's own factorisation, one transform per row (test_gpu_f64_long.OWN); runs at an odd start too
    ("f64-fft-long", {}, t64.OWN[0], lambda r: r["ntiles"] == 1, True),
    # overlap-save tiles of 64 x 64 points (test_gpu_f64_long.TILED)
    ("f64-fft-long-tiles", {"FFTCONV_F64_LONG_N": "64x64", "FFTCONV_F64_LONG": "2"},
     t64.TILED[0], lambda r: (r["N1"], r["N2"]) == (64, 64) and r["ntiles"] >= 3, False),
]


@pytest.mark.parametrize("name,env,c,expect,odd", F64_LONG, ids=[f[0] for f in F64_LONG])
def test_float64_long_route(name, env, c, expect, odd, monkeypatch):
    _set(monkeypatch, env)
    c = C(**{**c.__dict__, "public": True})
    _forward_case(name, c, lambda r: r["kind"] == "f64_fft_long", odd, expect)
    RAN.add(name)
    if odd:
        RAN.add("odd-start:" + name)


# ------------------------------------------------------------------------------------------------ (b) backward
class _Spies:
    """What a training step launched: fc_wgrad1d (slices, db rider, stride), fc_wgrad_nd runs, the forward-plan dW, and
    (ndim, transposed, dtype) of every plan that ran a forward launch."""

    def __init__(self, monkeypatch):
        self.w1d, self.wnd, self.plans, self.launches = [], [], [], []
        real_db, real_run, real_plans, real_fwd = (_native.wgrad1d_db, _native.WgradPlan.run, autograd._grad_weight_plans,
                                                   fc._forward_native)

        def wgrad1d_db(desc, x_ptr, dy_ptr, part_ptr, db_ptr, row, slices, stream):
            self.w1d.append(dict(slices=slices, db=db_ptr is not None, stride=int(desc.stride[0]), dtype=int(desc.dtype),
                                 kd=(int(desc.kernel[0]) - 1) * int(desc.dilation[0]) + 1))
            return real_db(desc, x_ptr, dy_ptr, part_ptr, db_ptr, row, slices, stream)

        def run(plan, *a):
            self.wnd.append(plan)
            return real_run(plan, *a)

        def plans(x, grad, wshape, stride, *a):
            kext = (grad.shape[2] - 1) * stride[0] + 1
            kd0 = (wshape[2] - 1) * a[1][0] + 1
            self.plans.append(x.ndim == 3 and kext > max(autograd._DW_TILE - kd0 + 1, autograd._DW_TILE // 4))
            return real_plans(x, grad, wshape, stride, *a)

        def forward_native(signal, spectrum, bias):
            key = spectrum.plan.key
            self.launches.append((key[0], bool(key[13]), spectrum.plan.dtype))
            return real_fwd(signal, spectrum, bias)
        monkeypatch.setattr(_native, "wgrad1d_db", wgrad1d_db)
        monkeypatch.setattr(_native.WgradPlan, "run", run)
        monkeypatch.setattr(autograd, "_grad_weight_plans", plans)
        monkeypatch.setattr(fc, "_forward_native", forward_native)


def _train_op(fn):
    def op(x, w, b, gy):
        xs, ws, bs = (t.detach().requires_grad_() for t in (x, w, b))      # (leaves on the guarded views: no copies)
        y = fn(xs, ws, bs)
        y.backward(gy)
        return y.detach(), xs.grad, ws.grad, bs.grad
    return op


F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
BACKWARD = [
    # (families, knobs, case, dtype, what the spies must have seen)
    # route_util "1d-block-diagonal-gs2": 104 (batch item, tile) work items in more than one slice, db riding the launch
    (("fc_wgrad1d-slices-db", "dx-plan-1d"), {}, C(4, 16, 16, (20000,), (257,), g=8), F32,
     lambda s: s.w1d and all(v["slices"] > 1 and v["db"] for v in s.w1d) and (1, True, F32) in s.launches),
    # the 1-D cases of test_gpu_half_train.CASES: stride 3; 1000 taps (past 768: two segments of taps)
    (("fc_wgrad1d-strided",), {}, C(2, 8, 6, (3001,), (17,), s=3, p=5), F32,
     lambda s: s.w1d and all(v["stride"] == 3 for v in s.w1d)),
    (("fc_wgrad1d-tap-segments",), {}, C(1, 8, 16, (5000,), (1000,), p=5), F32,
     lambda s: s.w1d and all(v["kd"] > 768 for v in s.w1d)),
    # its 2-D / 3-D cases
    (("fc_wgrad_nd-2d", "dx-plan-2d"), {}, C(2, 3, 4, (40, 60), (9, 11), p=2), F32,
     lambda s: len(s.wnd) == len(RUNS) and (2, True, F32) in s.launches),
    (("fc_wgrad_nd-3d", "dx-plan-3d"), {}, C(2, 3, 4, (17, 19, 23), (3, 5, 3), p=1), F32,
     lambda s: len(s.wnd) == len(RUNS) and (3, True, F32) in s.launches),
    # test_gpu_half_train.test_nd_weight_gradient_segments_of_taps: segments of 8 taps in the separable passes
    (("fc_wgrad_nd-segments",), {"FFTCONV_NDSEG": "8", "FFTCONV_PLANES": "0"}, C(2, 4, 6, (30, 40), (3, 5), p=1), F32,
     lambda s: len(s.wnd) == len(RUNS)),
    # route_util "f64-1d-fft": dY (3001 samples) is longer than one tile of the role-swapped plan takes: chunks
    (("f64-chunked-dw",), {}, C(3, 4, 6, (3001,), (65,), p=32, mode="reflect", f64=True), F64,
     lambda s: s.plans == [True] * len(RUNS) and not s.w1d),
    # 16-bit descriptors (test_gpu_half_train.CASES "1d-dense-db" and "2d-default")
    (("half-wgrad1d", "half-dx-plan-1d"), {}, C(2, 8, 8, (3000,), (33,), p=16), BF16,
     lambda s: s.w1d and all(v["dtype"] == 3 for v in s.w1d) and (1, True, BF16) in s.launches),
    (("half-wgrad_nd", "half-dx-plan-nd"), {}, C(2, 3, 4, (40, 60), (9, 11), p=2), F16,
     lambda s: len(s.wnd) == len(RUNS) and (2, True, F16) in s.launches),
]
BACKWARD_FAMILIES = [f for case in BACKWARD for f in case[0]]


@pytest.mark.parametrize("families,env,c,dtype,seen", BACKWARD, ids=[b[0][0] for b in BACKWARD])
def test_training_step(families, env, c, dtype, seen, monkeypatch):
    _set(monkeypatch, env)
    x, w, b = (t.to(dtype) for t in _case_tensors(c))
    fn = _public_op(c)
    with torch.no_grad():
        shape = fn(x, w, b).shape
    gy = torch.randn(shape, generator=torch.Generator(device=DEV).manual_seed(9), device=DEV).to(dtype)
    spies = _Spies(monkeypatch)
    what = f"{families[0]} / {c.ident()} {dtype}"
    got = _runs(_train_op(fn), (x, w, b, gy), what)
    assert seen(spies), f"{what}: the step did not take the kernels it is here for: w1d {spies.w1d}, wnd {len(spies.wnd)}, " \
                        f"forward-plan dW {spies.plans}, launches {spies.launches}"
    names = ("y", "dX", "dW", "db")
    if dtype in (F16, BF16):
        monkeypatch.setenv("FFTCONV_HALF_IO", "0")
        want = _train_op(fn)(x, w, b, gy)
        torch.cuda.synchronize()
        for part, g_, w_ in zip(names, got, want):
            assert torch.isfinite(g_).all(), part
            gu.same_bits(g_, w_, f"{what} {part} against the cast path")
    else:
        xr, wr, br = (t.double().clone().requires_grad_() for t in (x, w, b))
        ref = tr._reference(c, xr, wr, br)
        ref.backward(gy.double())
        tol = ru.TOL64 if c.f64 else ru.TOL32
        for part, g_, w_ in zip(names, got, (ref, xr.grad, wr.grad, br.grad)):
            _anchor(g_, w_, tol, f"{what} {part}")
    RAN.update(families)


# ------------------------------------------------------------------------------------------------ (c) fft_long_conv
@pytest.fixture
def long_ran(monkeypatch):
    """(N1, N2, x dtype code, y dtype code) of every long plan whose forward ran."""
    seen = []
    real = _native.LongPlan.forward

    def forward(plan, x_ptr, spectrum_ptr, bias_ptr, y_ptr, workspace_ptr, stream, x_dtype=0, y_dtype=0):
        seen.append((plan.info["N1"], plan.info["N2"], x_dtype, y_dtype))
        return real(plan, x_ptr, spectrum_ptr, bias_ptr, y_ptr, workspace_ptr, stream, x_dtype, y_dtype)
    monkeypatch.setattr(_native.LongPlan, "forward", forward)
    return seen


def _long_op(**kw):
    return lambda x, w, b: fft_long_conv(x, w, b, **kw)


def _long_kw(padding, g, causal, s=1, d=1, mode="constant"):
    return dict(padding=padding, groups=g, causal=causal, stride=s, dilation=d, padding_mode=mode)


MAPPED = (3, 4, 4, 2, 5000, 1200, 37, False, 2, 3, "reflect")       # test_gpu_long_general's case of every geometry


@functools.lru_cache(maxsize=None)
def _mapped_reference():
    """Tensors and float64 oracle of MAPPED, shared by the geometries (never written)."""
    B, cin, cout, g, L, K, padding, causal, s, d, mode = MAPPED
    x, w, b = tg._tensors(B, cin, cout, g, L, K)
    return x, w, b, tg._want(x, w, b, padding, g, causal, s, d, mode)


def _plain_case(N1, N2):
    """test_gpu_long_conv's shape of a forced factorisation."""
    causal = (N1 + N2) % 3 != 0
    return 3, 4, 6, 2, (2500 if N1 * N2 == 4096 else 3000), 1500, (0 if causal else 700), causal


@pytest.mark.parametrize("N1,N2", tg.COLUMN_GEOMETRIES)
def test_long_column_geometry(N1, N2, monkeypatch, long_ran):
    _set(monkeypatch, {"FFTCONV_LONG_N": f"{N1}x{N2}"})
    g, (padding, causal, s, d, mode) = MAPPED[3], MAPPED[6:]
    x, w, b, want = _mapped_reference()
    what = f"long mapped {N1}x{N2}"
    (y0,) = _runs(_long_op(**_long_kw(padding, g, causal, s, d, mode)), (x, w, b), what)
    assert long_ran and all(r[:2] == (N1, N2) for r in long_ran), long_ran
    _anchor(y0, want, ru.TOL32, what)
    RAN.add(f"long-mapped-{N1}x{N2}")

    del long_ran[:]
    B, cin, cout, g, L, K, padding, causal = _plain_case(N1, N2)
    x, w, b = tl._tensors(B, cin, cout, g, L, K, True)
    what = f"long plain {N1}x{N2}"
    odd = (N1, N2) == (128, 64)
    (y0,) = _runs(_long_op(**_long_kw(padding, g, causal)), (x, w, b), what)
    assert long_ran and all(r[:2] == (N1, N2) for r in long_ran), long_ran
    _anchor(y0, tl._want(x, w, b, padding, g, causal), ru.TOL32, what)
    RAN.add(f"long-plain-{N1}x{N2}")
    if odd:
        _runs(_long_op(**_long_kw(padding, g, causal)), (x, w, b), what, patterns=RUNS[:2], offset=1, same_as=(y0,))
        RAN.add("odd-start:long-f32")


def test_long_64_x_64_at_the_primitive(monkeypatch):
    """Rows of at most 4096 points go to fft_conv in the functional: the primitive is called, mapped and plain, as
    test_gpu_long_general.py and test_gpu_long_conv.py do for this factorisation."""
    _set(monkeypatch, {"FFTCONV_LONG_N": "64x64"})

    def primitive(cout, g, K, pl, pr, flip, keep, **ext):
        def op(x, w, b):
            plan = fc._long_plan(x, cout, g, K, pl, pr, flip, keep, True, **ext)
            assert (plan.info["N1"], plan.info["N2"]) == (64, 64)
            spectrum = fc.transform_kernel(plan, w)
            out = torch.empty((x.shape[0], cout, plan.out_len), dtype=torch.float32, device=x.device)
            ws = fc.new_workspace(plan, x.device)
            plan.forward(x.data_ptr(), spectrum.buf.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
            return out
        return op

    B, cin, cout, g, L, K, s, d, mode = 3, 4, 4, 2, 3900, 900, 2, 3, "reflect"
    x, w, b = tg._tensors(B, cin, cout, g, L, K)
    (y0,) = _runs(primitive(cout, g, K, 37, 37, False, 0, pad_mode=MODES[mode], tap_dil=d, out_step=s), (x, w, b),
                  "long mapped 64x64")
    _anchor(y0, tg._want(x, w, b, 37, g, False, s, d, mode), ru.TOL32, "long mapped 64x64")
    RAN.add("long-mapped-64x64")

    B, cin, cout, g, L, K, padding, causal = _plain_case(64, 64)
    x, w, b = tl._tensors(B, cin, cout, g, L, K, True)
    pl, pr = (K - 1, 0) if causal else (padding, padding)
    (y0,) = _runs(primitive(cout, g, K, pl, pr, causal, L if causal else 0), (x, w, b), "long plain 64x64")
    _anchor(y0, tl._want(x, w, b, padding, g, causal), ru.TOL32, "long plain 64x64")
    RAN.add("long-plain-64x64")


HALF_CASE = (3, 4, 4, 2, 5001, 1201)       # test_gpu_long_general's 16-bit case
HALF_KW = dict(padding=37, groups=2, stride=2, dilation=3, padding_mode="reflect")


def _half_tensors(dtype):
    B, cin, cout, g, L, K = HALF_CASE
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(B, cin, L, generator=gen).to(DEV).to(dtype)
    w = (torch.randn(cout, cin // g, K, generator=gen) / math.sqrt(cin // g * K)).to(DEV).to(dtype)
    b = torch.randn(cout, generator=gen).to(DEV).to(dtype)
    return x, w, b, gen


@pytest.mark.parametrize("dtype", (F16, BF16), ids=["f16", "bf16"])
def test_long_sixteen_bit_forward(dtype, monkeypatch, long_ran):
    x, w, b, _ = _half_tensors(dtype)
    code = fc._DTYPE_CODES[dtype]
    what = f"long {dtype}"
    (y0,) = _runs(_long_op(**HALF_KW), (x, w, b), what)
    assert long_ran and all(r[2:] == (code, code) for r in long_ran), long_ran
    assert torch.isfinite(y0).all()
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    gu.same_bits(y0, fft_long_conv(x, w, b, **HALF_KW), f"{what} against the cast path")
    monkeypatch.delenv("FFTCONV_HALF_IO")
    RAN.add(f"long-{str(dtype).split('.')[1]}")
    # x, w and b two bytes past an aligned address: the 16-bit loads that cannot go four at a time
    del long_ran[:]
    _runs(_long_op(**HALF_KW), (x, w, b), what, patterns=RUNS[:2], offset=1, same_as=(y0,))
    assert long_ran and all(r[2:] == (code, code) for r in long_ran), long_ran
    RAN.add(f"odd-start:long-{str(dtype).split('.')[1]}")


CX_PLAIN = (3, 6, 4, 2, 5001, 1201, 100, False, 1, 1, "constant")        # test_gpu_long_complex.LAYOUTS[0]
CX_MAPPED = (3, 4, 6, 2, 5000, 1200, 37, False, 2, 3, "circular")        # ... MAPPED: all three maps at once


@pytest.mark.parametrize("name,case", [("long-complex64-plain", CX_PLAIN), ("long-complex64-mapped", CX_MAPPED)])
def test_long_complex_forward(name, case, long_ran):
    B, cin, cout, g, L, K, padding, causal, s, d, mode = case
    x, w, b = (t.to(DEV) for t in tcx._tensors(B, cin, cout, g, L, K))
    (y0,) = _runs(_long_op(**_long_kw(padding, g, causal, s, d, mode)), (x, w, b), name)
    assert long_ran and all(r[2:] == (4, 4) for r in long_ran), long_ran
    _anchor(y0, tcx._want(B, cin, cout, g, L, K, padding, causal, s, d, mode, True), ru.TOL32, name)
    RAN.add(name)


def test_long_training_step_float32(long_ran):
    B, cin, cout, g, L, K, padding, causal, s, d, mode = tg.GRADS[0]
    x, w, b = tg._tensors(B, cin, cout, g, L, K)
    x64, w64, b64 = (t.double().cpu().requires_grad_() for t in (x, w, b))
    want = _expect(x64, w64, b64, padding, g, causal, s, d, mode)
    gy = torch.randn(want.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    want.backward(gy)
    got = _runs(_train_op(_long_op(**_long_kw(padding, g, causal, s, d, mode))), (x, w, b, gy.float().to(DEV)),
                "long training step float32")
    assert len(long_ran) == 3 * len(RUNS), long_ran            # forward, dX, dW: one run of the primitive each
    for part, g_, w_ in zip(("y", "dX", "dW", "db"), got, (want, x64.grad, w64.grad, b64.grad)):
        _anchor(g_, w_, ru.TOL32, f"long training step float32 {part}")
    RAN.add("long-train-float32")


def test_long_training_step_bfloat16(monkeypatch, long_ran):
    x, w, b, gen = _half_tensors(BF16)
    with torch.no_grad():
        shape = fft_long_conv(x, w, b, **HALF_KW).shape
    gy = torch.randn(shape, generator=gen).to(DEV).to(BF16)
    del long_ran[:]
    got = _runs(_train_op(_long_op(**HALF_KW)), (x, w, b, gy), "long training step bfloat16")
    # forward 16 -> 16; dX of the padded row in float32 (folded, then rounded once); dW float32 from 16-bit operands
    assert [r[2:] for r in long_ran] == [(3, 3), (3, 0), (3, 0)] * len(RUNS), long_ran
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    want = _train_op(_long_op(**HALF_KW))(x, w, b, gy)
    torch.cuda.synchronize()
    for part, g_, w_ in zip(("y", "dX", "dW", "db"), got, want):
        assert torch.isfinite(g_).all(), part
        gu.same_bits(g_, w_, f"long training step bfloat16 {part} against the cast path")
    RAN.add("long-train-bfloat16")


def test_long_training_step_complex64(long_ran):
    B, cin, cout, g, L, K, padding, causal, s, d, mode, _ = tcx.GRAD_CASES[2]
    x, w, b = tcx._tensors(B, cin, cout, g, L, K)
    x64, w64, b64 = (t.to(torch.complex128).requires_grad_() for t in (x, w, b))
    want = tcx._conv_ref(x64, w64, b64, padding, g, causal, s, d, mode)
    gy = torch.view_as_complex(torch.randn(tuple(want.shape) + (2,), generator=torch.Generator().manual_seed(1)))
    want.backward(gy.to(torch.complex128))
    got = _runs(_train_op(_long_op(**_long_kw(padding, g, causal, s, d, mode))), (x.to(DEV), w.to(DEV), b.to(DEV), gy.to(DEV)),
                "long training step complex64")
    assert [r[2:] for r in long_ran] == [(4, 4)] * 3 * len(RUNS), long_ran
    for part, g_, w_ in zip(("y", "dX", "dW", "db"), got, (want, x64.grad, w64.grad, b64.grad)):
        _anchor(g_, w_, ru.TOL32, f"long training step complex64 {part}")
    RAN.add("long-train-complex64")


# ------------------------------------------------------------------------------------------------ the cap
def test_every_route_and_family_ran():
    """Every route of route_util.ROUTES and every family of (a) to (d) passed its case in this run of the file: one that
    was skipped, deselected or failed is missing here."""
    geometries = [f"{n1}x{n2}" for n1, n2 in tg.COLUMN_GEOMETRIES] + ["64x64"]
    expected = {r.name for r in ru.ROUTES} | {f[0] for f in F64_LONG} | set(BACKWARD_FAMILIES)
    expected |= {f"long-mapped-{n}" for n in geometries} | {f"long-plain-{n}" for n in geometries}
    expected |= {"long-float16", "long-bfloat16", "long-complex64-plain", "long-complex64-mapped",
                 "long-train-float32", "long-train-bfloat16", "long-train-complex64"}
    expected |= {"odd-start:" + n for n in ODD_START_ROUTES} | {"odd-start:f64-fft-long", "odd-start:long-f32",
                                                                  "odd-start:long-float16", "odd-start:long-bfloat16",
                                                                  "odd-start:half-1d-pers-1024-nb2-float16",
                                                                  "odd-start:half-1d-pers-1024-nb2-bfloat16"}
    assert len(BACKWARD_FAMILIES) == len(set(BACKWARD_FAMILIES))
    missing, extra = sorted(expected - RAN), sorted(RAN - expected)
    assert not missing and not extra, f"not exercised: {missing}; unexpected: {extra}"
