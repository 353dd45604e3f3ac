"""``fft_long_conv_transpose`` / ``FFTLongConvTranspose1d`` on the GPU: the phases builds of the column kernels
(csrc/long1d.hpp) and the zero-spread route, on the table of tests/test_host_long_transpose.py.

Inputs are the integers of tests/accuracy_util.py, so torch's float64 ``conv_transpose1d`` of them is exact; the bound is
``accuracy_util.check`` with its standard margins against the model project's formulation in float32 on the zero-spread
row.  Every forward case runs between guard bands into NaN-filled and zero-filled buffers; 16-bit results and gradients
are compared bit for bit with the cast path.  A truth and a baseline are computed once per (case, class) and shared."""
import pytest
import torch

from fft_conv_pytorch_amd import FFTLongConvTranspose1d, _native, autograd, fft_long_conv_transpose
from fft_conv_pytorch_amd import functional as F_
from fft_conv_pytorch_amd.functional import fft_conv_transpose
from tests import accuracy_util as au
from tests import guard_util as gu
from tests.route_util import TOL32
from tests.test_host_long_transpose import CASES, PHASES_CASES, out_len, route_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, C64 = torch.float32, torch.complex64
KNOBS = ("FFTCONV_LONG_POLY", "FFTCONV_LONG_NLC", "FFTCONV_LONG_N", "FFTCONV_LONG_WS_MB", "FFTCONV_HALF_IO", "FFTCONV_TILE")
DIRECT_MAX_TAPS = 1100        # longer filters take the float64 FFT truth (accuracy_util.truth_by_fft)
PHASES_POINTS = {1: 4096, 2: 4096, 3: 4096, 4: 8192, 5: 4096, 6: 4096}


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
def ran(monkeypatch):
    """The long plans whose forward ran: (plan, x layout, y layout) per launch."""
    seen = []
    real, real_lay = _native.LongPlan.forward, _native.LongPlan.forward_lay

    def forward(plan, *args):
        seen.append((plan, _native.LONG_NCL, _native.LONG_NCL))
        return real(plan, *args)

    def forward_lay(plan, *args):
        seen.append((plan, args[-2], args[-1]))
        return real_lay(plan, *args)
    monkeypatch.setattr(_native.LongPlan, "forward", forward)
    monkeypatch.setattr(_native.LongPlan, "forward_lay", forward_lay)
    return seen


def _is_phases(plan):
    return isinstance(plan, _native.LongPhasesPlan)


def _points(plan):
    return plan.info["N1"] * plan.info["N2"]


_SHARED = {}


def _data(i, cls, complex_=False):
    """(x, w, b, exact y, float32 baseline y) of case i, computed once and left unchanged."""
    key = (i, cls, complex_)
    if key not in _SHARED:
        c = CASES[i]
        au.assert_exact(c, cls, complex_)
        x, w, b = au.inputs(c, cls, DEV, complex_=complex_)
        want = au.truth(c, x, w, b) if c.k[0] <= DIRECT_MAX_TAPS else au.truth_by_fft(c, x, w, b)
        assert tuple(want.shape) == (c.B, c.cout, out_len(c))
        _SHARED[key] = (x, w, b, want, au.baseline(c, x, w, b))
    return _SHARED[key]


def _call(c, x, w, b, **kw):
    return fft_long_conv_transpose(x, w, b, c.s, c.p, c.op, c.d, c.g, **kw)


def _guarded_call(c, x, w, b, **kw):
    """The call into NaN-filled and into zero-filled buffers, the inputs between guard bands of their own: no byte outside
    a tensor changes, the inputs keep their bits, the two results agree bit for bit and hold no NaN."""
    outs = []
    for pattern in (0xFF, 0x00):
        held = [gu.guarded(t, pattern, offset=1) for t in (x, w, b)]
        with gu.guarded_empty(pattern) as ge:
            y = _call(c, *(h[0] for h in held), **kw)
        assert ge.violations() == [], f"pattern {pattern:#x}: {ge.violations()}"
        assert ge.served, "no buffer of the call came from torch.empty"
        for name, h in zip("xwb", held):
            assert h[1]() == [], f"pattern {pattern:#x}, {name}: {h[1]()}"
        assert not torch.isnan(torch.view_as_real(y) if y.is_complex() else y).any(), f"pattern {pattern:#x}: NaN in y"
        outs.append(y)
    gu.same_bits(outs[0], outs[1], "NaN-filled against zero-filled buffers")
    return outs[0]


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("poly", ["default", "0"])
@pytest.mark.parametrize("i", sorted(CASES))
def test_forward_against_the_exact_result(i, poly, monkeypatch, ran):
    c = CASES[i]
    if poly == "0":
        monkeypatch.setenv("FFTCONV_LONG_POLY", "0")
    route = route_of(c)
    assert route == ("phases" if i in PHASES_CASES and poly == "default" else "spread")
    for cls in au.CLASSES:
        x, w, b, want, base = _data(i, cls)
        del ran[:]
        got = _guarded_call(c, x, w, b)
        assert got.shape == want.shape and got.dtype == F32 and got.is_contiguous()
        assert len(ran) == 2 and ran[0][0] is ran[1][0], ran
        plan = ran[0][0]
        if route == "phases":
            assert _is_phases(plan) and _points(plan) == PHASES_POINTS[i] and plan.out_len == out_len(c)
        else:
            assert not _is_phases(plan) and plan.key[11:15] == (0, c.s, c.d, 1) and plan.key[9] == 1, plan.key
            assert _points(plan) > F_.LONG_HANDOFF_POINTS
        au.check(f"case {i} [{cls}] {route}", got, want, base, F32)
        if i == 3 and route == "phases":      # phase 2 has no tap: its samples, the output_padding tail among them, are the bias itself
            assert torch.equal(got[..., 2::3], b.view(1, -1, 1).expand_as(got[..., 2::3]))
            assert torch.equal(got[..., -1], b.view(1, -1).expand(c.B, -1))


def test_case_1_phases_plan_is_half_the_spread_plan(monkeypatch, ran):
    c = CASES[1]
    x, w, b, want, base = _data(1, "centred")
    _call(c, x, w, b)
    monkeypatch.setenv("FFTCONV_LONG_POLY", "0")
    _call(c, x, w, b)
    (ph, _, _), (sp, _, _) = ran
    assert _is_phases(ph) and not _is_phases(sp)
    assert (ph.info["N1"], ph.info["N2"]) == (64, 64) and (sp.info["N1"], sp.info["N2"]) == (64, 128)
    assert ph.spectrum_bytes == sp.spectrum_bytes and ph.workspace_bytes < sp.workspace_bytes


def test_agrees_with_the_segment_route_of_fft_conv_transpose(ran):
    c = CASES[1]
    x, w, b, want, base = _data(1, "offset")
    long = _call(c, x, w, b)
    assert len(ran) == 1 and _is_phases(ran[0][0])
    seg = fft_conv_transpose(x, w, b, c.s, c.p, c.op, c.d, c.g)
    assert len(ran) == 1 and seg.shape == long.shape
    au.check("fft_conv_transpose (segments)", seg, want, base, F32)
    au.check("phases against fft_conv_transpose", long, seg, base, F32)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("poly", ["default", "0"])
def test_sixteen_bit_results_have_the_bits_of_the_cast_path(dtype, poly, monkeypatch, ran):
    c = CASES[5]
    if poly == "0":
        monkeypatch.setenv("FFTCONV_LONG_POLY", "0")
    x, w, b, want, base = _data(5, "centred")
    xh, wh, bh = (t.to(dtype) for t in (x, w, b))       # (integers up to 8: exact in both formats)
    got = _guarded_call(c, xh, wh, bh)
    assert got.dtype == dtype and _is_phases(ran[0][0]) == (poly == "default")
    ref = _call(c, x, w, b).to(dtype)
    gu.same_bits(got, ref, f"{dtype} against widen -> float32 call -> .to(dtype)")
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    gu.same_bits(_call(c, xh, wh, bh), ref, f"{dtype} under FFTCONV_HALF_IO=0")


def test_complex_rows_take_the_spread_route_and_match_four_real_calls(ran):
    c = CASES[1]
    assert route_of(c, C64) == "spread"
    x, w, b, want, base = _data(1, "centred", complex_=True)
    got = _guarded_call(c, x, w, b)
    assert got.dtype == C64 and all(not _is_phases(p) and p.complex for p, _, _ in ran)
    au.check("case 1 complex64", got, want, base, C64)
    # the bilinear product as four real calls of the same operation (these run by phases)
    del ran[:]
    re = _call(c, x.real.contiguous(), w.real.contiguous(), None) - _call(c, x.imag.contiguous(), w.imag.contiguous(), None)
    im = _call(c, x.real.contiguous(), w.imag.contiguous(), None) + _call(c, x.imag.contiguous(), w.real.contiguous(), None)
    assert len(ran) == 4 and all(_is_phases(p) for p, _, _ in ran)
    four = torch.complex(re, im) + b.view(1, -1, 1)
    au.check("four real calls", four, want, base, C64)
    au.check("complex64 against four real calls", got, four, base, C64)
    # a lazily conjugated signal is resolved on entry
    gu.same_bits(_call(c, x.conj(), w, b), _call(c, x.conj().resolve_conj(), w, b), "lazy conjugate")


def test_channels_last_takes_the_spread_route_with_the_bits_of_the_contiguous_call(monkeypatch, ran):
    """(The contiguous call it is compared with runs on the same route: the default contiguous call runs by phases, whose
    bits are those of other transforms.)"""
    c = CASES[1]
    x, w, b, want, base = _data(1, "offset")
    xl = x.transpose(1, 2).contiguous().transpose(1, 2)
    assert F_._long_layout(xl) == "nlc" and route_of(c, F32, ("nlc", True)) == "spread"
    got = _guarded_call(c, xl, w, b, channels_last=True)
    assert [(_is_phases(p), lx, ly) for p, lx, ly in ran] == [(False, _native.LONG_NCL, _native.LONG_NLC)] * 2, ran
    assert tuple(got.stride()) == (out_len(c) * c.cout, 1, c.cout)
    del ran[:]
    got2 = _call(c, xl, w, b, channels_last=True)       # (the signal read where it lies)
    assert [(_is_phases(p), lx, ly) for p, lx, ly in ran] == [(False, _native.LONG_NLC, _native.LONG_NLC)]
    au.check("case 1 channels-last", got, want, base, F32)
    monkeypatch.setenv("FFTCONV_LONG_POLY", "0")
    plain = _call(c, x, w, b)
    assert plain.is_contiguous()
    gu.same_bits(got.contiguous(), plain, "channels-last against the contiguous call")
    gu.same_bits(got2.contiguous(), plain, "channels-last signal against the contiguous call")
    monkeypatch.delenv("FFTCONV_LONG_POLY")
    half = _call(c, xl, w, b)                            # one of the two layouts is enough to leave the phases route
    assert half.is_contiguous()
    gu.same_bits(half, plain, "channels-last signal, contiguous result")


def test_phases_plan_refuses_channels_last_tensors():
    c = CASES[1]
    x, w, b, _, _ = _data(1, "centred")
    plan = F_._long_phases_plan(x, c.cout, c.g, c.k[0], c.s, c.p, c.op, True)
    spectrum = F_.transform_kernel(plan, w)
    out = torch.empty(c.B, c.cout, plan.out_len, device=DEV)
    ws = F_.new_workspace(plan, x.device)
    args = (x.data_ptr(), spectrum.buf.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream, 0, 0)
    for lay in ((_native.LONG_NLC, _native.LONG_NCL), (_native.LONG_NCL, _native.LONG_NLC)):
        with pytest.raises(NotImplementedError, match="phases plan reads and writes"):
            plan.forward_lay(*args, *lay)
    plan.forward_lay(*args, _native.LONG_NCL, _native.LONG_NCL)
    torch.cuda.synchronize()
    gu.same_bits(out, _call(c, x, w, b), "forward_lay with both layouts (B, C, L)")


def test_short_rows_hand_off(ran):
    x = au.integers((2, 4, 1000), torch.Generator().manual_seed(1), F32, DEV)
    w = au.integers((4, 2, 100), torch.Generator().manual_seed(2), F32, DEV)
    got = fft_long_conv_transpose(x, w, None, 2, 3, 1, 1, 2)
    assert ran == []
    want = torch.nn.functional.conv_transpose1d(x.double(), w.double(), None, 2, 3, 1, 2, 1)
    assert got.shape == want.shape and (got - want).abs().max().item() / want.abs().max().item() <= TOL32


# ------------------------------------------------------------------------------------------------ gradients
def _step(c, x, w, b, gy):
    xs, ws, bs = (t.detach().clone().requires_grad_() for t in (x, w, b))
    y = _call(c, xs, ws, bs)
    saved = [(t.dtype, t.numel()) for t in y.grad_fn.saved_tensors] if hasattr(y.grad_fn, "saved_tensors") else None
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), xs.grad, ws.grad, bs.grad, saved


@pytest.mark.parametrize("i,complex_", [(1, False), (2, False), (4, False), (7, False), (1, True)])
def test_gradients_against_float64_autograd(i, complex_, ran):
    c = CASES[i]
    dtype = C64 if complex_ else F32
    x, w, b, want_y, _ = _data(i, "centred", complex_)
    gy = au.grad_output(want_y.shape, dtype, DEV)
    y, dx, dw, db, _ = _step(c, x, w, b, gy)
    # the forward on its route, then dX (the forward strided primitive on dY) and dW (batch and channels exchanged)
    assert len(ran) == 3, ran
    assert _is_phases(ran[0][0]) == (route_of(c, dtype) == "phases")
    assert ran[1][0].key[11:15] == (0, 1, c.d, c.s) and ran[2][0].key[11:15] == (0, 1, c.s, c.d), [r[0].key for r in ran]
    assert ran[1][0].key[:4] == (c.B, c.cout, c.cin, c.g) and ran[2][0].key[:4] == (c.cout // c.g, c.g * c.B, c.cin, c.g)
    want = (want_y,) + au.truth_grads(c, x, w, b, gy, by_fft=c.k[0] > DIRECT_MAX_TAPS)
    base = au.baseline_grads(c, x, w, b, gy)
    for q, got_, want_, base_ in zip(("y", "dX", "dW", "db"), (y, dx, dw, db), want, base):
        assert got_.shape == want_.shape and got_.dtype == dtype, q
        au.check(f"case {i} {dtype} {q}", got_, want_, base_, dtype)


def test_sixteen_bit_gradients_have_the_bits_of_the_float32_cast_path(monkeypatch, ran):
    c, dtype = CASES[5], torch.bfloat16
    x, w, b, want_y, _ = _data(5, "centred")
    xh, wh, bh = (t.to(dtype) for t in (x, w, b))
    gy = au.grad_output(want_y.shape, dtype, DEV)
    code = F_._DTYPE_CODES[dtype]
    y, dx, dw, db, saved = _step(c, xh, wh, bh, gy)
    assert len(ran) == 3 and _is_phases(ran[0][0])
    assert sorted(saved) == sorted([(dtype, x.numel()), (dtype, w.numel())]), saved       # the 16-bit tensors are saved
    assert (dx.dtype, dw.dtype, db.dtype) == (dtype,) * 3 and dx.shape == x.shape and dw.shape == w.shape

    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    y0, dx0, dw0, db0, _ = _step(c, xh, wh, bh, gy)
    monkeypatch.delenv("FFTCONV_HALF_IO")
    for name, got, ref in (("y", y, y0), ("dX", dx, dx0), ("dW", dw, dw0), ("db", db, db0)):
        gu.same_bits(got, ref, f"{dtype} {name} (FFTCONV_HALF_IO=0)")
    # the cast written out by hand: float32 leaves, the float32 function, everything rounded once
    y32, dx32, dw32, db32, _ = _step(c, x, w, b, gy.float())
    for name, got, ref in (("y", y, y32), ("dX", dx, dx32), ("dW", dw, dw32), ("db", db, db32)):
        gu.same_bits(got, ref.to(dtype), f"{dtype} {name} against the float32 function")
    assert code == 3


# ------------------------------------------------------------------------------------------------ module
@pytest.mark.parametrize("dilation", [1, 2])
def test_module_cache_invalidation_and_graph_capture(dilation, monkeypatch, ran):
    """dilation 1: the phases plan transforms the weight itself; dilation 2: the spread plan a rearranged copy of it."""
    c = CASES[1]
    torch.manual_seed(0)
    layer = FFTLongConvTranspose1d(c.cin, c.cout, c.k[0], stride=c.s, padding=3, output_padding=1, groups=c.g,
                                   dilation=dilation).to(DEV)
    x = au.integers((c.B, c.cin, c.size[0]), torch.Generator().manual_seed(3), F32, DEV)
    calls = []
    real = F_.transform_kernel
    monkeypatch.setattr(F_, "transform_kernel", lambda plan, kernel: calls.append(plan) or real(plan, kernel))
    layer.eval()
    with torch.no_grad():
        y1, y2 = layer(x), layer(x)
    assert len(calls) == 1 and _is_phases(calls[0]) == (dilation == 1), calls       # one transform for two calls
    assert len(ran) == 2 and ran[0][0] is ran[1][0] is calls[0]
    want = torch.nn.functional.conv_transpose1d(x.double(), layer.weight.detach().double(), layer.bias.detach().double(),
                                                c.s, 3, 1, c.g, dilation)
    assert y1.shape == want.shape and au.e_max(y1, want) <= 1e-5 and torch.equal(y1, y2)
    gu.same_bits(y1, fft_long_conv_transpose(x, layer.weight.detach(), layer.bias.detach(), c.s, 3, 1, dilation, c.g),
                 "module against the functional")
    assert len(calls) == 2
    layer.invalidate_kernel_spectrum()
    with torch.no_grad():
        y3 = layer(x)
    assert len(calls) == 3 and torch.equal(y3, y1)
    # output_size picks the output padding as nn.ConvTranspose1d does
    with torch.no_grad():
        assert layer(x, output_size=[want.shape[2] - 1]).shape[2] == want.shape[2] - 1
    n_calls = len(calls)

    # a warm call captures and replays
    with torch.no_grad():
        layer(x)
    static_x = x.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        static_y = layer(static_x)
    assert len(calls) == n_calls + 1          # (output_size made another plan: the warm call transformed once more)
    for seed in (4, 5):
        fresh = au.integers(x.shape, torch.Generator().manual_seed(seed), F32, DEV)
        static_x.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            gu.same_bits(static_y, layer(fresh), f"replay {seed} against the eager call")


def test_module_trains_and_matches_conv_transpose1d(ran):
    c = CASES[2]
    torch.manual_seed(1)
    ref = torch.nn.ConvTranspose1d(c.cin, c.cout, c.k[0], stride=c.s, padding=c.p, output_padding=c.op, groups=c.g).double()
    layer = FFTLongConvTranspose1d(c.cin, c.cout, c.k[0], stride=c.s, padding=c.p, output_padding=c.op, groups=c.g)
    layer.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    layer = layer.to(DEV)
    ref.load_state_dict({k: v.double().cpu() for k, v in layer.state_dict().items()})
    x = torch.randn(c.B, c.cin, c.size[0], generator=torch.Generator().manual_seed(2))
    xs, x64 = x.to(DEV).requires_grad_(), x.double().requires_grad_()
    y = layer(xs)
    want = ref(x64)
    gy = torch.randn(want.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    y.backward(gy.float().to(DEV))
    want.backward(gy)
    assert len(ran) == 3 and _is_phases(ran[0][0])
    for name, got, r in (("y", y.detach(), want.detach()), ("dX", xs.grad, x64.grad), ("dW", layer.weight.grad, ref.weight.grad), ("db", layer.bias.grad, ref.bias.grad)):
        err = (got.double().cpu() - r).abs().max().item() / r.abs().max().item()
        assert err <= 1e-4, (name, err)
