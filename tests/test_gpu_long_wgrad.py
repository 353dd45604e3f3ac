"""The weight-gradient plan of ``fft_long_conv`` on the GPU (FFTCONV_LONG_WGRAD=1): ``long_wgrad_rows`` and the
weight-gradient build of ``long_cols_inv`` (csrc/long1d.hpp) on the table of tests/test_host_long_wgrad.py.

Inputs are the integers of tests/accuracy_util.py, so torch's float64 autograd of them is exact (``by_fft`` past 1100
taps); the bound is ``accuracy_util.check`` with its standard margins against the gradient of the model project's
formulation in float32.  Truth and baseline are those of the plain cross-correlation the layer is on its padded row
(a causal layer: against the flipped taps), computed once per layer and left unchanged."""
import pytest
import torch
import torch.nn.functional as F

from fft_conv_pytorch_amd import FFTLongConv1d, _native, autograd, fft_long_conv
from fft_conv_pytorch_amd import functional as F_
from tests import accuracy_util as au
from tests import guard_util as gu
from tests.route_util import Case
from tests.test_host_long_wgrad import KNOBS, TABLE, Layer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
DIRECT_MAX_TAPS = 1100        # longer filters take the float64 FFT truth (accuracy_util.truth_grads by_fft)


def _clear():
    _native.clear_plan_cache()
    F_._REFUSED_HALF.clear()
    autograd._BWD_PLANS.clear()


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for k in KNOBS + ("FFTCONV_TILE",):
        monkeypatch.delenv(k, raising=False)
    _clear()
    yield
    _clear()


@pytest.fixture
def ran(monkeypatch):
    """What ran: ``ran.fwd`` the long plans whose forward ran, ``ran.wgrad`` (plan, x layout, dY layout, dtype codes) per
    ``LongWgradPlan.run``, ``ran.made`` the weight-gradient plans created."""
    class Seen:
        fwd, wgrad, made = [], [], []
    seen = Seen()
    seen.fwd, seen.wgrad, seen.made = [], [], []
    real, real_lay, real_run, real_init = (_native.LongPlan.forward, _native.LongPlan.forward_lay, _native.LongWgradPlan.run,
                                           _native.LongWgradPlan.__init__)

    def forward(plan, *args):
        seen.fwd.append(plan)
        return real(plan, *args)

    def forward_lay(plan, *args):
        seen.fwd.append(plan)
        return real_lay(plan, *args)

    def run(plan, *args):
        seen.wgrad.append((plan, args[8], args[9], args[5:8]))
        return real_run(plan, *args)

    def init(plan, *args, **kw):
        seen.made.append(plan)
        return real_init(plan, *args, **kw)
    monkeypatch.setattr(_native.LongPlan, "forward", forward)
    monkeypatch.setattr(_native.LongPlan, "forward_lay", forward_lay)
    monkeypatch.setattr(_native.LongWgradPlan, "run", run)
    monkeypatch.setattr(_native.LongWgradPlan, "__init__", init)
    return seen


# ------------------------------------------------------------------------------------------------ data
def _view(lay):
    """The layer as the plain cross-correlation ``accuracy_util`` knows, on the row padded by hand -> (case, prepare)."""
    pl, pr, nout = lay.words()
    view = Case(lay.B, lay.cin, lay.cout, (lay.L + pl + pr,), (lay.K,), s=lay.s, d=lay.d, g=lay.g, note=lay.note)

    def prepare(x, w):
        xp = F.pad(x, (pl, pr)) if lay.mode == "constant" else F.pad(x, (pl, pr), mode=lay.mode)
        return xp, (w.flip(-1) if lay.causal else w)
    return view, prepare, nout


_SHARED = {}


def _data(lay):
    """(x, w, b, dY, exact dW, float32 baseline dW) of a layer, computed once and left unchanged."""
    if lay not in _SHARED:
        view, prepare, nout = _view(lay)
        au.assert_exact(view, "centred")
        x, w, b = au.inputs(Case(lay.B, lay.cin, lay.cout, (lay.L,), (lay.K,), g=lay.g), "centred", DEV)
        xv, wv = prepare(x, w)
        gy = au.grad_output((lay.B, lay.cout, nout), F32, DEV)
        # (a causal layer keeps the first nout samples of the row's outputs: the others get a zero gradient)
        full = au.out_spatial(view)[0]
        gyv = F.pad(gy, (0, full - nout))
        want = au.truth_grads(view, xv, wv, b, gyv, by_fft=lay.K > DIRECT_MAX_TAPS)[1]
        base = au.baseline_grads(view, xv, wv, b, gyv)[2]
        if lay.causal:
            want, base = want.flip(-1), base.flip(-1)
        _SHARED[lay] = (x, w, b, gy, want, base)
    return _SHARED[lay]


def _call(lay, x, w, b, **kw):
    return fft_long_conv(x, w, b, 0 if lay.causal else lay.p, lay.g, lay.causal, stride=lay.s, dilation=lay.d,
                         padding_mode=lay.mode, **kw)


def _step(lay, x, w, b, gy, only_w=False, **kw):
    """One training step -> (y, dX, dW, db, saved (dtype, numel), backward's peak bytes above what was allocated)."""
    xs, ws, bs = (t.detach().clone().requires_grad_(not only_w or t is w) for t in (x, w, b))
    y = _call(lay, xs, ws, bs, **kw)
    saved = [(t.dtype, t.numel()) for t in y.grad_fn.saved_tensors]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), xs.grad, ws.grad, bs.grad, saved, torch.cuda.max_memory_allocated() - before


def _check_dw(what, lay, dw, dtype=F32):
    x, w, b, gy, want, base = _data(lay)
    assert dw.shape == want.shape == w.shape and dw.dtype == dtype and dw.is_contiguous(), what
    return au.check(what, dw, want, base, F32)


def _plan_step(lay, monkeypatch, ran, **kw):
    """The step under FFTCONV_LONG_WGRAD=1 with the route asserted: the forward and dX on plain long plans, dW on ONE
    weight-gradient plan."""
    monkeypatch.setenv("FFTCONV_LONG_WGRAD", "1")
    assert lay.route() == "plan"
    x, w, b, gy, _, _ = _data(lay)
    del ran.fwd[:], ran.wgrad[:]
    out = _step(lay, x, w, b, gy, **kw)
    assert len(ran.fwd) == 2 and all(type(p) is _native.LongPlan for p in ran.fwd), ran.fwd
    assert len(ran.wgrad) == 1 and ran.wgrad[0][0].key == lay.key(), ran.wgrad
    return out


# ------------------------------------------------------------------------------------------------ the cases
def test_1_depthwise_causal_without_transposed_copies(monkeypatch, ran):
    lay = TABLE["1"]
    y, dx, dw, db, saved, _ = _plan_step(lay, monkeypatch, ran)
    plan = ran.wgrad[0][0]
    assert plan.info["slab_pairs"] == 2 and plan.info["slabs"] == 1 and plan.info["lags"] == lay.K
    _check_dw("case 1 dW", lay, dw)
    # neither permute(...).contiguous() operand nor the flipped copy exists: with dW alone asked for, the exchanged route
    # holds xt and dyt on top of a spectrum and a workspace that are no smaller than the plan's one workspace
    x, w, b, gy, _, _ = _data(lay)
    peak_plan = _step(lay, x, w, b, gy, only_w=True)[5]
    monkeypatch.delenv("FFTCONV_LONG_WGRAD")
    made = len(ran.made)
    *_, dw0, _, _, peak_exchanged = _step(lay, x, w, b, gy, only_w=True)
    assert len(ran.made) == made
    copies = x.numel() * 4 + gy.numel() * 4
    print(f"    backward peak: plan {peak_plan} bytes, exchanged {peak_exchanged} bytes, xt + dyt {copies} bytes")
    assert peak_plan + copies <= peak_exchanged
    _check_dw("case 1 dW, exchanged route", lay, dw0)


def test_2_grouped_dense(monkeypatch, ran):
    lay = TABLE["2"]
    y, dx, dw, db, _, _ = _plan_step(lay, monkeypatch, ran)
    _check_dw("case 2 dW", lay, dw)
    # dX and db are those of the unset switch, bit for bit
    monkeypatch.delenv("FFTCONV_LONG_WGRAD")
    x, w, b, gy, _, _ = _data(lay)
    y0, dx0, dw0, db0, _, _ = _step(lay, x, w, b, gy)
    for name, a, b_ in (("y", y, y0), ("dX", dx, dx0), ("db", db, db0)):
        gu.same_bits(a, b_, f"case 2 {name} under the switch against unset")


@pytest.mark.parametrize("name", ["3", "3s", "3c", "3r"])
def test_3_stride_dilation_and_padding_modes(name, monkeypatch, ran):
    lay = TABLE[name]
    if name == "3s":
        assert lay.words()[:2] == (58, 59)
    dw = _plan_step(lay, monkeypatch, ran)[2]
    _check_dw(f"case {name} dW ({lay.note})", lay, dw)


def test_4_causal_filter_longer_than_the_row(monkeypatch, ran):
    lay = TABLE["4"]
    dw = _plan_step(lay, monkeypatch, ran)[2]
    assert ran.wgrad[0][0].info["lags"] == lay.L
    # tap k >= L of the causal filter meets no sample: exactly 0.0, in the weight's own order
    assert dw[..., lay.L:].numel() and not dw[..., lay.L:].any()
    assert dw[..., :lay.L].any()
    _check_dw("case 4 dW", lay, dw)


def test_5_partial_last_block_of_output_channels(monkeypatch, ran):
    ob = _native.wgrad_geometry(Layer(2, 3, 1, 4300, 200, p=7).key())["out_block"]
    lay = Layer(2, 6, 2 * (ob + 1), 4300, 200, g=2, p=7, note="Cog = out_block + 1")
    dw = _plan_step(lay, monkeypatch, ran)[2]
    info = ran.wgrad[0][0].info
    assert info["out_block"] == ob and lay.cout // lay.g == info["out_block"] + 1 and lay.cin // lay.g == 3
    _check_dw("case 5 dW", lay, dw)


def test_6_one_item_and_three_slabs(monkeypatch, ran):
    dw = _plan_step(TABLE["6a"], monkeypatch, ran)[2]
    _check_dw("case 6a dW (B 1)", TABLE["6a"], dw)
    lay = TABLE["6b"]
    one = _plan_step(lay, monkeypatch, ran)[2]
    assert ran.wgrad[0][0].info["slabs"] == 1
    _check_dw("case 6b dW (B 5, one slab)", lay, one)
    # room for W2 and the W1 rows of one pair, not of two
    n, rows = 8192, lay.cout * lay.cin // lay.g
    monkeypatch.setenv("FFTCONV_LONG_WS_MB", str(-(-((rows + lay.cin + lay.cout) * n * 8) // (1 << 20))))
    _clear()
    three = _plan_step(lay, monkeypatch, ran)[2]
    info = ran.wgrad[0][0].info
    assert (info["N1"] * info["N2"], info["slabs"], info["slab_pairs"]) == (n, 3, 1), info
    _check_dw("case 6b dW (B 5, three slabs)", lay, three)


@pytest.mark.parametrize("n1,n2", [(64, 128), (128, 64), (64, 4096), (4096, 64), (512, 512), (64, 256), (64, 1024), (64, 2048)])
def test_7_every_tile(n1, n2, monkeypatch, ran):
    lay = TABLE["2"]
    monkeypatch.setenv("FFTCONV_LONG_N", f"{n1}x{n2}")
    dw = _plan_step(lay, monkeypatch, ran)[2]
    info = ran.wgrad[0][0].info
    assert (info["N1"], info["N2"]) == (n1, n2)
    _check_dw(f"case 2 dW at {n1} x {n2}", lay, dw)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_8_sixteen_bit_tensors(dtype, monkeypatch, ran):
    lay = TABLE["2"]
    x, w, b, gy, _, _ = _data(lay)
    monkeypatch.setenv("FFTCONV_LONG_WGRAD", "1")
    y32, dx32, dw32, db32, _, _ = _step(lay, x, w, b, gy)
    del ran.fwd[:], ran.wgrad[:]
    xh, wh, bh, gyh = (t.to(dtype) for t in (x, w, b, gy))        # (integers up to 8: exact in both formats)
    y, dx, dw, db, saved, _ = _step(lay, xh, wh, bh, gyh)
    code = F_._DTYPE_CODES[dtype]
    assert len(ran.wgrad) == 1 and ran.wgrad[0][3] == (code, code, code), ran.wgrad
    assert sorted(saved) == sorted([(dtype, x.numel()), (dtype, w.numel())]), saved       # the 16-bit tensors are saved
    assert dw.dtype == dtype and dw.shape == w.shape
    gu.same_bits(dw, dw32.to(dtype), f"{dtype} dW against the float32 call's dW rounded once")
    gu.same_bits(dx, dx32.to(dtype), f"{dtype} dX")


def test_9_channels_last_operands(monkeypatch, ran):
    lay = TABLE["2"]
    x, w, b, gy, _, _ = _data(lay)
    monkeypatch.setenv("FFTCONV_LONG_WGRAD", "1")
    ref = _step(lay, x, w, b, gy)[2]
    assert ran.wgrad[-1][1:3] == (_native.LONG_NCL, _native.LONG_NCL)
    nlc = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)      # noqa: E731
    xl, gyl = nlc(x), nlc(gy)
    assert F_._long_layout(xl) == "nlc" and F_._long_layout(gyl) == "nlc"
    for what, xs, gys, cl, lays in (("both", xl, gyl, True, (_native.LONG_NLC, _native.LONG_NLC)),
                                    ("x alone", xl, gy, False, (_native.LONG_NLC, _native.LONG_NCL)),
                                    ("dY alone", x, gyl, True, (_native.LONG_NCL, _native.LONG_NLC))):
        dw = _step(lay, xs, w, b, gys, channels_last=cl)[2]
        assert ran.wgrad[-1][1:3] == lays, (what, ran.wgrad[-1])
        gu.same_bits(dw, ref, f"channels-last {what} against the contiguous call")
    # FFTCONV_LONG_NLC=0: torch copies, the same bits
    monkeypatch.setenv("FFTCONV_LONG_NLC", "0")
    dw = _step(lay, xl, w, b, gyl, channels_last=True)[2]
    assert ran.wgrad[-1][1:3] == (_native.LONG_NCL, _native.LONG_NCL)
    gu.same_bits(dw, ref, "channels-last tensors under FFTCONV_LONG_NLC=0")


@pytest.mark.parametrize("name", ["1", "4"])
def test_10_memory_discipline(name, monkeypatch, ran):
    lay = TABLE[name]
    x, w, b, gy, _, _ = _data(lay)
    monkeypatch.setenv("FFTCONV_LONG_WGRAD", "1")
    outs = []
    for pattern in (0xFF, 0x00):
        held = [gu.guarded(t, pattern, offset=1) for t in (x, w, gy)]
        xs, ws = (h[0].requires_grad_() for h in held[:2])
        with gu.guarded_empty(pattern) as ge:
            y = _call(lay, xs, ws, None)
            y.backward(held[2][0])
        assert ge.violations() == [], f"pattern {pattern:#x}: {ge.violations()}"
        assert ge.served, "no buffer of the step came from torch.empty"
        for what, h in zip(("x", "w", "dY"), held):
            assert h[1]() == [], f"pattern {pattern:#x}, {what}: {h[1]()}"
        assert au.finite(ws.grad), f"pattern {pattern:#x}: dW not finite"
        outs.append(ws.grad.clone())
    assert len(ran.wgrad) == 2
    gu.same_bits(outs[0], outs[1], "dW into NaN-filled against zero-filled buffers")
    _check_dw(f"case {name} dW between guard bands", lay, outs[0])


def test_11_routes_that_stay(monkeypatch, ran):
    lay = TABLE["2"]
    x, w, b, gy, _, _ = _data(lay)
    # the switch unset
    _step(lay, x, w, b, gy)
    assert len(ran.fwd) == 3 and not ran.made and not ran.wgrad
    assert ran.fwd[2].key[:5] == (lay.cin // lay.g, lay.g * lay.B, lay.cout, lay.g, lay.L), ran.fwd[2].key
    monkeypatch.setenv("FFTCONV_LONG_WGRAD", "1")
    # complex64
    del ran.fwd[:]
    xc, wc, bc = (torch.complex(t, t.flip(0)) for t in (x, w, b))
    xs, ws = xc.clone().requires_grad_(), wc.clone().requires_grad_()
    yc = _call(lay, xs, ws, bc)
    yc.backward(torch.complex(gy, gy))
    torch.cuda.synchronize()
    assert len(ran.fwd) == 3 and all(p.complex for p in ran.fwd) and not ran.made and not ran.wgrad
    # a non-causal strided forward that ran by phases: its gradients by phases
    monkeypatch.setenv("FFTCONV_LONG_DECIM", "1")
    strided = Layer(2, 2, 2, 9000, 600, s=2, p=3)
    assert strided.route() == "exchanged"
    del ran.fwd[:]
    xs = au.integers((2, 2, 9000), torch.Generator().manual_seed(1), F32, DEV).requires_grad_()
    ws = au.integers(strided.wshape, torch.Generator().manual_seed(2), F32, DEV).requires_grad_()
    ys = _call(strided, xs, ws, None)
    ys.backward(au.grad_output(ys.shape, F32, DEV))
    torch.cuda.synchronize()
    assert len(ran.fwd) == 3 and isinstance(ran.fwd[0], _native.LongDecimPlan) and not ran.made and not ran.wgrad
    assert au.finite(ws.grad) and ws.grad.shape == strided.wshape


def test_12_a_captured_training_step_replays_bit_for_bit(monkeypatch, ran):
    lay = TABLE["1"]
    x, w, b, gy, _, _ = _data(lay)
    monkeypatch.setenv("FFTCONV_LONG_WGRAD", "1")
    layer = FFTLongConv1d(lay.cin, lay.cout, lay.K, groups=lay.g, causal=True).to(DEV)
    with torch.no_grad():
        layer.weight.copy_(w)
        layer.bias.copy_(b)
    static_x, static_gy = x.clone().requires_grad_(), gy.clone()

    def zero():
        static_x.grad = None
        layer.zero_grad(set_to_none=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):               # warm: plans, tables and the allocator's pools exist
            zero()
            layer(static_x).backward(static_gy)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert len(ran.made) == 1 and len(ran.wgrad) == 2
    zero()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        layer(static_x).backward(static_gy)
    assert len(ran.made) == 1 and len(ran.wgrad) == 3
    for seed in (4, 5):
        fresh = au.integers(x.shape, torch.Generator().manual_seed(seed), F32, DEV)
        fresh_gy = au.integers(gy.shape, torch.Generator().manual_seed(seed + 10), F32, DEV)
        with torch.no_grad():
            static_x.copy_(fresh)
            static_gy.copy_(fresh_gy)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in (static_x.grad, layer.weight.grad, layer.bias.grad)]
        xs = fresh.clone().requires_grad_()
        ws, bs = layer.weight.detach().clone().requires_grad_(), layer.bias.detach().clone().requires_grad_()
        _call(lay, xs, ws, bs).backward(fresh_gy)
        for name, a, e in zip(("dX", "dW", "db"), got, (xs.grad, ws.grad, bs.grad)):
            gu.same_bits(a, e, f"replay {seed} {name} against the eager step")
