"""``fft_long_conv`` by phases on the GPU: the decimation builds of ``long_cols_fwd`` (csrc/long1d.hpp) in the forward, the
gradients of a forward that ran by phases, and the gradients of ``fft_long_conv_transpose`` on rows ``stride`` times
shorter, on the table of tests/test_host_long_decim.py, under FFTCONV_LONG_DECIM=1 and =0.

Inputs are the integers of tests/accuracy_util.py, so torch's float64 convolution of them is exact; the bound is
``accuracy_util.check`` with its standard margins against the model project's formulation in float32.  Every forward case
runs between guard bands into NaN-filled and zero-filled buffers; 16-bit results and gradients are compared bit for bit
with the cast path on the same route.  A truth and a baseline are computed once per (case, class) and shared."""
import pytest
import torch
import torch.nn.functional as F

from fft_conv_pytorch_amd import FFTLongConv1d, _native, autograd, fft_long_conv, fft_long_conv_transpose
from fft_conv_pytorch_amd import functional as F_
from tests import accuracy_util as au
from tests import guard_util as gu
from tests.route_util import Case
from tests.test_host_long_decim import CASES, CAUSAL, PHASES_CASES, as_forward_case, out_len, route_of
from tests.test_host_long_transpose import CASES as TCASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
KNOBS = ("FFTCONV_LONG_DECIM", "FFTCONV_LONG_POLY", "FFTCONV_LONG_NLC", "FFTCONV_LONG_N", "FFTCONV_LONG_WS_MB", "FFTCONV_HALF_IO",
         "FFTCONV_TILE")
DIRECT_MAX_TAPS = 1100        # longer filters take the float64 FFT truth (accuracy_util.truth_by_fft)
MODES = ["1", "0"]


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


def _is_decim(plan):
    return isinstance(plan, _native.LongDecimPlan)


def _is_plain(plan):
    return type(plan) is _native.LongPlan


def _points(plan):
    return plan.info["N1"] * plan.info["N2"]


def _snug(plan, need):
    """The plan's transform is the smallest that holds ``need`` points."""
    n = _points(plan)
    return n >= need and (n == 4096 or n < 2 * need)


_SHARED = {}


def _data(i, cls):
    """(x, w, b, exact y, float32 baseline y) of case i, computed once and left unchanged."""
    key = (i, cls)
    if key not in _SHARED:
        c = CASES[i]
        view, prepare = as_forward_case(i)
        au.assert_exact(view, cls)
        x, w, b = au.inputs(c, cls, DEV)
        xv, wv = prepare(x, w)
        want = au.truth(view, xv, wv, b) if c.k[0] <= DIRECT_MAX_TAPS else au.truth_by_fft(view, xv, wv, b)
        assert tuple(want.shape) == (c.B, c.cout, out_len(i))
        _SHARED[key] = (x, w, b, want, au.baseline(view, xv, wv, b))
    return _SHARED[key]


def _call(i, x, w, b, **kw):
    c = CASES[i]
    return fft_long_conv(x, w, b, c.p, c.g, i in CAUSAL, stride=c.s, dilation=c.d, **kw)


def _guarded_call(i, x, w, b, **kw):
    """The call into NaN-filled and into zero-filled buffers, the inputs between guard bands of their own: no byte outside
    a tensor changes, the inputs keep their bits, the two results agree bit for bit and hold no NaN."""
    outs = []
    for pattern in (0xFF, 0x00):
        held = [gu.guarded(t, pattern, offset=1) for t in (x, w, b)]
        with gu.guarded_empty(pattern) as ge:
            y = _call(i, *(h[0] for h in held), **kw)
        assert ge.violations() == [], f"pattern {pattern:#x}: {ge.violations()}"
        assert ge.served, "no buffer of the call came from torch.empty"
        for name, h in zip("xwb", held):
            assert h[1]() == [], f"pattern {pattern:#x}, {name}: {h[1]()}"
        assert not torch.isnan(y).any(), f"pattern {pattern:#x}: NaN in y"
        outs.append(y)
    gu.same_bits(outs[0], outs[1], "NaN-filled against zero-filled buffers")
    return outs[0]


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("i", sorted(CASES))
def test_forward_against_the_exact_result(i, mode, monkeypatch, ran):
    c = CASES[i]
    monkeypatch.setenv("FFTCONV_LONG_DECIM", mode)
    route = route_of(i)
    assert route == ("phases" if i in PHASES_CASES and mode == "1" else "plain")
    for cls in au.CLASSES:
        x, w, b, want, base = _data(i, cls)
        del ran[:]
        got = _guarded_call(i, x, w, b)
        assert got.shape == want.shape and got.dtype == F32 and got.is_contiguous()
        assert len(ran) == 2 and ran[0][0] is ran[1][0], ran
        plan = ran[0][0]
        if route == "phases":
            assert _is_decim(plan) and plan.out_len == out_len(i)
            assert _snug(plan, out_len(i) + -(-c.k[0] // c.s) - 1), plan.info
        else:
            assert _is_plain(plan) and plan.key[11:15] == (0, 1, c.d, c.s), plan.key
            assert _points(plan) > F_.LONG_HANDOFF_POINTS
        au.check(f"case {i} [{cls}] {route}", got, want, base, F32)


def test_case_1_decimated_plan_has_half_the_points_of_the_plain_plan(monkeypatch, ran):
    x, w, b, want, base = _data(1, "centred")
    monkeypatch.setenv("FFTCONV_LONG_DECIM", "1")
    _call(1, x, w, b)
    monkeypatch.setenv("FFTCONV_LONG_DECIM", "0")
    _call(1, x, w, b)
    (dec, _, _), (plain, _, _) = ran
    assert _is_decim(dec) and _is_plain(plain)
    assert (dec.info["N1"], dec.info["N2"]) == (64, 128) and (plain.info["N1"], plain.info["N2"]) == (128, 128)
    assert dec.spectrum_bytes == plain.spectrum_bytes and dec.workspace_bytes < plain.workspace_bytes


@pytest.mark.parametrize("n1", [64, 128, 256, 512, 1024, 2048, 4096])
def test_case_1_at_every_column_length(n1, monkeypatch, ran):
    """Every N1 of the engine runs the decimation builds of its geometry (N2 = 128 where the row needs it, else 64)."""
    monkeypatch.setenv("FFTCONV_LONG_DECIM", "1")
    monkeypatch.setenv("FFTCONV_LONG_N", f"{n1}x{128 if n1 == 64 else 64}")
    x, w, b, want, base = _data(1, "offset")
    got = _guarded_call(1, x, w, b)
    assert _is_decim(ran[0][0]) and ran[0][0].info["N1"] == n1
    au.check(f"case 1 N1 = {n1}", got, want, base, F32)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("mode", MODES)
def test_sixteen_bit_results_have_the_bits_of_the_cast_path(dtype, mode, monkeypatch, ran):
    monkeypatch.setenv("FFTCONV_LONG_DECIM", mode)
    x, w, b, want, base = _data(5, "centred")
    xh, wh, bh = (t.to(dtype) for t in (x, w, b))       # (integers up to 8: exact in both formats)
    got = _guarded_call(5, xh, wh, bh)
    assert got.dtype == dtype and _is_decim(ran[0][0]) == (mode == "1")
    ref = _call(5, x, w, b).to(dtype)
    gu.same_bits(got, ref, f"{dtype} against widen -> float32 call -> .to(dtype)")
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    gu.same_bits(_call(5, xh, wh, bh), ref, f"{dtype} under FFTCONV_HALF_IO=0")


@pytest.mark.parametrize("mode", MODES)
def test_channels_last_result_and_signal(mode, monkeypatch, ran):
    """A channels-last RESULT comes from the unchanged last pass and has the bits of the contiguous call; a channels-last
    SIGNAL takes the plain route in every mode."""
    monkeypatch.setenv("FFTCONV_LONG_DECIM", mode)
    c = CASES[1]
    x, w, b, want, base = _data(1, "offset")
    plain = _call(1, x, w, b)
    del ran[:]
    got = _guarded_call(1, x, w, b, channels_last=True)
    assert [(_is_decim(p), lx, ly) for p, lx, ly in ran] == [(mode == "1", _native.LONG_NCL, _native.LONG_NLC)] * 2, ran
    assert tuple(got.stride()) == (out_len(1) * c.cout, 1, c.cout)
    gu.same_bits(got.contiguous(), plain, "channels-last result against the contiguous call")
    au.check("case 1 channels-last result", got, want, base, F32)
    xl = x.transpose(1, 2).contiguous().transpose(1, 2)
    assert F_._long_layout(xl) == "nlc" and route_of(1, F32, "nlc") == "plain"
    del ran[:]
    got2 = _call(1, xl, w, b)
    assert [(_is_plain(p), lx, ly) for p, lx, ly in ran] == [(True, _native.LONG_NLC, _native.LONG_NCL)], ran
    au.check("case 1 channels-last signal", got2, want, base, F32)


def test_decimation_plan_refuses_a_channels_last_signal():
    c = CASES[1]
    x, w, b, _, _ = _data(1, "centred")
    plan = F_._long_decim_plan(x, c.cout, c.g, c.k[0], c.s, c.p, c.p, 0, False, True)
    spectrum = F_.transform_kernel(plan, w)
    out = torch.empty(c.B, c.cout, plan.out_len, device=DEV)
    ws = F_.new_workspace(plan, x.device)
    args = (x.data_ptr(), spectrum.buf.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream, 0, 0)
    with pytest.raises(NotImplementedError, match="decimation plan reads a"):
        plan.forward_lay(*args, _native.LONG_NLC, _native.LONG_NCL)
    plan.forward_lay(*args, _native.LONG_NCL, _native.LONG_NCL)
    torch.cuda.synchronize()
    want = F.conv1d(x.double(), w.double(), b.double(), c.s, c.p, 1, c.g)
    assert au.e_max(out, want) <= 1e-5


# ------------------------------------------------------------------------------------------------ gradients
def _step(fn, x, w, b, gy):
    xs, ws, bs = (t.detach().clone().requires_grad_() for t in (x, w, b))
    y = fn(xs, ws, bs)
    saved = [(t.dtype, t.numel()) for t in y.grad_fn.saved_tensors] if hasattr(y.grad_fn, "saved_tensors") else None
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), xs.grad, ws.grad, bs.grad, saved


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("i", [1, 2, 4, 6])
def test_gradients_against_float64_autograd(i, mode, monkeypatch, ran):
    c = CASES[i]
    monkeypatch.setenv("FFTCONV_LONG_DECIM", mode)
    x, w, b, want_y, _ = _data(i, "centred")
    gy = au.grad_output(want_y.shape, F32, DEV)
    y, dx, dw, db, _ = _step(lambda *t: _call(i, *t), x, w, b, gy)
    assert len(ran) == 3, ran
    L, K, kp = c.size[0], c.k[0], -(-c.k[0] // c.s)
    if mode == "1":
        # the forward decimated, dX the transposed convolution of dY by phases, dW with the phases of x as batch
        assert _is_decim(ran[0][0]) and isinstance(ran[1][0], _native.LongPhasesPlan) and _is_plain(ran[2][0]), ran
        assert ran[1][0].out_len == L and ran[1][0].key[5:9] == (K, c.s, c.p, (L + 2 * c.p - K) % c.s), ran[1][0].key
        assert ran[2][0].key[:11] == (c.cin // c.g * c.s, c.g * c.B, c.cout, c.g, out_len(i) + kp - 1, out_len(i), 0, 0, kp, 0, 0)
        assert len(ran[2][0].key) == 11 and _snug(ran[2][0], out_len(i) + kp - 1)
    else:
        assert all(_is_plain(p) for p, _, _ in ran)
        assert ran[0][0].key[11:15] == (0, 1, 1, c.s) and ran[1][0].key[11:15] == (0, c.s, 1, 1) and ran[2][0].key[11:15] == (0, 1, c.s, 1)
    want = (want_y,) + au.truth_grads(c, x, w, b, gy, by_fft=K > DIRECT_MAX_TAPS)
    base = au.baseline_grads(c, x, w, b, gy)
    for q, got_, want_, base_ in zip(("y", "dX", "dW", "db"), (y, dx, dw, db), want, base):
        assert got_.shape == want_.shape and got_.dtype == F32, q
        au.check(f"case {i} {q} (FFTCONV_LONG_DECIM={mode})", got_, want_, base_, F32)


def test_a_causal_forward_by_phases_keeps_the_plain_gradients(monkeypatch, ran):
    """Case 7 (causal, K = L, flipped taps): the forward runs decimated, dX and dW on the plain plans of before."""
    c, K = CASES[7], CASES[7].k[0]
    monkeypatch.setenv("FFTCONV_LONG_DECIM", "1")
    x, w, b, want_y, _ = _data(7, "centred")
    gy = au.grad_output(want_y.shape, F32, DEV)
    y, dx, dw, db, _ = _step(lambda *t: _call(7, *t), x, w, b, gy)
    assert len(ran) == 3 and _is_decim(ran[0][0]) and _is_plain(ran[1][0]) and _is_plain(ran[2][0]), ran
    assert ran[1][0].key[11:15] == (0, c.s, 1, 1) and ran[2][0].key[11:15] == (0, 1, c.s, 1), [r[0].key for r in ran]
    # the gradients of the row with K - 1 zeros in front against the flipped taps, carried back to x and w
    view, prepare = as_forward_case(7)
    xv, wv = prepare(x, w)
    tdx, tdw, tdb = au.truth_grads(view, xv, wv, b, gy, by_fft=True)
    _, bdx, bdw, bdb = au.baseline_grads(view, xv, wv, b, gy)
    for q, got_, want_, base_ in (("dX", dx, tdx[..., K - 1:], bdx[..., K - 1:]), ("dW", dw, tdw.flip(-1), bdw.flip(-1)),
                                  ("db", db, tdb, bdb)):
        assert got_.shape == want_.shape and got_.dtype == F32, q
        au.check(f"case 7 causal {q}", got_, want_, base_, F32)


@pytest.mark.parametrize("mode", MODES)
def test_sixteen_bit_gradients_have_the_bits_of_the_float32_cast_path(mode, monkeypatch, ran):
    dtype = torch.bfloat16
    monkeypatch.setenv("FFTCONV_LONG_DECIM", mode)
    x, w, b, want_y, _ = _data(5, "centred")
    xh, wh, bh = (t.to(dtype) for t in (x, w, b))
    gy = au.grad_output(want_y.shape, dtype, DEV)
    fn = lambda *t: _call(5, *t)      # noqa: E731
    y, dx, dw, db, saved = _step(fn, xh, wh, bh, gy)
    assert len(ran) == 3 and _is_decim(ran[0][0]) == (mode == "1")
    assert sorted(saved) == sorted([(dtype, x.numel()), (dtype, w.numel())]), saved       # the 16-bit tensors are saved
    assert (dx.dtype, dw.dtype, db.dtype) == (dtype,) * 3 and dx.shape == x.shape and dw.shape == w.shape
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    y0, dx0, dw0, db0, _ = _step(fn, xh, wh, bh, gy)
    monkeypatch.delenv("FFTCONV_HALF_IO")
    for name, got, ref in (("y", y, y0), ("dX", dx, dx0), ("dW", dw, dw0), ("db", db, db0)):
        gu.same_bits(got, ref, f"{dtype} {name} (FFTCONV_HALF_IO=0)")
    # the cast written out by hand: float32 leaves, the float32 function, everything rounded once
    y32, dx32, dw32, db32, _ = _step(fn, x, w, b, gy.float())
    for name, got, ref in (("y", y, y32), ("dX", dx, dx32), ("dW", dw, dw32), ("db", db, db32)):
        gu.same_bits(got, ref.to(dtype), f"{dtype} {name} against the float32 function")


@pytest.mark.parametrize("i", [1, 2, 4, 5])
def test_transposed_gradients_run_on_decimated_rows(i, monkeypatch, ran):
    """``fft_long_conv_transpose`` under FFTCONV_LONG_DECIM=1: dX on a decimation plan, dW on a plain plan of about
    L + ceil(K / s) points, both against float64 autograd."""
    c = TCASES[i]
    monkeypatch.setenv("FFTCONV_LONG_DECIM", "1")
    au.assert_exact(c, "centred")
    x, w, b = au.inputs(c, "centred", DEV)
    by_fft = c.k[0] > DIRECT_MAX_TAPS
    want_y = au.truth_by_fft(c, x, w, b) if by_fft else au.truth(c, x, w, b)
    gy = au.grad_output(want_y.shape, F32, DEV)
    y, dx, dw, db, _ = _step(lambda *t: fft_long_conv_transpose(*t, c.s, c.p, c.op, c.d, c.g), x, w, b, gy)
    L, K, kp, cog = c.size[0], c.k[0], -(-c.k[0] // c.s), c.cout // c.g
    assert len(ran) == 3 and isinstance(ran[0][0], _native.LongPhasesPlan), ran
    assert _is_decim(ran[1][0]) and ran[1][0].out_len == L and _snug(ran[1][0], L + kp - 1), ran[1][0].info
    assert ran[1][0].key == (c.B, c.cout, c.cin, c.g, want_y.shape[2], K, c.s, c.p, c.p, L, 0, 0), ran[1][0].key
    assert _is_plain(ran[2][0]) and ran[2][0].key == (cog * c.s, c.g * c.B, c.cin, c.g, L + kp - 1, L, 0, 0, kp, 0, 0), ran[2][0].key
    assert _snug(ran[2][0], L + kp - 1)
    want = (want_y,) + au.truth_grads(c, x, w, b, gy, by_fft=by_fft)
    base = au.baseline_grads(c, x, w, b, gy)
    for q, got_, want_, base_ in zip(("y", "dX", "dW", "db"), (y, dx, dw, db), want, base):
        assert got_.shape == want_.shape and got_.dtype == F32, q
        au.check(f"transposed case {i} {q}", got_, want_, base_, F32)
    # FFTCONV_LONG_DECIM=0 and the variable unset: the constructions of before (these rows fit them)
    for value in ("0", None):
        if value is None:
            monkeypatch.delenv("FFTCONV_LONG_DECIM")
        else:
            monkeypatch.setenv("FFTCONV_LONG_DECIM", value)
        del ran[:]
        _, dx0, dw0, _, _ = _step(lambda *t: fft_long_conv_transpose(*t, c.s, c.p, c.op, c.d, c.g), x, w, b, gy)
        assert ran[1][0].key[11:15] == (0, 1, c.d, c.s) and ran[2][0].key[11:15] == (0, 1, c.s, c.d), [r[0].key for r in ran]
        au.check(f"transposed case {i} dX against the construction of before", dx, dx0, base[1], F32)
        au.check(f"transposed case {i} dW against the construction of before", dw, dw0, base[2], F32)


# ------------------------------------------------------------------------------------------------ module
@pytest.mark.parametrize("mode", MODES)
def test_module_cache_invalidation_graph_capture_and_state_dict(mode, monkeypatch, ran):
    c = CASES[1]
    monkeypatch.setenv("FFTCONV_LONG_DECIM", mode)
    torch.manual_seed(0)
    ref = torch.nn.Conv1d(c.cin, c.cout, c.k[0], stride=c.s, padding=3, groups=c.g)
    layer = FFTLongConv1d(c.cin, c.cout, c.k[0], padding=3, groups=c.g, stride=c.s)
    layer.load_state_dict(ref.state_dict())
    layer = layer.to(DEV)
    x = au.integers((c.B, c.cin, c.size[0]), torch.Generator().manual_seed(3), F32, DEV)
    calls = []
    real = F_.transform_kernel
    monkeypatch.setattr(F_, "transform_kernel", lambda plan, kernel: calls.append(plan) or real(plan, kernel))
    layer.eval()
    with torch.no_grad():
        y1, y2 = layer(x), layer(x)
    assert len(calls) == 1 and _is_decim(calls[0]) == (mode == "1"), calls       # one transform for two calls
    assert len(ran) == 2 and ran[0][0] is ran[1][0] is calls[0]
    want = ref.double()(x.double().cpu())
    assert y1.shape == want.shape and au.e_max(y1.cpu(), want.detach()) <= 1e-5 and torch.equal(y1, y2)
    gu.same_bits(y1, fft_long_conv(x, layer.weight.detach(), layer.bias.detach(), 3, c.g, stride=c.s), "module against the functional")
    assert len(calls) == 2
    layer.invalidate_kernel_spectrum()
    with torch.no_grad():
        y3 = layer(x)
    assert len(calls) == 3 and torch.equal(y3, y1)

    # a warm call captures and replays
    static_x = x.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        static_y = layer(static_x)
    assert len(calls) == 3
    for seed in (4, 5):
        fresh = au.integers(x.shape, torch.Generator().manual_seed(seed), F32, DEV)
        static_x.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            gu.same_bits(static_y, layer(fresh), f"replay {seed} against the eager call")


# ------------------------------------------------------------------------------------------------ past 2**24 points
def test_a_strided_row_past_the_plain_limit_runs_with_nothing_set(ran):
    """B1 1 -> 1, L = 2**24 + 4096, K 1000, stride 64: the plain row does not fit 2**24 points (NotImplementedError before
    the decimation plan existed); the decimated row has 2**19."""
    c = Case(1, 1, 1, ((1 << 24) + 4096,), (1000,), s=64, note="past-plain")
    au.assert_exact(c, "offset")
    x, w, b = au.inputs(c, "offset", DEV)
    got = fft_long_conv(x, w, b, stride=64)
    torch.cuda.synchronize()
    assert len(ran) == 1 and _is_decim(ran[0][0]) and _points(ran[0][0]) == 1 << 19
    # float64 on the CPU: 2.6e8 products, exact on these integers
    want = F.conv1d(x.double().cpu(), w.double().cpu(), b.double().cpu(), 64).to(DEV)
    assert au.is_whole(want) and got.shape == want.shape == (1, 1, (c.size[0] - 1000) // 64 + 1)
    au.check("2**24 + 4096 samples, stride 64", got, want, au.baseline(c, x, w, b), F32)


def test_a_transposed_layer_past_the_plain_limit_trains_with_nothing_set(ran):
    """B1 1 -> 1, L 262,200, K 1000, stride 64: the forward ran by phases before, its backward needed two plain plans of
    16.8e6 points and raised; both gradients now run on rows of about L + 16 points."""
    c = Case(1, 1, 1, (262_200,), (1000,), s=64, tr=True, note="past-plain-T")
    au.assert_exact(c, "centred")
    x, w, b = au.inputs(c, "centred", DEV)
    lout = (c.size[0] - 1) * 64 + 1000
    assert lout + 999 > F_.LONG_MAX_POINTS
    gy = au.grad_output((1, 1, lout), F32, DEV)
    y, dx, dw, db, _ = _step(lambda *t: fft_long_conv_transpose(*t, 64), x, w, b, gy)
    assert len(ran) == 3 and isinstance(ran[0][0], _native.LongPhasesPlan) and _is_decim(ran[1][0]) and _is_plain(ran[2][0])
    assert _points(ran[1][0]) == _points(ran[2][0]) == 1 << 19
    # float64 autograd on the CPU: 2.6e8 products, exact on these integers
    xr, wr, br = (t.double().cpu().requires_grad_() for t in (x, w, b))
    want_y = F.conv_transpose1d(xr, wr, br, 64)
    want_y.backward(gy.double().cpu())
    base = au.baseline_grads(c, x, w, b, gy)
    for q, got_, want_, base_ in zip(("y", "dX", "dW", "db"), (y, dx, dw, db), (want_y.detach(), xr.grad, wr.grad, br.grad), base):
        assert au.is_whole(want_) and got_.shape == want_.shape, q
        au.check(f"transposed training step past the plain limit, {q}", got_.cpu(), want_, base_.cpu(), F32)
