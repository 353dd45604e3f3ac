"""``fft_long_conv_gated`` on the GPU.  The reference is always the composed line

    postgate * fft_long_conv(pregate * signal, kernel, bias, ...)

built from the public functions on float32 tensors (16-bit cases: the widened tensors, the result rounded once with
``.to(dtype)``), compared with ``guard_util.same_bits``.  The integer-valued placement cases are also compared with torch's
float64 ``conv1d``, exactly.  Small rows: every case is a few thousand samples per row.

Two figures of this feature's test plan do not reach what they are meant to reach, so each is run as stated AND once more where it does:
``FFTCONV_LONG_N=64x64`` holds 4096 points and case 1 needs 4999 (the library refuses it), so N1 = 64 runs as 64x128; case 2
(a padded row of 3600 samples) is one tile of ``fft_conv`` and hands off, so ``CASE2B`` is the same layer on a row of 4800.
Case 2 as stated therefore takes the composed route, whose promise is the line itself in the tensors' own dtype: in 16 bits
that is three roundings, not the one of the float32 composition (5002 of 14400 float16 samples differ from it), so it is
compared with the hand-written line, and ``CASE2B`` carries the rounded-once contract of the fused route."""
import pytest
import torch
import torch.nn.functional as F

from fft_conv_pytorch_amd import FFTLongConv1d, _native, fft_long_conv, fft_long_conv_gated
from fft_conv_pytorch_amd import functional as F_
from tests import accuracy_util as au
from tests import guard_util as gu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F16, BF16, C64 = torch.float32, torch.float16, torch.bfloat16, torch.complex64
KNOBS = ("FFTCONV_LONG_N", "FFTCONV_LONG_WS_MB", "FFTCONV_LONG_DECIM", "FFTCONV_LONG_NLC", "FFTCONV_HALF_IO", "FFTCONV_LONG_WGRAD")
N1S = (64, 128, 256, 512, 1024, 2048, 4096)

# B, cin, cout, groups, L, K, padding, causal
CASE1 = (3, 5, 5, 5, 2500, 2500, 0, True)        # depthwise; the last pair has no partner
CASE2 = (2, 6, 4, 2, 3000, 1801, 300, False)     # as the test plan states it: 3600 samples, hands off to fft_conv
CASE2B = (2, 6, 4, 2, 4000, 2401, 400, False)    # the same layer on the long path: nout 2400 of a row of 4800
CASES = {"case1": CASE1, "case2": CASE2, "case2b": CASE2B}


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    """The knobs are read at plan creation and are not part of a cache key."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    _native.clear_plan_cache()
    yield
    _native.clear_plan_cache()


@pytest.fixture
def launches(monkeypatch):
    """Arguments of every ``fc_long_forward_gated`` call: which optional tensors it was given."""
    seen = []
    real = _native.LongPlan.forward_gated

    def spy(self, *args, **kw):
        seen.append({k[:-4]: v is not None for k, v in kw.items() if k.endswith("_ptr")})
        return real(self, *args, **kw)
    monkeypatch.setattr(_native.LongPlan, "forward_gated", spy)
    return seen


def force(monkeypatch, N1):
    N2 = 128 if N1 == 64 else 64
    monkeypatch.setenv("FFTCONV_LONG_N", f"{N1}x{N2}")
    _native.clear_plan_cache()
    return N1, N2


def kw_of(case):
    return dict(padding=case[6], groups=case[3], causal=case[7])


def out_len(case):
    B, cin, cout, g, L, K, padding, causal = case
    return L if causal else L + 2 * padding - K + 1


def tensors(case, dtype=F32, bias=True, seed=0, pre=True, post=True):
    """(x, w, b, pregate, postgate): normal samples, the taps scaled so that y is of order one."""
    B, cin, cout, g, L, K, padding, causal = case
    gen = torch.Generator().manual_seed(seed + L + 3 * K + B)
    rnd = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    x, w = rnd(B, cin, L), rnd(cout, cin // g, K) / (K * cin // g) ** 0.5
    b = rnd(cout) if bias else None
    p, q = rnd(B, cin, L), rnd(B, cout, out_len(case))
    return tuple(None if t is None else t.to(DEV).to(dtype) for t in (x, w, b, p if pre else None, q if post else None))


def composed(x, w, b, pre, post, **kw):
    out = fft_long_conv(x if pre is None else pre * x, w, b, **kw)
    return out if post is None else post * out


def wide(ts):
    return [None if t is None else t.detach().float() for t in ts]


def reference(ts, **kw):
    """The composed line on the float32 (widened) tensors, rounded once."""
    with torch.no_grad():
        return composed(*wide(ts), **kw).to(ts[0].dtype)


def route_of(case, dtype=F32, **more):
    B, cin, cout, g, L, K, padding, causal = case
    return F_._long_gated_route((B, cin, L), (cout, cin // g, K), padding=padding, groups=g, causal=causal, dtype=dtype, **more)


def check_forward(case, ts, what, fused=True, launches=None):
    kw = kw_of(case)
    assert route_of(case, ts[0].dtype) == ("fused" if fused else "composed"), what
    with torch.no_grad():
        got = fft_long_conv_gated(ts[0], ts[1], ts[2], pregate=ts[3], postgate=ts[4], **kw)
    assert got.dtype == ts[0].dtype and got.is_contiguous() and tuple(got.shape) == (case[0], case[2], out_len(case))
    if fused:
        gu.same_bits(got, reference(ts, **kw), what)
    else:       # the composed route promises the line itself, in the tensors' own dtype (16-bit: its three roundings)
        with torch.no_grad():
            gu.same_bits(got, composed(*ts, **kw), what)
    if launches is not None:
        assert bool(launches) == fused, (what, launches)
    return got


# ------------------------------------------------------------------------------------------------ 1. every N1
@pytest.mark.parametrize("N1", N1S)
def test_every_column_build(N1, monkeypatch, launches):
    N1, N2 = force(monkeypatch, N1)
    ts = tensors(CASE1)
    check_forward(CASE1, ts, f"case 1 at {N1}x{N2}", launches=launches)
    plan = F_._long_forward_plan(ts[0], ts[1].shape, True, 2499, 0, True, 5, 1, 1, 0, "plain")[0]
    assert (plan.info["N1"], plan.info["N2"]) == (N1, N2)
    assert launches == [dict(pregate=True, gate=True, y2=False, gate2=False)]


def test_64_x_64_does_not_hold_case_1(monkeypatch):
    """Why N1 = 64 runs as 64 x 128 above."""
    monkeypatch.setenv("FFTCONV_LONG_N", "64x64")
    _native.clear_plan_cache()
    ts = tensors(CASE1)
    with pytest.raises(ValueError, match="holds 4096 points but the row needs 4999"):
        fft_long_conv_gated(*ts[:3], pregate=ts[3], postgate=ts[4], **kw_of(CASE1))


# ------------------------------------------------------------------------------------------------ 2. grouped, shorter result
def test_grouped_result_shorter_than_the_row(launches):
    check_forward(CASE2B, tensors(CASE2B), "case 2b", launches=launches)


def test_case_2_as_stated_hands_off(launches):
    check_forward(CASE2, tensors(CASE2), "case 2", fused=False, launches=launches)


# ------------------------------------------------------------------------------------------------ 3. placement
def _truth(case, x, w, b, pre, post):
    """float64 conv1d of the integer tensors on the CPU: exact."""
    B, cin, cout, g, L, K, padding, causal = case
    x, w, b, pre, post = (None if t is None else t.double().cpu() for t in (x, w, b, pre, post))
    z = x if pre is None else pre * x
    if causal:
        c = F.conv1d(F.pad(z, (K - 1, 0)), w.flip(-1), b, groups=g)
    else:
        c = F.conv1d(z, w, b, padding=padding, groups=g)
    return c if post is None else post * c


@pytest.mark.parametrize("name", ["case1", "case2b"])
@pytest.mark.parametrize("which", ["pregate", "postgate"])
def test_a_one_hot_gate_lands_on_its_sample(name, which, launches):
    """x all ones, integer taps and bias (accuracy_util.integers), a gate that is one at a single (b, c, t) and zero
    elsewhere; the truth is torch's float64 conv1d, which is exact on these integers.  A float32 transform is not exact,
    so "equal to the truth" is asked in the two forms that are: where the truth is zero because a gate is (every sample but
    one of a one-hot postgate) the result is zero, and everywhere the result rounds to the truth's integer; and the error
    itself stays within the bound of a float32 transform (below), far from the whole units that a gate read one sample off
    would move a sample by."""
    case = CASES[name]
    B, cin, cout, g, L, K, padding, causal = case
    gen = torch.Generator().manual_seed(11)
    w = au.integers((cout, cin // g, K), gen, F32, DEV)
    b = au.integers((cout,), gen, F32, DEV)
    x = torch.ones(B, cin, L, device=DEV)
    nout = out_len(case)
    for spot in ((B - 1, cin - 1, L - 1), (0, 0, 0), (B - 1, 1, 1237)):
        pre = post = None
        if which == "pregate":
            pre = torch.zeros(B, cin, L, device=DEV)
            pre[spot] = 1.0
        else:
            spot = (spot[0], min(spot[1], cout - 1), min(spot[2], nout - 1))
            post = torch.zeros(B, cout, nout, device=DEV)
            post[spot] = 1.0
        ts = (x, w, b, pre, post)
        what = f"{name} {which} at {spot}"
        got = check_forward(case, ts, what, launches=launches).double().cpu()
        want = _truth(case, *ts)
        assert au.is_whole(want) and want.abs().max() < 2 ** 16
        # the bound of a float32 FFT convolution on one output: eps * log2(N) * |z|_2 * |w|_2 over the group's rows (z the
        # gated row; N = 8192 points here), and one more eps of the sum for the bias add; a postgate of at most one keeps it
        z = x if pre is None else pre * x
        z2 = z.double().square().view(B, g, -1).sum(-1).max().sqrt().item()
        w2 = w.double().square().view(cout, -1).sum(-1).max().sqrt().item()
        bound = 2.0 ** -23 * (13 * z2 * w2 + want.abs().max().item() + 8)
        err = (got - want).abs().max().item()
        print(f"    {what}: e_max {au.e_max(got, want):.2e}, max error {err:.2e} within {bound:.2e}")
        assert err <= bound, f"{what}: error {err:.3e} above the float32 transform's bound {bound:.3e}"
        assert torch.equal(got.round(), want), f"{what}: {int((got.round() != want).sum())} samples are not the truth's integer"
        if post is not None:
            assert int((got != 0).sum()) <= 1 and int((want != 0).sum()) <= 1, what


# ------------------------------------------------------------------------------------------------ 4. combinations and edges
EDGES = {
    "pregate only": (CASE1, dict(post=False)),
    "postgate only": (CASE1, dict(pre=False)),
    "batch of one": ((1,) + CASE1[1:], {}),
    "K 5000 > L 2500": ((3, 5, 5, 5, 2500, 5000, 0, True), {}),
    "no bias": (CASE2B, dict(bias=False)),
    "no bias, pregate only": (CASE1, dict(bias=False, post=False)),
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_gate_combinations_and_edges(name, launches):
    case, opts = EDGES[name]
    check_forward(case, tensors(case, **opts), name, launches=launches)
    assert launches[0]["pregate"] == opts.get("pre", True) and launches[0]["gate"] == opts.get("post", True)


def test_gates_that_do_not_lie_contiguous_are_copied(launches):
    ts = list(tensors(CASE1))
    ts[3] = ts[3].transpose(0, 2).contiguous().transpose(0, 2)        # the same values under other strides
    big = torch.zeros(3, 5, 5000, device=DEV)
    big[..., ::2] = tensors(CASE1)[4]
    ts[4] = big[..., ::2]
    assert not ts[3].is_contiguous() and not ts[4].is_contiguous()
    check_forward(CASE1, ts, "strided gates", launches=launches)


# ------------------------------------------------------------------------------------------------ 5. slabs
def test_later_slabs_start_at_their_own_pairs(monkeypatch, launches):
    monkeypatch.setenv("FFTCONV_LONG_WS_MB", "1")
    _native.clear_plan_cache()
    case = (7,) + CASE1[1:]
    ts = tensors(case)
    plan = F_._long_forward_plan(ts[0], ts[1].shape, True, 2499, 0, True, 5, 1, 1, 0, "plain")[0]
    assert plan.info["slabs"] >= 3 and plan.info["slab_pairs"] < 4
    check_forward(case, ts, "B7 in slabs", launches=launches)


# ------------------------------------------------------------------------------------------------ 6. 16-bit
@pytest.mark.parametrize("N1", (64, 1024))
@pytest.mark.parametrize("dtype", (F16, BF16), ids=("f16", "bf16"))
@pytest.mark.parametrize("name", ["case1", "case2", "case2b"])
def test_16_bit(name, dtype, N1, monkeypatch, launches):
    N1, N2 = force(monkeypatch, N1) if name != "case2" else (0, 0)      # (a row that hands off takes no long plan)
    check_forward(CASES[name], tensors(CASES[name], dtype), f"{name} {dtype} at {N1}x{N2}", fused=name != "case2",
                  launches=launches)


# ------------------------------------------------------------------------------------------------ 7. gradients
NAMES = ("dX", "dW", "db", "dPre", "dPost")


def grads_of(fn, ts, gy, need):
    leaves = [None if t is None else t.detach().clone().requires_grad_(n) for t, n in zip(ts, need)]
    y = fn(*leaves)
    wanted = [t for t, n in zip(leaves, need) if t is not None and n]
    got = iter(torch.autograd.grad(y, wanted, gy, retain_graph=True))      # (a test looks at the saved tensors afterwards)
    return y, [next(got) if t is not None and n else None for t, n in zip(leaves, need)]


def check_grads(case, ts, what, need=(True,) * 5, fused=True):
    kw = kw_of(case)
    dtype = ts[0].dtype
    gy = torch.randn((case[0], case[2], out_len(case)), generator=torch.Generator().manual_seed(5)).to(DEV).to(dtype)
    y, got = grads_of(lambda x, w, b, p, q: fft_long_conv_gated(x, w, b, pregate=p, postgate=q, **kw), ts, gy, need)
    _, want = grads_of(lambda x, w, b, p, q: composed(x, w, b, p, q, **kw), wide(ts), gy.float(), need)
    assert (type(y.grad_fn).__name__ == "FFTLongConvGatedFunctionBackward") == fused
    for name, a, r, t in zip(NAMES, got, want, ts):
        assert (a is None) == (r is None), (what, name)
        if a is not None:
            assert a.dtype == dtype and a.shape == t.shape
            gu.same_bits(a, r.to(dtype), f"{what}: {name}")
    return y


@pytest.mark.parametrize("name", ["case1", "case2", "case2b"])
def test_all_five_gradients(name, launches):
    check_grads(CASES[name], tensors(CASES[name]), name, fused=name != "case2")
    if name != "case2":
        assert launches == TWO_LAUNCHES


@pytest.mark.parametrize("N1", (64, 1024))
@pytest.mark.parametrize("dtype", (F16, BF16), ids=("f16", "bf16"))
@pytest.mark.parametrize("name", ["case1", "case2b"])
def test_all_five_gradients_16_bit(name, dtype, N1, monkeypatch):
    N1, N2 = force(monkeypatch, N1)
    check_grads(CASES[name], tensors(CASES[name], dtype), f"{name} {dtype} at {N1}x{N2}")


TWO_LAUNCHES = [dict(pregate=True, gate=True, y2=True, gate2=False),       # forward: y and c from one launch
                dict(pregate=True, gate=True, y2=True, gate2=True)]        # backward: dX and d(pregate) from one launch


@pytest.mark.parametrize("dtype", (F32, BF16), ids=("f32", "bf16"))
@pytest.mark.parametrize("N1", N1S)
def test_all_five_gradients_every_column_build(N1, dtype, monkeypatch, launches):
    """Every N1 is a compiled build of its own: the second store of the gated inverse pass (c in the forward, float32 for
    16-bit tensors; d(pregate) through gate2 in the backward) and the gated first pass of the dX run, at each of them."""
    N1, N2 = force(monkeypatch, N1)
    check_grads(CASE1, tensors(CASE1, dtype), f"case 1 {dtype} at {N1}x{N2}")
    assert launches == TWO_LAUNCHES
    for pl in (2499, 0):      # the forward plan and the dX plan (pad_left K - 1 and 0) both took the forced geometry
        info = F_._long_plan(tensors(CASE1)[0], 5, 5, 2500, pl, 2499 - pl, pl > 0, 2500, pl > 0).info
        assert (info["N1"], info["N2"]) == (N1, N2)


SUBSETS = {
    "kernel only": (False, True, False, False, False),
    "gates only": (False, False, False, True, True),
    "signal only": (True, False, False, False, False),
    "pregate only": (False, False, False, True, False),
    "bias only": (False, False, True, False, False),
    "postgate frozen": (True, True, True, True, False),
}


@pytest.mark.parametrize("dtype", (F32, BF16), ids=("f32", "bf16"))
@pytest.mark.parametrize("name", sorted(SUBSETS))
def test_subsets_of_requires_grad(name, dtype, launches):
    need = SUBSETS[name]
    ts = tensors(CASE1, dtype)
    y = check_grads(CASE1, ts, f"{name} {dtype}", need)
    saved = [t for t in y.grad_fn.saved_tensors if t is not None]
    # never pregate * x nor y; c (the only saved tensor of y's shape besides postgate) only where postgate needs a gradient
    assert len(saved) == 5 + int(need[4]), [tuple(t.shape) for t in saved]
    assert launches[0]["y2"] == need[4]
    if len(launches) > 1:
        assert launches[1]["y2"] == (need[0] and need[3])      # one store where one of dX, d(pregate) is wanted
    assert (len(launches) > 1) == (need[0] or need[3])


def test_gradients_without_one_gate():
    for opts in (dict(pre=False), dict(post=False), dict(pre=False, bias=False)):
        check_grads(CASE2B, tensors(CASE2B, **opts), f"case 2b {opts}")


def test_double_backward_goes_through_the_composed_line():
    """A backward that records a graph differentiates the composed line: d/d(postgate) of sum(dX) through it matches."""
    ts = tensors(CASE1)
    kw = kw_of(CASE1)

    def second(fn):
        x, w, b, p, q = (t.detach().clone().requires_grad_() for t in ts)
        y = fn(x, w, b, p, q)
        (dx,) = torch.autograd.grad(y.sum(), x, create_graph=True)
        return torch.autograd.grad(dx.square().sum(), p)[0]
    got = second(lambda x, w, b, p, q: fft_long_conv_gated(x, w, b, pregate=p, postgate=q, **kw))
    want = second(lambda x, w, b, p, q: composed(x, w, b, p, q, **kw))
    gu.same_bits(got, want, "second derivative")


# ------------------------------------------------------------------------------------------------ 8. guard bands and poison
def test_guard_bands_and_poison():
    from tests import test_gpu_memory_discipline as tm
    kw = kw_of(CASE1)
    ts = tensors(CASE1)
    gy = torch.randn((3, 5, 2500), generator=torch.Generator().manual_seed(5)).to(DEV)

    def step(x, w, b, p, q):
        leaves = [t.detach().requires_grad_() for t in (x, w, b, p, q)]
        y = fft_long_conv_gated(*leaves[:3], pregate=leaves[3], postgate=leaves[4], **kw)
        return (y.detach(),) + torch.autograd.grad(y, leaves, gy)
    first = tm._runs(step, ts, "gated training step")
    gu.same_bits(first[0], reference(ts, **kw), "guarded forward")
    (y0,) = tm._runs(lambda x, w, b, p, q: fft_long_conv_gated(x, w, b, pregate=p, postgate=q, **kw), ts, "gated forward",
                     patterns=tm.RUNS[:2], offset=1)
    gu.same_bits(y0, first[0], "odd start against the aligned run")


# ------------------------------------------------------------------------------------------------ 9. composed inputs
def _cl(t):
    return t.transpose(1, 2).contiguous().transpose(1, 2)


COMPOSED = {
    "complex64": (dict(dtype=C64), {}),
    "stride 2": ({}, dict(stride=2)),
    "dilation 2": ({}, dict(dilation=2)),
    "reflect": ({}, dict(padding=100, padding_mode="reflect")),
    "channels_last=True": ({}, dict(channels_last=True)),
    "channels-last signal": (dict(nlc=True), {}),
    "L 1000": (dict(L=1000), {}),
}


@pytest.mark.parametrize("name", sorted(COMPOSED))
def test_composed_inputs(name, launches):
    how, kw = COMPOSED[name]
    B, C, L, K = 2, 4, how.get("L", 3000), 1500 if "L" not in how else 400
    dtype = how.get("dtype", F32)
    kw = dict(dict(padding=0, groups=C, causal="padding" not in kw), **kw)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(B, C, L, generator=gen).to(DEV).to(dtype)
    w = (torch.randn(C, 1, K, generator=gen) / K ** 0.5).to(DEV).to(dtype)
    b = torch.randn(C, generator=gen).to(DEV).to(dtype)
    if dtype == C64:
        x, w, b = x + 1j * x.flip(-1), w * (1 - 0.5j), b * (2 + 1j)
    if how.get("nlc"):
        x = _cl(x)
    with torch.no_grad():
        plain = fft_long_conv(x, w, b, **kw)
        pre = torch.randn(x.shape, generator=gen).to(DEV).to(dtype)
        post = torch.randn(plain.shape, generator=gen).to(DEV).to(dtype)
        got = fft_long_conv_gated(x, w, b, pregate=pre, postgate=post, **kw)
        want = post * fft_long_conv(pre * x, w, b, **kw)
    layout = F_._long_layout(x)
    assert F_._long_gated_route(x.shape, w.shape, kw.get("stride", 1), kw["padding"], kw.get("dilation", 1), C, kw["causal"],
                                kw.get("padding_mode", "constant"), dtype, layout, kw.get("channels_last", False)) == "composed"
    assert not launches
    assert got.stride() == want.stride()
    gu.same_bits(got, want, name)
    # and differentiable as torch differentiates the line
    ts = [t.detach().clone().requires_grad_() for t in (x, w, b, pre, post)]
    y = fft_long_conv_gated(ts[0], ts[1], ts[2], pregate=ts[3], postgate=ts[4], **kw)
    grads = torch.autograd.grad(y, ts, torch.ones_like(y))
    assert all(g.shape == t.shape for g, t in zip(grads, ts))


def test_no_gates_is_fft_long_conv_bit_for_bit(launches):
    x, w, b, _, _ = tensors(CASE1)
    gu.same_bits(fft_long_conv_gated(x, w, b, **kw_of(CASE1)), fft_long_conv(x, w, b, **kw_of(CASE1)), "no gates")
    assert not launches


def test_library_refuses_the_plans_it_does_not_take():
    """Complex plans, a non-default fc_long_ext, phases and decimation plans: FC_ERR_UNSUPPORTED with a sentence, and not
    one launch (the output keeps its NaNs)."""
    x = torch.randn(2, 4, 5000, device=DEV)
    plans = {
        "real plans only": F_._long_plan(x.to(C64), 4, 4, 100, 99, 0, True, 5000, False),
        "default fc_long_ext only": F_._long_plan(x, 4, 4, 100, 50, 50, False, 0, False, pad_mode=1),
        "neither a phases plan nor a decimation plan": F_._long_decim_plan(x, 4, 4, 100, 2, 0, 0, 0, False, False),
    }
    plans["default fc_long_ext only "] = F_._long_plan(x, 4, 4, 100, 0, 0, False, 0, False, out_step=2)
    plans["neither a phases plan nor a decimation plan "] = F_._long_phases_plan(x, 4, 4, 100, 2, 0, 0, False)
    for text, plan in plans.items():
        out = torch.full((2, 4, 16384), float("nan"), device=DEV)
        ws = F_.new_workspace(plan, x.device)
        spec = torch.zeros(plan.spectrum_bytes // 4, device=DEV)
        gate = torch.ones_like(out)
        with pytest.raises(NotImplementedError, match=text.strip()):
            plan.forward_gated(x.data_ptr(), spec.data_ptr(), None, out.data_ptr(), ws.data_ptr(),
                               torch.cuda.current_stream().cuda_stream, gate_ptr=gate.data_ptr())
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), text


# ------------------------------------------------------------------------------------------------ 10. module and capture
def test_module_with_gates_reuses_its_spectrum(monkeypatch, launches):
    torch.manual_seed(0)
    layer = FFTLongConv1d(5, 5, 2500, groups=5, causal=True).to(DEV).eval()
    x, _, _, pre, post = tensors(CASE1)
    calls = []
    real = F_.transform_kernel
    monkeypatch.setattr(F_, "transform_kernel", lambda plan, kernel: calls.append(1) or real(plan, kernel))
    with torch.no_grad():
        plain = layer(x)
        y1, y2 = layer(x, pre, post), layer(x, pregate=pre, postgate=post)
        want = composed(x, layer.weight, layer.bias, pre, post, **kw_of(CASE1))
    assert len(calls) == 2 and len(launches) == 2          # one transform by the module, one by the reference line
    gu.same_bits(y1, want, "module with gates")
    gu.same_bits(y2, want, "module with gates, again")
    gu.same_bits(layer(x).detach(), plain, "module without gates")


def test_warm_fused_call_is_capturable_and_replays_bit_for_bit():
    x, w, b, pre, post = tensors(CASE1)
    kw = kw_of(CASE1)
    with torch.no_grad():
        fft_long_conv_gated(x, w, b, pregate=pre, postgate=post, **kw)       # warm: plan and device tables exist
        torch.cuda.synchronize()
        sx, sp, sq = x.clone(), pre.clone(), post.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            sy = fft_long_conv_gated(sx, w, b, pregate=sp, postgate=sq, **kw)
        for seed in (1, 2):
            fx, _, _, fp, fq = tensors(CASE1, seed=seed)
            sx.copy_(fx), sp.copy_(fp), sq.copy_(fq)
            graph.replay()
            torch.cuda.synchronize()
            gu.same_bits(sy, fft_long_conv_gated(fx, w, b, pregate=fp, postgate=fq, **kw), f"replay {seed}")
            gu.same_bits(sy, reference((fx, w, b, fp, fq), **kw), f"replay {seed} against the composed line")


# ------------------------------------------------------------------------------------------------ 11. memory
def _added_peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def test_no_product_tensor_exists():
    """Derived, not measured: a fused no-grad forward allocates y, the workspace and the spectrum (and the float32 bias,
    rounded up to an allocator block); the composed line also holds pregate * x across the call (and the ungated result
    while it multiplies)."""
    case = (4, 8, 8, 8, 20000, 20000, 0, True)
    x, w, b, pre, post = tensors(case)
    kw = kw_of(case)

    def fused():
        with torch.no_grad():
            return fft_long_conv_gated(x, w, b, pregate=pre, postgate=post, **kw)

    def line():
        with torch.no_grad():
            return composed(x, w, b, pre, post, **kw)
    want = fused()                                        # warm: plan and tables
    gu.same_bits(line(), want, "composed line")
    plan = F_._long_forward_plan(x, w.shape, True, 19999, 0, True, 8, 1, 1, 0, "plain")[0]
    a, c = _added_peak(fused), _added_peak(line)
    nbytes = x.numel() * x.element_size()
    bound = want.numel() * want.element_size() + plan.workspace_bytes + plan.spectrum_bytes + 4 * 512
    print(f"added peak: fused {a / 2**20:.2f} MiB, composed {c / 2**20:.2f} MiB, signal {nbytes / 2**20:.2f} MiB, "
          f"y + workspace + spectrum {bound / 2**20:.2f} MiB")
    assert a <= bound
    assert a <= c - nbytes
