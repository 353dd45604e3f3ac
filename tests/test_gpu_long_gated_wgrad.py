"""The weight-gradient plan with the gates of ``fft_long_conv_gated`` inside its two column reads, on the GPU
(``fc_long_wgrad_gated``, ``LongWgradPlan.run_gated``, ``F_._long_wgrad_run(..., pregate=, postgate=)``, and
``FFTLongConvGatedFunction.backward`` under FFTCONV_LONG_WGRAD=1).

"Reference dW" is ``F_._long_wgrad_run(x.float() * pre.float(), dy.float() * post.float(), ..., out_dtype=dtype)``: the same
plan on the float32 products torch forms, which is what the parent computes under the switch.  "The line" is autograd
through ``postgate * fft_long_conv(pregate * x, ...)`` on the widened float32 tensors under the same switch, rounded once.
Comparisons are ``guard_util.same_bits``.  Shapes are those of tests/test_gpu_long_gated.py: rows only just past the
4096-point hand-off.

The one-hot tests state their truth as a single product of small integers, which is exact in float32.  The transform that
computes it is not: three float32 FFT passes lie between the gate and dW, so the result is the truth plus the rounding
error of those passes (measured on an MI355X: 1.0e-5 to 1.8e-4 over the 120 placements below, on values up to 512, against
a bound of 1e-2 to 7e-2), never the truth's bits -- a comparison of the raw result with ``==`` cannot pass, for the reference dW (whose bits the
result must have, and has) no more than for the result.  "Equal to the truth" is therefore asked in the forms
that are exact, as tests/test_gpu_long_gated.py does for the forward: every row of dW whose gated operand is zero is zero
(``==``), every element rounds to the truth's integer (``==``; a gate read one sample, one channel, one batch item or one
slab off moves elements by whole units), and the error stays inside the bound of three float32 transforms written out at
``_transform_bound``.  On top of that the result has the bits of the reference dW.  16-bit operands are read as 16-bit
there and dW is asked for in float32, so that no store rounding lies between the result and the integer."""
import pytest
import torch

from fft_conv_pytorch_amd import _native, autograd, fft_long_conv_gated
from fft_conv_pytorch_amd import functional as F_
from tests import accuracy_util as au
from tests import guard_util as gu
from tests import test_gpu_long_gated as tg

pytestmark = pytest.mark.gpu
DEV = tg.DEV
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
CASE1, CASE2B = tg.CASE1, tg.CASE2B
LONGER = (3, 5, 5, 5, 3000, 5000, 0, True)      # a causal filter longer than the row
CASES = {"case1": CASE1, "case2b": CASE2B, "K 5000 > L 3000": LONGER}


def _clear():
    _native.clear_plan_cache()
    F_._REFUSED_HALF.clear()
    autograd._BWD_PLANS.clear()


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    """The knobs are read at plan creation and are not part of a cache key."""
    for k in tg.KNOBS:
        monkeypatch.delenv(k, raising=False)
    _clear()
    yield
    _clear()


@pytest.fixture
def gated_runs(monkeypatch):
    """Every ``LongWgradPlan.run_gated``: which gates it was given and the dtype codes of x, dY and dW."""
    seen = []
    real = _native.LongWgradPlan.run_gated

    def spy(plan, *args):
        seen.append(dict(pregate=args[1] is not None, postgate=args[3] is not None, codes=tuple(args[7:10])))
        return real(plan, *args)
    monkeypatch.setattr(_native.LongWgradPlan, "run_gated", spy)
    return seen


def pads(case):
    B, cin, cout, g, L, K, padding, causal = case
    return (K - 1, 0) if causal else (padding, padding)


def key_of(case, mode=0, stride=1, dilation=1, nout=None):
    B, cin, cout, g, L, K, padding, causal = case
    pl, pr = pads(case)
    return F_._long_wgrad_key(B, cin, cout, g, L, K, pl, pr, tg.out_len(case) if nout is None else nout, causal, mode, stride,
                              dilation)


def wshape(case):
    return (case[2], case[1] // case[3], case[5])


def operands(case, dtype=F32, seed=0):
    """(x, pregate, dY, postgate): normal samples in ``dtype``."""
    x, _, _, pre, post = tg.tensors(case, dtype, seed=seed)
    gy = torch.randn(post.shape, generator=torch.Generator().manual_seed(5 + seed)).to(DEV).to(dtype)
    return x, pre, gy, post


def run(case, x, pre, dy, post, dtype, key=None):
    return F_._long_wgrad_run(x, dy, wshape(case), key_of(case) if key is None else key, dtype, pregate=pre, postgate=post)


def reference(case, x, pre, dy, post, dtype, key=None):
    """The plan on the float32 products torch forms (an absent gate: the widened tensor)."""
    z = x.float() if pre is None else x.float() * pre.float()
    q = dy.float() if post is None else dy.float() * post.float()
    return F_._long_wgrad_run(z, q, wshape(case), key_of(case) if key is None else key, dtype)


def plan_info(case, key=None):
    plan = _native.lookup_plan(0, ("long_wgrad",) + (key_of(case) if key is None else key))
    assert plan is not None, "no weight-gradient plan was created"
    return plan.info


def one_pair_per_slab(monkeypatch, case, points=8192):
    """FFTCONV_LONG_WS_MB with room for W2 and the W1 rows of one pair, not of two (tests/test_gpu_long_wgrad.py test_6)."""
    rows = case[2] * case[1] // case[3]
    monkeypatch.setenv("FFTCONV_LONG_WS_MB", str(-(-((rows + case[1] + case[2]) * points * 8) // (1 << 20))))
    _clear()


# ------------------------------------------------------------------------------------------------ 1. the call alone
@pytest.mark.parametrize("name", ["case1", "case2b"])
def test_the_call_alone(name, gated_runs):
    case = CASES[name]
    x, pre, dy, post = operands(case)
    for what, p, q in (("both gates", pre, post), ("pregate only", pre, None), ("postgate only", None, post)):
        gu.same_bits(run(case, x, p, dy, q, F32), reference(case, x, p, dy, q, F32), f"{name}, {what}")
    assert [(r["pregate"], r["postgate"]) for r in gated_runs] == [(True, True), (True, False), (False, True)]
    gu.same_bits(run(case, x, None, dy, None, F32), F_._long_wgrad_run(x, dy, wshape(case), key_of(case), F32), f"{name}, no gate")
    assert len(gated_runs) == 3                              # without a gate the call is the one it was
    info = plan_info(case)
    assert info["N1"] * info["N2"] == 8192 and info["slabs"] == 1


# ------------------------------------------------------------------------------------------------ 2. the step
def step_under_the_switch(case, ts, what, gated_runs, monkeypatch, need=(True,) * 5):
    """All the gradients asked for equal the line's under FFTCONV_LONG_WGRAD=1; dW came from ONE ``run_gated``."""
    monkeypatch.setenv("FFTCONV_LONG_WGRAD", "1")
    del gated_runs[:]
    tg.check_grads(case, ts, what, need)
    if need[1]:
        code = F_._DTYPE_CODES[ts[0].dtype]
        assert gated_runs == [dict(pregate=ts[3] is not None, postgate=ts[4] is not None, codes=(code,) * 3)], (what, gated_runs)
    else:
        assert gated_runs == [], what


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_step(name, gated_runs, monkeypatch):
    case = CASES[name]
    B, cin, cout, g, L, K, padding, causal = case
    assert F_._long_gated_dw_route((B, cin, L), wshape(case), padding, g, causal) == "products"
    ts = tg.tensors(case)
    # the switch unset: no gated plan, and dW is _long_grad_weight on the products torch forms
    tg.check_grads(case, ts, f"{name}, switch unset")
    assert gated_runs == []
    x, w, b, pre, post = ts
    gy = torch.randn((B, cout, tg.out_len(case)), generator=torch.Generator().manual_seed(5)).to(DEV)
    kw = tg.kw_of(case)
    _, got = tg.grads_of(lambda x, w, b, p, q: fft_long_conv_gated(x, w, b, pregate=p, postgate=q, **kw), ts, gy, (True,) * 5)
    pl, pr = pads(case)
    with torch.no_grad():
        want = autograd._long_grad_weight(pre * x, post * gy, w, g, pl, pr, causal, 0, 1, 1, False)
    gu.same_bits(got[1], want, f"{name}, switch unset: dW against _long_grad_weight on the products")
    assert gated_runs == []
    # the switch set
    monkeypatch.setenv("FFTCONV_LONG_WGRAD", "1")
    assert F_._long_gated_dw_route((B, cin, L), wshape(case), padding, g, causal) == "gated-plan"
    step_under_the_switch(case, ts, f"{name}, switch set", gated_runs, monkeypatch)
    _, got = tg.grads_of(lambda x, w, b, p, q: fft_long_conv_gated(x, w, b, pregate=p, postgate=q, **kw), ts, gy, (True,) * 5)
    gu.same_bits(got[1], reference(case, x, pre, gy, post, F32), f"{name}, switch set: dW against the reference dW")


SUBSETS = {
    "kernel only": ((False, True, False, False, False), {}),
    "kernel and bias": ((False, True, True, False, False), {}),
    "postgate frozen": ((True, True, True, True, False), {}),
    "no pregate": ((True,) * 5, dict(pre=False)),
    "no postgate": ((True,) * 5, dict(post=False)),
}


@pytest.mark.parametrize("dtype", (F32, BF16), ids=("f32", "bf16"))
@pytest.mark.parametrize("name", sorted(SUBSETS))
def test_subsets_of_requires_grad_and_absent_gates(name, dtype, gated_runs, monkeypatch):
    need, opts = SUBSETS[name]
    step_under_the_switch(CASE1, tg.tensors(CASE1, dtype, **opts), f"{name} {dtype}", gated_runs, monkeypatch, need)


# ------------------------------------------------------------------------------------------------ 3. every column build
@pytest.mark.parametrize("dtype", (F32, BF16), ids=("f32", "bf16"))
@pytest.mark.parametrize("N1", tg.N1S)
def test_every_column_build(N1, dtype, monkeypatch, gated_runs):
    """Every N1 is a compiled build of the gated column kernel, which here runs with the words of the dY side too."""
    N1, N2 = tg.force(monkeypatch, N1)
    x, pre, dy, post = operands(CASE1, dtype)
    gu.same_bits(run(CASE1, x, pre, dy, post, dtype), reference(CASE1, x, pre, dy, post, dtype), f"case 1 {dtype} at {N1}x{N2}")
    info = plan_info(CASE1)
    assert (info["N1"], info["N2"]) == (N1, N2)
    assert len(gated_runs) == 1 and gated_runs[0]["codes"] == (F_._DTYPE_CODES[dtype],) * 3


# ------------------------------------------------------------------------------------------------ 4. 16-bit
@pytest.mark.parametrize("N1", (64, 1024))
@pytest.mark.parametrize("dtype", (F16, BF16), ids=("f16", "bf16"))
@pytest.mark.parametrize("name", ["case1", "case2b"])
def test_16_bit(name, dtype, N1, monkeypatch, gated_runs):
    N1, N2 = tg.force(monkeypatch, N1)
    case = CASES[name]
    x, pre, dy, post = operands(case, dtype)
    what = f"{name} {dtype} at {N1}x{N2}"
    gu.same_bits(run(case, x, pre, dy, post, dtype), reference(case, x, pre, dy, post, dtype), what)
    assert gated_runs[0]["codes"] == (F_._DTYPE_CODES[dtype],) * 3
    step_under_the_switch(case, tg.tensors(case, dtype), what, gated_runs, monkeypatch)


# ------------------------------------------------------------------------------------------------ 5. one-hot gates
def _ints(shape, seed, dtype):
    return au.integers(shape, torch.Generator().manual_seed(seed), F32, DEV).to(dtype)      # |v| <= 8: exact in 16 bits


def _taps(case):
    """k' of the header's formula for every element k of a row of dW: k, or K - 1 - k where the forward flips (causal)."""
    K = case[5]
    k = torch.arange(K, device=DEV)
    return K - 1 - k if case[7] else k


def _truth_one_hot_postgate(case, x, pre, dy, b, o, t0):
    """dW[o, i, k] = dY[b, o, t0] * pregate[b, i, s] * x[b, i, s], s = t0 + k' - pad_left, i in o's group; zero off the row
    and for every other o'."""
    B, cin, cout, g, L, K, padding, causal = case
    cig, cog = cin // g, cout // g
    s = t0 + _taps(case) - pads(case)[0]
    ok = (s >= 0) & (s < L)
    rows = (x.float() * pre.float())[b, (o // cog) * cig:(o // cog + 1) * cig]
    truth = torch.zeros(wshape(case), device=DEV)
    truth[o] = dy[b, o, t0].float() * rows[:, s.clamp(0, L - 1)] * ok
    return truth


def _truth_one_hot_pregate(case, x, dy, post, b, i, s0):
    """dW[o, i, k] = x[b, i, s0] * postgate[b, o, t] * dY[b, o, t], t = s0 - k' + pad_left, o in i's group; zero off the row
    and for every other i'."""
    B, cin, cout, g, L, K, padding, causal = case
    cig, cog = cin // g, cout // g
    nout = tg.out_len(case)
    t = s0 - _taps(case) + pads(case)[0]
    ok = (t >= 0) & (t < nout)
    grp = i // cig
    rows = (dy.float() * post.float())[b, grp * cog:(grp + 1) * cog]
    truth = torch.zeros(wshape(case), device=DEV)
    truth[grp * cog:(grp + 1) * cog, i % cig] = x[b, i, s0].float() * rows[:, t.clamp(0, nout - 1)] * ok
    return truth


def _transform_bound(dense, hot, b, points, want):
    """The error of dW[o, i, k] = sum over the pairs of the correlation of two rows, computed by float32 transforms: x and
    dY each go through one forward transform and the product through one inverse, and each of the three is off by at most
    eps * log2(N) relative to the 2-norm of what it transforms, so by Parseval an element of the correlation of rows z and
    q is off by at most 3 * eps * log2(N) * |z|_2 * |q|_2.  A row of the transform packs the two items of a batch pair, so
    |z|_2 is taken over both; the one-hot side has the norm of its one sample; every other pair has a zero operand and adds
    nothing.  One more eps of the result for its own rounding.  ``dense`` (B, C, len): the dense product, ``hot``: |value|
    of the one sample."""
    pair = 2 * (b // 2)
    norm2 = dense.float().square().sum(-1)[pair:pair + 2].sum(0).max().sqrt().item()
    lg = points.bit_length() - 1
    return 2.0 ** -23 * (3 * lg * norm2 * hot + want.abs().max().item())


def _check_one_hot(what, got, want, bound, zero_rows):
    assert got.dtype == F32 and au.is_whole(want) and want.abs().max() <= 512 and bound < 0.5, (what, bound)
    err = (got.double() - want.double()).abs().max().item()
    print(f"    {what}: max error {err:.2e} within {bound:.2e}")
    assert not got[zero_rows].any(), f"{what}: a row of dW whose gated operand is zero holds a value"
    assert torch.equal(got.round(), want), f"{what}: {int((got.round() != want).sum())} elements are not the truth's integer"
    assert want.any() and err <= bound, f"{what}: error {err:.3e} above the bound of three float32 transforms {bound:.3e}"


def _one_hot_setups(monkeypatch):
    """(name, case, batch items): the second item of a pair and the unpaired last item; with B = 5 and one pair per slab an
    item of the second and of the third slab; and the grouped layer whose dY rows are shorter than x's."""
    yield "case 1", CASE1, (1, 2)
    five = (5,) + CASE1[1:]
    one_pair_per_slab(monkeypatch, five)
    yield "case 1, B 5 in three slabs", five, (3, 4)
    monkeypatch.delenv("FFTCONV_LONG_WS_MB")
    _clear()
    yield "case 2b", CASE2B, (1,)


@pytest.mark.parametrize("dtype", (F32, BF16), ids=("f32", "bf16"))
def test_a_one_hot_postgate_lands_on_its_sample(dtype, monkeypatch):
    for name, case, items in _one_hot_setups(monkeypatch):
        B, cin, cout, g, L, K, padding, causal = case
        nout = tg.out_len(case)
        x, pre, dy = _ints((B, cin, L), 1, dtype), _ints((B, cin, L), 2, dtype), _ints((B, cout, nout), 3, dtype)
        for t in (x, pre, dy):
            t[t == 0] = 7                                     # (no product is zero: the truth has a value wherever a tap meets the row)
        info = _native.wgrad_geometry(key_of(case))
        N2, points = info["N2"], info["N1"] * info["N2"]
        assert info["slabs"] == (3 if B == 5 else 1)
        # the ends of the row, a row boundary of the N1 x N2 layout, the last sample of a column block and its neighbour
        for t0 in (0, nout - 1, N2 - 1, N2, 16 * 77 - 1, 16 * 77):
            for b in items:
                o = (b + t0) % cout
                post = torch.zeros(B, cout, nout, device=DEV, dtype=dtype)
                post[b, o, t0] = 1.0
                what = f"{name} {dtype}: postgate one at ({b}, {o}, {t0})"
                got = run(case, x, pre, dy, post, F32)
                want = _truth_one_hot_postgate(case, x, pre, dy, b, o, t0)
                bound = _transform_bound(x.float() * pre.float(), abs(dy[b, o, t0].item()), b, points, want)
                _check_one_hot(what, got, want, bound, [r for r in range(cout) if r != o])
                gu.same_bits(got, reference(case, x, pre, dy, post, F32), what + ", against the reference dW")


@pytest.mark.parametrize("dtype", (F32, BF16), ids=("f32", "bf16"))
def test_a_one_hot_pregate_lands_on_its_sample(dtype, monkeypatch):
    for name, case, items in _one_hot_setups(monkeypatch):
        B, cin, cout, g, L, K, padding, causal = case
        nout, pl = tg.out_len(case), pads(case)[0]
        x, dy, post = _ints((B, cin, L), 4, dtype), _ints((B, cout, nout), 5, dtype), _ints((B, cout, nout), 6, dtype)
        for t in (x, dy, post):
            t[t == 0] = 7
        info = _native.wgrad_geometry(key_of(case))
        N2, points = info["N2"], info["N1"] * info["N2"]
        assert info["slabs"] == (3 if B == 5 else 1)
        # sample s of x sits at position s + pad_left of the row: the same places, counted in positions
        edge = (-pl) % N2 + 3 * N2
        assert (edge + pl) % N2 == 0 and (edge + 80 + pl) % 16 == 0 and (edge + 80 + pl) % N2
        for s0 in (0, L - 1, edge - 1, edge, edge + 79, edge + 80):
            for b in items:
                i = (b + s0) % cin
                pre = torch.zeros(B, cin, L, device=DEV, dtype=dtype)
                pre[b, i, s0] = 1.0
                what = f"{name} {dtype}: pregate one at ({b}, {i}, {s0})"
                got = run(case, x, pre, dy, post, F32)
                want = _truth_one_hot_pregate(case, x, dy, post, b, i, s0)
                bound = _transform_bound(dy.float() * post.float(), abs(x[b, i, s0].item()), b, points, want)
                cig, cog = cin // g, cout // g
                others = torch.ones(wshape(case), dtype=torch.bool, device=DEV)
                others[(i // cig) * cog:(i // cig + 1) * cog, i % cig] = False
                assert not got[others].any(), f"{what}: an element of dW whose signal row is zero holds a value"
                _check_one_hot(what, got, want, bound, [])
                gu.same_bits(got, reference(case, x, pre, dy, post, F32), what + ", against the reference dW")


# ------------------------------------------------------------------------------------------------ 6. slabs
def test_three_slabs(monkeypatch, gated_runs):
    case = (5,) + CASE1[1:]
    one_pair_per_slab(monkeypatch, case)
    for dtype in (F32, BF16):
        x, pre, dy, post = operands(case, dtype)
        gu.same_bits(run(case, x, pre, dy, post, dtype), reference(case, x, pre, dy, post, dtype), f"B 5 in three slabs, {dtype}")
    info = plan_info(case)
    assert (info["N1"] * info["N2"], info["slabs"], info["slab_pairs"]) == (8192, 3, 1), info
    assert len(gated_runs) == 2


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_launch_nothing_and_dilation_is_free():
    B, C, L, K = 2, 4, 5000, 100
    x, pre = torch.randn(B, C, L, device=DEV), torch.randn(B, C, L, device=DEV)
    NCL, NLC = _native.LONG_NCL, _native.LONG_NLC
    layers = {
        # text of the refusal -> (key words: pad_left, pad_right, nout, mode, stride, dilation), gates, layouts
        "a pregate with a \\(B, C, L\\) x only": ((0, 0, L - K + 1, 0, 1, 1), (True, False), (NLC, NCL)),
        "a pregate on plans with pad_mode constant only": ((50, 50, L + 100 - K + 1, 1, 1, 1), (True, False), (NCL, NCL)),
        "a postgate on plans with stride 1 only": ((0, 0, (L - K) // 2 + 1, 0, 2, 1), (False, True), (NCL, NCL)),
        "a postgate with a \\(B, C, L\\) dY only": ((0, 0, L - K + 1, 0, 1, 1), (False, True), (NCL, NLC)),
    }
    for text, ((pl, pr, nout, mode, s, d), (with_pre, with_post), (xl, dyl)) in layers.items():
        key = F_._long_wgrad_key(B, C, C, C, L, K, pl, pr, nout, False, mode, s, d)
        plan = F_._cached_plan(0, ("long_wgrad",) + key)
        dy, post = torch.randn(B, C, nout, device=DEV), torch.randn(B, C, nout, device=DEV)
        dw = torch.full((C, 1, K), 7.0, device=DEV)
        ws = F_.new_workspace(plan, x.device)
        stream = torch.cuda.current_stream().cuda_stream
        # (the ungated call takes the same tensors and layouts: what is refused is the gate)
        plan.run(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), stream, 0, 0, 0, xl, dyl)
        torch.cuda.synchronize()
        assert not (dw == 7.0).all()
        dw.fill_(7.0)
        with pytest.raises(NotImplementedError, match=text):
            plan.run_gated(x.data_ptr(), pre.data_ptr() if with_pre else None, dy.data_ptr(),
                           post.data_ptr() if with_post else None, dw.data_ptr(), ws.data_ptr(), stream, 0, 0, 0, xl, dyl)
        torch.cuda.synchronize()
        assert (dw == 7.0).all(), text
    # a dilation only chooses the lags the last pass keeps: both gates run
    d, nout = 2, L - 2 * (K - 1)
    key = F_._long_wgrad_key(B, C, C, C, L, K, 0, 0, nout, False, 0, 1, d)
    dy, post = torch.randn(B, C, nout, device=DEV), torch.randn(B, C, nout, device=DEV)
    case = (B, C, C, C, L, K, 0, False)
    gu.same_bits(run(case, x, pre, dy, post, F32, key), reference(case, x, pre, dy, post, F32, key), "dilation 2, both gates")


# ------------------------------------------------------------------------------------------------ 8. guard bands and poison
def test_guard_bands_and_poison(monkeypatch):
    from tests import test_gpu_memory_discipline as tm
    one_pair_per_slab(monkeypatch, CASE2B)
    x, pre, dy, post = operands(CASE2B, BF16)
    first = tm._runs(lambda x, pre, dy, post: run(CASE2B, x, pre, dy, post, BF16), (x, pre, dy, post), "gated weight gradient")
    assert plan_info(CASE2B)["slab_pairs"] == 1
    gu.same_bits(first[0], reference(CASE2B, x, pre, dy, post, BF16), "guarded dW against the reference dW")
    (odd,) = tm._runs(lambda x, pre, dy, post: run(CASE2B, x, pre, dy, post, BF16), (x, pre, dy, post),
                      "gated weight gradient", patterns=tm.RUNS[:2], offset=1)
    gu.same_bits(odd, first[0], "odd start against the aligned run")


# ------------------------------------------------------------------------------------------------ 9. memory
def test_no_product_tensor_exists(monkeypatch):
    """Derived, not measured: with the kernel's gradient alone asked for, the backward of the fused route under the switch
    allocates dW and the plan's workspace and nothing else; the parent's route also holds float32 pregate * x and
    postgate * dY while the plan runs."""
    monkeypatch.setenv("FFTCONV_LONG_WGRAD", "1")
    case = (4, 8, 8, 8, 20000, 20000, 0, True)
    x, w, _, pre, post = tg.tensors(case, BF16, bias=False)
    kw = tg.kw_of(case)
    gy = torch.randn(post.shape, generator=torch.Generator().manual_seed(5)).to(DEV).to(BF16)
    assert F_._long_gated_dw_route(x.shape, w.shape, 0, 8, True, BF16) == "gated-plan"

    def backward_peak():
        wl = w.detach().clone().requires_grad_()
        y = fft_long_conv_gated(x, wl, None, pregate=pre, postgate=post, **kw)       # the forward: before the statistics are reset
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        (dw,) = torch.autograd.grad(y, [wl], gy)
        torch.cuda.synchronize()
        return dw, torch.cuda.max_memory_allocated() - base

    def products_peak():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        z, q = x.float().mul_(pre), gy.float().mul_(post)      # (as the parent's backward forms them: one float32 tensor each)
        dw = F_._long_wgrad_run(z, q, wshape(case), key_of(case), BF16)
        del z, q
        torch.cuda.synchronize()
        return dw, torch.cuda.max_memory_allocated() - base

    backward_peak()                                          # warm: plans and tables
    (dw, a), (ref, c) = backward_peak(), products_peak()
    gu.same_bits(dw, ref, "dW of the step against the reference dW")
    ws = plan_info(case)["workspace_bytes"]
    blocks = 4 * 512                                         # allocator rounding of dW and of the workspace, twice over
    bound = dw.numel() * dw.element_size() + ws + blocks
    product = x.numel() * 4
    print(f"added peak of backward: gated plan {a / 2**20:.2f} MiB, float32 products {c / 2**20:.2f} MiB; dW + workspace "
          f"{bound / 2**20:.2f} MiB, one float32 product {product / 2**20:.2f} MiB")
    assert a <= bound
    assert a <= c - product


# ------------------------------------------------------------------------------------------------ 10. capture
def test_a_captured_training_step_replays_bit_for_bit(monkeypatch, gated_runs):
    monkeypatch.setenv("FFTCONV_LONG_WGRAD", "1")
    kw = tg.kw_of(CASE1)
    ts = tg.tensors(CASE1)
    static = [t.clone().requires_grad_() for t in ts]
    static_gy = torch.randn((3, 5, 2500), generator=torch.Generator().manual_seed(5)).to(DEV)

    def step():
        for t in static:
            t.grad = None
        fft_long_conv_gated(static[0], static[1], static[2], pregate=static[3], postgate=static[4], **kw).backward(static_gy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):               # warm: plans, tables and the allocator's pools exist
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert len(gated_runs) == 2
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    assert len(gated_runs) == 3 and all(r["pregate"] and r["postgate"] for r in gated_runs)
    for seed in (1, 2):
        fresh = tg.tensors(CASE1, seed=seed)
        fresh_gy = torch.randn(static_gy.shape, generator=torch.Generator().manual_seed(20 + seed)).to(DEV)
        with torch.no_grad():
            for s, f in zip(static, fresh):
                s.copy_(f)
            static_gy.copy_(fresh_gy)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.grad.clone() for t in static]
        _, eager = tg.grads_of(lambda x, w, b, p, q: fft_long_conv_gated(x, w, b, pregate=p, postgate=q, **kw), fresh, fresh_gy,
                               (True,) * 5)
        _, line = tg.grads_of(lambda x, w, b, p, q: tg.composed(x, w, b, p, q, **kw), fresh, fresh_gy, (True,) * 5)
        for name, a, e, l in zip(tg.NAMES, got, eager, line):
            gu.same_bits(a, e, f"replay {seed} {name} against the eager step")
            gu.same_bits(a, l, f"replay {seed} {name} against the line")
