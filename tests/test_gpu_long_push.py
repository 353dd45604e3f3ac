"""``FFTLongConvStream.push`` on the GPU: T tokens appended at once at any position.

Inputs, truth and baseline are those of ``tests/test_gpu_long_stream.py`` (integers in [-8, 8], an exact float64 causal
convolution, the plain-FFT baseline in the same precision; its ``row`` cache is shared), and every column a push or a step
emits is held to ``accuracy_util.check`` (``exact=True`` where no transform runs).  The (row, taps, head, prefill) tuples are
those of ``tests/test_host_long_push.py``, whose schedule they exercise under a seeded mix of steps and pushes, with the
bulk convolutions and under FFTCONV_LONG_PUSH_BULK=0.  Bit-equality claims (cuts of a head-only row, 16-bit streams,
``reset``) use ``guard_util.same_bits`` on normal samples."""
import numpy as np
import pytest
import torch

from fft_conv_pytorch_amd import FFTLongConvStream, _native
from fft_conv_pytorch_amd import functional as F_
from tests import accuracy_util as au
from tests import guard_util as gu
from tests.test_gpu_long_stream import GROUPED, exact_causal, fft_baseline, normal_row, row
from tests.test_host_long_push import IDS, SCHEDULES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


@pytest.fixture(autouse=True, scope="module")
def _fresh_cache():
    _native.clear_plan_cache()
    yield
    _native.clear_plan_cache()


@pytest.fixture(params=["bulk", "windows-only"])
def bulk(request, monkeypatch):
    monkeypatch.setenv("FFTCONV_LONG_PUSH_BULK", "1" if request.param == "bulk" else "0")
    return request.param == "bulk"


# ------------------------------------------------------------------------------------------------ helpers
def feed(stream, x, sizes, pre=None, post=None, out=None):
    """The columns the stream emits from its position on for ``sizes``: 0 is one ``step``, T >= 1 a ``push`` of T tokens,
    None a push of the rest of the row."""
    B, _, L = x.shape
    out = torch.empty((B, stream.out_channels, L), dtype=x.dtype, device=x.device) if out is None else out
    for T in sizes:
        p = stream.position
        if T == 0:
            col = lambda t: None if t is None else t[:, :, p].contiguous()      # noqa: E731
            out[:, :, p] = stream.step(col(x), col(pre), col(post))
            assert stream.position == p + 1
            continue
        T = L - p if T is None else T
        cut = lambda t: None if t is None else t[:, :, p:p + T]      # noqa: E731  (non-contiguous: push copies)
        y = stream.push(cut(x), cut(pre), cut(post))
        assert tuple(y.shape) == (B, stream.out_channels, T) and y.is_contiguous() and y.dtype == x.dtype
        assert not y.requires_grad and stream.position == p + T
        out[:, :, p:p + T] = y
    return out


CUT = [1, 3, 15, 16, 17, 32, None]


def causal64(x, w, b, groups):
    """b + the causal convolution of x with w as torch's float64 convolution on the CPU (any samples, not only integers)."""
    x, w, b = (t.double().cpu() for t in (x, w, b))
    return torch.nn.functional.conv1d(torch.nn.functional.pad(x, (w.shape[2] - 1, 0)), w.flip(-1), b, groups=groups)


# ------------------------------------------------------------------------------------------------ a. head only
@pytest.mark.parametrize("K", [5, 16])
def test_head_only_pushes_are_exact_and_do_not_depend_on_the_cut(K):
    """No block level exists (K <= head): every column is the push kernel's own sum.  On integers it is exact; on normal
    samples the bits of a column are the same whether the row came as one push or in pieces (one chain of fused
    multiply-adds per output, c ascending then k ascending), and a step's -- a wave-wide butterfly sum of the same terms --
    stay within the forward error bound of such a sum of the float64 result: (terms + 2) eps (|b| + sum |w| |z|), terms =
    head x channels per group (eps is twice the unit roundoff: the bound has that factor to spare)."""
    B, cin, cout, groups = GROUPED
    L = 130
    x, w, b, _, _, want, base = row(B, cin, cout, groups, L, K)
    stream = FFTLongConvStream(w, b, groups, batch=B, max_len=L, head=16)
    got = feed(stream, x, CUT)
    assert stream.position == L and stream._levels == {} and stream._bulk_levels == {} and not stream.acc.any()
    au.check(f"head only K={K}, pushes of {CUT}", got, want, base, F32, exact=True)
    gu.same_bits(stream.hist, x, "hist after the pushes")

    xn, wn, bn, _, _ = normal_row(B, cin, cout, groups, L, K, F32)
    stream = FFTLongConvStream(wn, bn, groups, batch=B, max_len=L, head=16)
    once = feed(stream, xn, [None])
    stream.reset()
    pieces = feed(stream, xn, CUT)
    gu.same_bits(once, pieces, "one push against pushes of " + str(CUT))
    stream.reset()
    steps = feed(stream, xn, [0] * L)
    exact, budget = causal64(xn, wn, bn, groups), causal64(xn.abs(), wn.abs(), bn.abs(), groups)
    bound = ((cin // groups) * 16 + 2) * float(torch.finfo(F32).eps) * budget
    for name, y in (("push", once), ("step", steps)):
        assert bool(((y.double().cpu() - exact).abs() <= bound).all()), f"{name}: outside the forward error bound"


# ------------------------------------------------------------------------------------------------ b. every schedule
def mix(L, U, L0, seed):
    """A seeded mix of steps (0) and pushes from L0 to L: a push of 3 and two steps, then whatever the seed draws.  The
    last entry is a push that ends at L."""
    rng = np.random.default_rng(seed)
    sizes, out, p = [0, 0, 1, 3, U - 1, U, U + 1, 2 * U, 5 * U + 3, 8 * U], [3, 0, 0], L0 + 5
    while L - p > 2 * U:
        T = int(sizes[rng.integers(len(sizes))])
        T = min(T, L - p - 2)
        out.append(T)
        p += max(T, 1)
    return out + [None]


@pytest.mark.parametrize("L,K,U,L0", SCHEDULES, ids=IDS)
def test_every_schedule_under_a_mix_of_steps_and_pushes(L, K, U, L0, bulk):
    """Prefill of L0, then steps and pushes that start and end on and off the grid of the head; the last push ends exactly
    at max_len = L (K = 500 > max_len among the tuples)."""
    layer = (2, 2, 2, 2) if U == 64 else GROUPED
    B, cin, cout, groups = layer
    x, w, b, _, _, want, base = row(B, cin, cout, groups, L, K)
    sizes = mix(L, U, L0, L + K + U + L0)
    starts, p = [], L0
    for T in sizes:
        T = L - p if T is None else T
        if T:
            starts.append((p, p + T))
        p += max(T, 1)
    assert p == L and 0 in sizes
    assert any(a % U for a, _ in starts) and any(e % U for _, e in starts) and starts[-1][1] == L
    if K > U and bulk:
        ops = [op for a, e in starts for op in F_._long_push_plan(a, e - a, U, K, L0)]
        assert any(op[0] == "bulk" for op in ops)
    stream = FFTLongConvStream(w, b, groups, batch=B, max_len=L, head=U)
    out = torch.empty((B, cout, L), dtype=F32, device=DEV)
    if L0:
        out[:, :, :L0] = stream.prefill(x[:, :, :L0])
    feed(stream, x, sizes, out=out)
    assert stream.position == L and (bulk or stream._bulk_levels == {})
    au.check(f"L={L} K={K} head {U} prefill {L0} bulk={bulk}", out, want, base, F32, exact=K <= U and not L0)
    gu.same_bits(stream.hist, x, "hist")


# ------------------------------------------------------------------------------------------------ c. the long transform
def test_a_bulk_through_the_long_transform_and_lazy_levels():
    """K = L = max_len = 4096, head 64: one push at 0 is one bulk of 4096 samples against the taps [64, 4096), about 8128
    points, past the hand-off to the tile kernels.  Levels are made by the first push that needs them, never again."""
    B, C, L, K, head = 2, 2, 4096, 4096, 64
    x, w, b, _, _, want, base = row(B, C, C, C, L, K)
    assert F_._long_push_plan(0, L, head, K, 0) == [("bulk", 0, L, head, K), ("window", 0, L)]
    stream = FFTLongConvStream(w, b, C, batch=B, max_len=L, head=head)
    assert stream._bulk_levels == {} and stream.bulk_spectrum_bytes == 0
    got = feed(stream, x, [None])
    assert sorted(stream._bulk_levels) == [4096] and stream._bulk_levels[4096][2] is None      # (no hand-off plan: the long path)
    assert stream.bulk_spectrum_bytes > 0
    au.check("one push of 4096, bulk through the long transform", got, want, base, F32)
    plans, level = len(_native._plans), stream._bulk_levels[4096]
    stream.reset()
    again = feed(stream, x, [None])
    assert len(_native._plans) == plans and stream._bulk_levels[4096] is level, "a second push made a plan or a spectrum"
    gu.same_bits(again, got, "the same push after reset()")

    fresh = FFTLongConvStream(w, b, C, batch=B, max_len=L, head=head)
    got = feed(fresh, x, [2048] + [0] * 64 + [None])
    assert sorted(fresh._bulk_levels) == [128, 256, 512, 1024, 2048]
    au.check("2048 + 64 steps + the rest", got, want, base, F32)


# ------------------------------------------------------------------------------------------------ d. gates, 16-bit
@pytest.mark.parametrize("which", ["both", "pregate", "postgate"])
def test_gates(which, bulk):
    B, cin, cout, groups = GROUPED
    L, K, head = 200, 300, 16
    x, w, b, pre, post, _, _ = row(B, cin, cout, groups, L, K, True)
    pre, post = (pre if which != "postgate" else None), (post if which != "pregate" else None)
    want, base = exact_causal(x, w, b, groups, pre, post), fft_baseline(x, w, b, groups, pre, post)
    stream = FFTLongConvStream(w, b, groups, batch=B, max_len=L, head=head)
    got = feed(stream, x, [3, 45, 0, 0, 64, None], pre, post)
    au.check(f"gates: {which}, bulk={bulk}", got, want, base, F32)
    gu.same_bits(stream.hist, x if pre is None else pre * x, "hist holds pregate * x")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["float16", "bfloat16"])
def test_16_bit_pushes_have_the_bits_of_the_widened_float32_stream(dtype):
    """Every ``push`` output: the float32 stream's push on the widened tensors, rounded once with ``.to(dtype)``."""
    B, cin, cout, groups = GROUPED
    L = 150
    x, w, b, pre, post = normal_row(B, cin, cout, groups, L, 300, dtype)
    half = FFTLongConvStream(w, b, groups, batch=B, max_len=L, head=16)
    wide = FFTLongConvStream(w.float(), b.float(), groups, batch=B, max_len=L, head=16)
    gu.same_bits(half.prefill(x[:, :, :5]), wide.prefill(x[:, :, :5].float()).to(dtype), f"{dtype} prefill")
    for T, gated in ((3, True), (40, False), (70, True), (L - 118, True)):
        p = half.position
        cols = [t[:, :, p:p + T].contiguous() if gated or t is x else None for t in (x, pre, post)]
        y = half.push(*cols)
        ref = wide.push(*(None if t is None else t.float() for t in cols))
        assert y.dtype == dtype and ref.dtype == F32
        gu.same_bits(y, ref.to(dtype), f"{dtype} push of {T} at {p}")
    assert half.position == wide.position == L and sorted(half._bulk_levels) == sorted(wide._bulk_levels) == [32]
    gu.same_bits(half.hist, wide.hist, f"{dtype} history")
    gu.same_bits(half.acc, wide.acc, f"{dtype} accumulator")


# ------------------------------------------------------------------------------------------------ e. state discipline
@pytest.fixture
def library_calls(monkeypatch):
    """Names of the library calls made: the step, the push, and every launch entry of the two plan classes."""
    seen = []

    def spy(owner, name):
        real = getattr(owner, name)

        def wrapped(*a, **k):
            seen.append(name)
            return real(*a, **k)
        monkeypatch.setattr(owner, name, wrapped)
    spy(_native, "long_step")
    spy(_native, "long_push")
    for cls in (_native.LongPlan, _native.Plan):
        for name in ("forward", "forward_lay", "transform_kernel"):
            spy(cls, name)
    return seen


@pytest.mark.parametrize("p,T", [(21, 1), (21, 11), (21, 100), (32, 64), (130, 70)])
def test_a_push_writes_its_columns_of_hist_and_its_own_output(p, T, library_calls, bulk):
    B, cin, cout, groups = GROUPED
    x, w, b, pre, _, _, _ = row(B, cin, cout, groups, 200, 300, True)
    L = 200
    stream = FFTLongConvStream(w, b, groups, batch=B, max_len=L, head=16)
    stream.prefill(x[:, :, :p])                       # (acc holds the prefill's tail: something to damage)
    hist, acc = stream.hist.clone(), stream.acc.clone()
    with gu.guarded_empty(0xFF) as guard:             # y, and every copy a window makes, between NaN-filled guard bands
        y = stream.push(x[:, :, p:p + T], pre[:, :, p:p + T])
    assert guard.violations() == [] and guard.served[0] == ((B, cout, T), F32)
    assert au.finite(y), "a sample of y was not written"
    assert library_calls.count("long_push") == sum(op[0] == "window" for op in F_._long_push_plan(p, T, 16, 300, p, bulk))
    gu.same_bits(stream.hist[:, :, :p], hist[:, :, :p], "hist below the chunk")
    gu.same_bits(stream.hist[:, :, p + T:], hist[:, :, p + T:], "hist behind the chunk")
    gu.same_bits(stream.hist[:, :, p:p + T], (pre * x)[:, :, p:p + T], "hist of the chunk: pregate * x")
    gu.same_bits(stream.acc[:, :, :p], acc[:, :, :p], "acc below the chunk")
    assert stream.position == p + T


def test_a_refused_push_touches_nothing(library_calls):
    B, cin, cout, groups = GROUPED
    x, w, b, _, _, _, _ = row(B, cin, cout, groups, 200, 300, True)
    stream = FFTLongConvStream(w, b, groups, batch=B, max_len=60, head=16)
    stream.push(x[:, :, :50])
    hist, acc, calls = stream.hist.clone(), stream.acc.clone(), len(library_calls)
    with pytest.raises(RuntimeError, match="T = 11 tokens at position 50 passes max_len = 60"):
        stream.push(x[:, :, 50:61])
    with pytest.raises(ValueError, match="`x` must have shape"):
        stream.push(x[:, :1, 50:55])
    assert len(library_calls) == calls and stream.position == 50
    gu.same_bits(stream.hist, hist, "hist after the refused pushes")
    gu.same_bits(stream.acc, acc, "acc after the refused pushes")
    stream.push(x[:, :, 50:60])                       # up to max_len exactly
    assert stream.position == 60
    with pytest.raises(RuntimeError, match="max_len"):
        stream.push(x[:, :, :1])


# ------------------------------------------------------------------------------------------------ f. mixing with steps
def test_steps_continue_a_push_and_a_push_continues_steps(bulk):
    B, cin, cout, groups = GROUPED
    L, K = 300, 300
    x, w, b, _, _, want, base = row(B, cin, cout, groups, L, K)
    stream = FFTLongConvStream(w, b, groups, batch=B, max_len=L, head=16)
    sizes = [100] + [0] * 41 + [70] + [0] * 20 + [None]
    got = feed(stream, x, sizes)
    au.check(f"push, steps, push, steps, push; bulk={bulk}", got, want, base, F32)
    au.check("the steps after the first push", got[:, :, 100:141], want[:, :, 100:141], base[:, :, 100:141], F32)
    au.check("the push after those steps", got[:, :, 141:211], want[:, :, 141:211], base[:, :, 141:211], F32)
    stream.reset()
    assert stream.position == 0 and not stream.hist.any() and not stream.acc.any()
    gu.same_bits(feed(stream, x, sizes), got, "replay after reset()")
