"""``FFTLongConvStream`` on the GPU: a causal long filter decoded one token at a time.

Inputs are the integers of ``tests/accuracy_util.py`` ([-8, 8], so that a float64 convolution of them is exact) and every
column the stream emits is held to that file's bound against its FFT baseline of the whole row in the same precision
(``accuracy_util.check``; ``exact=True`` where the stream runs no transform).  The (row, taps, head, prefill) tuples are
those of ``tests/test_host_long_stream.py``, whose schedule they exercise: a truncated top level, more taps than positions,
partial blocks behind a prefill, one tap in the first level, and -- the one long case -- block levels whose padded row
passes 4096 points and runs the long transform.  Bit-equality claims (16-bit streams, gates, ``reset``) use
``guard_util.same_bits`` on normal samples."""
import functools

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from fft_conv_pytorch_amd import FFTLongConv1d, FFTLongConvStream, _native, fft_long_conv_gated
from tests import accuracy_util as au
from tests import guard_util as gu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


@pytest.fixture(autouse=True, scope="module")
def _fresh_cache():
    _native.clear_plan_cache()
    yield
    _native.clear_plan_cache()


# ------------------------------------------------------------------------------------------------ helpers
def decode(stream, x, prefill=0, pre=None, post=None, upto=None):
    """Every column the stream emits for the row x (B, Cin, L): ``prefill`` columns at once, the rest step by step."""
    B, _, L = x.shape
    L = L if upto is None else upto
    out = torch.empty((B, stream.out_channels, L), dtype=x.dtype, device=x.device)
    if prefill:
        out[:, :, :prefill] = stream.prefill(x[:, :, :prefill])
    cols = lambda t, j: None if t is None else t[:, :, j].contiguous()      # noqa: E731
    for j in range(prefill, L):
        out[:, :, j] = stream.step(cols(x, j), cols(pre, j), cols(post, j))
    assert stream.position == L
    return out


def exact_causal(x, w, b, groups, pre=None, post=None):
    """post * (b + causal convolution of pre * x with w) in float64 on the CPU: a float64 FFT convolution of the integers,
    rounded to the whole numbers it is within 1/4 of (``accuracy_util.whole``), and checked against explicit dot products."""
    x, w, b, pre, post = (None if t is None else t.double().cpu() for t in (x, w, b, pre, post))
    z = x if pre is None else pre * x
    (B, cin, L), (cout, cig, K) = z.shape, w.shape
    n = 1 << (L + K - 1).bit_length()
    zf = torch.fft.rfft(z, n).view(B, groups, 1, cig, -1)
    wf = torch.fft.rfft(w, n).view(groups, cout // groups, cig, -1)
    c = au.whole(torch.fft.irfft((zf * wf).sum(3), n)[..., :L].reshape(B, cout, L), "causal truth")
    gen = torch.Generator().manual_seed(3)
    for bi, o, t in zip(*(torch.randint(0, hi, (24,), generator=gen).tolist() for hi in (B, cout, L))):
        g, m = o // (cout // groups), min(K, t + 1)
        rows = z[bi, g * cig:(g + 1) * cig, t - m + 1:t + 1].flip(-1)
        assert c[bi, o, t] == (rows * w[o, :, :m]).sum(), (bi, o, t)
    if b is not None:
        c = c + b.view(1, -1, 1)
    return c if post is None else post * c


def fft_baseline(x, w, b, groups, pre=None, post=None):
    """The model project's FFT formulation of the whole row in the tensors' own precision (``accuracy_util.baseline_conv``)."""
    K = w.shape[2]
    z = x if pre is None else pre * x
    c = au.baseline_conv(torch.nn.functional.pad(z, (K - 1, 0)), w.flip(-1).contiguous(), b, 1, 0, 1, groups)
    return c if post is None else post * c


@functools.lru_cache(maxsize=None)
def row(B, cin, cout, groups, L, K, gates=False):
    """(x, w, b, pre, post, truth, baseline) of one layer on integers: made once, shared, never written."""
    gen = torch.Generator().manual_seed(L + 3 * K + B)
    x = au.integers((B, cin, L), gen, F32, DEV)
    w = au.integers((cout, cin // groups, K), gen, F32, DEV)
    b = au.integers((cout,), gen, F32, DEV)
    pre = au.integers((B, cin, L), gen, F32, DEV) if gates else None
    post = au.integers((B, cout, L), gen, F32, DEV) if gates else None
    assert (8 if gates else 1) ** 2 * 64 * K * (cin // groups) + 64 < 2 ** 24      # every partial sum: an integer float32 holds
    return x, w, b, pre, post, exact_causal(x, w, b, groups, pre, post), fft_baseline(x, w, b, groups, pre, post)


def check_row(what, layer, L, K, head, prefill, max_len=None, exact=False):
    B, cin, cout, groups = layer
    x, w, b, _, _, want, base = row(B, cin, cout, groups, L, K)
    stream = FFTLongConvStream(w, b, groups, batch=B, max_len=max_len or L, head=head)
    got = decode(stream, x, prefill)
    assert got.dtype == F32 and not got.requires_grad
    au.check(what, got, want, base, F32, exact=exact)
    return stream, got


GROUPED = (3, 4, 6, 2)        # odd batch, 4 -> 6 channels in 2 groups


# ------------------------------------------------------------------------------------------------ 1. head only
@pytest.mark.parametrize("K", [5, 16])
def test_head_only_streams_are_exact(K):
    """No block level exists (K <= head): every column is the step kernel's own sum of integers below 2**24."""
    stream, _ = check_row(f"head only K={K}", GROUPED, 130, K, 16, 0, exact=True)
    assert stream._levels == {} and not stream.acc.any()


@pytest.mark.parametrize("K", [16, 17])
def test_one_tap_in_the_first_block_level(K):
    """K = head + 1: the first level holds tap 16 alone (K = 16: none); a prefill of 3 leaves partial blocks."""
    stream, _ = check_row(f"K={K} head 16 prefill 3", GROUPED, 200, K, 16, 3)
    assert sorted(stream._levels) == ([16] if K == 17 else [])


# ------------------------------------------------------------------------------------------------ 2. grouped, odd batch
@pytest.mark.parametrize("K,head,prefill,L,max_len", [(300, 16, 0, 300, 300), (77, 16, 0, 300, 300), (500, 8, 100, 257, 257)],
                         ids=["K300", "K77-truncated-top", "K500-past-max_len"])
def test_grouped_odd_batch_every_column(K, head, prefill, L, max_len):
    check_row(f"grouped K={K}", GROUPED, L, K, head, prefill, max_len)


@pytest.mark.parametrize("L,K,head,prefill", [(1024, 1024, 64, 0), (1000, 513, 64, 129)])
def test_head_64_schedules(L, K, head, prefill):
    check_row(f"L={L} K={K} head {head} prefill {prefill}", (2, 2, 2, 2), L, K, head, prefill)


# ------------------------------------------------------------------------------------------------ 3. prefill, then decode
@pytest.mark.parametrize("prefill", [37, 48])
def test_prefill_then_decode(prefill):
    """L0 = 37 is no multiple of the head, 48 is one; the prefill's columns and every later one are checked."""
    B, cin, cout, groups = GROUPED
    x, w, b, _, _, want, base = row(B, cin, cout, groups, 300, 300)
    stream = FFTLongConvStream(w, b, groups, batch=B, max_len=300, head=16)
    first = stream.prefill(x[:, :, :prefill])
    assert tuple(first.shape) == (B, cout, prefill) and first.is_contiguous() and stream.position == prefill
    au.check(f"prefill {prefill}: its own columns", first, want[:, :, :prefill], base[:, :, :prefill], F32)
    with pytest.raises(RuntimeError, match="position 0 only"):
        stream.prefill(x[:, :, :prefill])
    stream.reset()
    got = decode(stream, x, prefill)
    au.check(f"prefill {prefill}: every column", got, want, base, F32)
    au.check(f"prefill {prefill}: the decoded columns", got[:, :, prefill:], want[:, :, prefill:], base[:, :, prefill:], F32)
    with pytest.raises(RuntimeError, match="position 0 only"):
        stream.prefill(x[:, :, :prefill])


# ------------------------------------------------------------------------------------------------ 4. long-transform blocks
def test_long_transform_blocks_and_no_plan_in_steady_state():
    """Depthwise K = 8197, head 64, prefill 4000, decoded to 8300: the 4096-point level (due at i = 8192; a padded row of
    12286 points) and its neighbours (2048 points: 6142; 8192 points against five taps: 8200) run the N1 x N2 transform, the levels
    below hand off, and the blocks due between 4000 and 4096 straddle ``first``.  Steady-state steps create no plan."""
    B, C, L, K, head, prefill = 2, 3, 8300, 8197, 64, 4000
    x, w, b, _, _, want, base = row(B, C, C, C, L, K)
    stream = FFTLongConvStream(w, b, C, batch=B, max_len=L, head=head)
    assert sorted(stream._levels) == [64 << j for j in range(8)]
    assert [n for n, lv in stream._levels.items() if lv[2] is None] == [2048, 4096, 8192]      # (no hand-off plan: the long path)
    got = decode(stream, x, prefill, upto=L - 1000)
    plans = len(_native._plans)
    tail = torch.stack([stream.step(x[:, :, j].contiguous()) for j in range(L - 1000, L)], dim=2)
    assert len(_native._plans) == plans, "a steady-state step created a plan"
    assert L - 1000 < 8192 < L        # the 4096- and 8192-point levels fell due (for the first time) inside those steps
    au.check("K=8197 depthwise, long-transform levels", torch.cat([got, tail], dim=2), want, base, F32)


# ------------------------------------------------------------------------------------------------ 5. 16-bit streams
def normal_row(B, cin, cout, groups, L, K, dtype, seed=0):
    gen = torch.Generator().manual_seed(seed + L + 3 * K + B)
    rnd = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    ts = (rnd(B, cin, L), rnd(cout, cin // groups, K) / (K * cin // groups) ** 0.5, rnd(cout), rnd(B, cin, L), rnd(B, cout, L))
    return tuple(t.to(DEV).to(dtype) for t in ts)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["float16", "bfloat16"])
def test_16_bit_streams_have_the_bits_of_the_widened_float32_stream(dtype):
    """Every ``prefill`` / ``step`` output: the float32 stream on the widened tensors, rounded once with ``.to(dtype)``."""
    B, cin, cout, groups = GROUPED
    x, w, b, pre, post = normal_row(B, cin, cout, groups, 150, 300, dtype)
    half = FFTLongConvStream(w, b, groups, batch=B, max_len=150, head=16)
    wide = FFTLongConvStream(w.float(), b.float(), groups, batch=B, max_len=150, head=16)
    assert half.state_bytes == wide.state_bytes == 4 * 150 * B * (cin + cout)
    assert half.hist.dtype == half.acc.dtype == F32
    y = half.prefill(x[:, :, :37])
    assert y.dtype == dtype
    gu.same_bits(y, wide.prefill(x[:, :, :37].float()).to(dtype), f"{dtype} prefill")
    for j in range(37, 150):
        gates = (pre[:, :, j].contiguous(), post[:, :, j].contiguous()) if j % 3 else (None, None)
        y = half.step(x[:, :, j].contiguous(), *gates)
        ref = wide.step(x[:, :, j].float().contiguous(), *(None if g is None else g.float() for g in gates))
        assert y.dtype == dtype and tuple(y.shape) == (B, cout)
        gu.same_bits(y, ref.to(dtype), f"{dtype} step {j}")
    gu.same_bits(half.hist, wide.hist, f"{dtype} history")
    gu.same_bits(half.acc, wide.acc, f"{dtype} accumulator")


# ------------------------------------------------------------------------------------------------ 6. gates
@pytest.mark.parametrize("which", ["both", "pregate", "postgate"])
def test_gates(which):
    """Bits: the gated step is the ungated stream fed pregate * x_t, its output multiplied by postgate (float32: the same
    two multiplies).  Accuracy: within the bound, with ``fft_long_conv_gated`` on the whole row as the baseline."""
    B, cin, cout, groups = GROUPED
    L, K, head = 200, 300, 16
    x, w, b, pre, post, _, _ = row(B, cin, cout, groups, L, K, True)
    pre, post = (pre if which != "postgate" else None), (post if which != "pregate" else None)
    gated = FFTLongConvStream(w, b, groups, batch=B, max_len=L, head=head)
    plain = FFTLongConvStream(w, b, groups, batch=B, max_len=L, head=head)
    got = decode(gated, x, 0, pre, post)
    ref = decode(plain, x if pre is None else pre * x, 0)
    gu.same_bits(got, ref if post is None else post * ref, f"gates: {which}")
    want = exact_causal(x, w, b, groups, pre, post)
    with torch.no_grad():
        base = fft_long_conv_gated(x, w, b, groups=groups, causal=True, pregate=pre, postgate=post)
    au.check(f"gates: {which}, against fft_long_conv_gated", got, want, base, F32)


# ------------------------------------------------------------------------------------------------ 7. memory discipline
@pytest.fixture
def library_calls(monkeypatch):
    """Names of the library calls made: the step, and every launch entry of the two plan classes."""
    seen = []

    def spy(owner, name):
        real = getattr(owner, name)

        def wrapped(*a, **k):
            seen.append(name)
            return real(*a, **k)
        monkeypatch.setattr(owner, name, wrapped)
    spy(_native, "long_step")
    for cls in (_native.LongPlan, _native.Plan):
        for name in ("forward", "forward_lay", "transform_kernel"):
            spy(cls, name)
    spy(_native.LongPlan, "forward_gated")
    return seen


def test_a_step_writes_one_column_of_hist_and_its_own_output(library_calls):
    B, cin, cout, groups = GROUPED
    x, w, b, pre, _, _, _ = row(B, cin, cout, groups, 200, 300, True)
    L = 60
    stream = FFTLongConvStream(w, b, groups, batch=B, max_len=L, head=16)
    stream.prefill(x[:, :, :21])                      # (acc holds the prefill's tail: something to damage)
    z = torch.cat([x[:, :, :21], (pre * x)[:, :, 21:]], dim=2)
    for j in range(21, L):
        acc = stream.acc.clone()
        with gu.guarded_empty(0xFF) as guard:         # y_t lies between NaN-filled guard bands
            y = stream.step(x[:, :, j].contiguous(), pre[:, :, j].contiguous())
        assert guard.violations() == [] and guard.served[0] == ((B, cout), F32)
        assert len(guard.served) == 1 or (j + 1) % 16 == 0
        assert au.finite(y), "a sample of y_t was not written"
        assert not stream.hist[:, :, j + 1:].any(), f"step {j} wrote hist behind its column"
        gu.same_bits(stream.hist[:, :, :j + 1], z[:, :, :j + 1], f"hist after step {j}")
        if (j + 1) % 16:
            gu.same_bits(stream.acc, acc, f"acc across step {j}")
        else:                                         # blocks fell due: they reach positions from j + 1 on only
            gu.same_bits(stream.acc[:, :, :j + 1], acc[:, :, :j + 1], f"acc below {j + 1} across step {j}")
    assert stream.position == L == stream.max_len
    hist, acc, calls = stream.hist.clone(), stream.acc.clone(), len(library_calls)
    with pytest.raises(RuntimeError, match="max_len"):
        stream.step(x[:, :, 0].contiguous())
    assert len(library_calls) == calls, "a step past max_len launched something"
    gu.same_bits(stream.hist, hist, "hist after the refused step")
    gu.same_bits(stream.acc, acc, "acc after the refused step")


class _Ops(TorchDispatchMode):
    """Every ATen operator torch dispatches while active."""

    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(str(func))
        return func(*args, **(kwargs or {}))


def test_a_step_without_a_block_is_one_library_call_and_no_torch_kernel(library_calls):
    B, cin, cout, groups = GROUPED
    x, w, b, pre, post, _, _ = row(B, cin, cout, groups, 200, 300, True)
    stream = FFTLongConvStream(w, b, groups, batch=B, max_len=200, head=16)
    cols = [t[:, :, 0].contiguous() for t in (x, pre, post)]
    del library_calls[:]
    for j in range(40):
        with _Ops() as ops:
            stream.step(*cols)
        kernels = [n for n in ops.names if not n.startswith(("aten.empty", "aten.detach", "aten.alias"))]
        if (j + 1) % 16:
            assert library_calls == ["long_step"], (j, library_calls)
            assert kernels == [], (j, kernels)          # the output's allocation is all torch does
        else:
            assert library_calls[0] == "long_step" and "forward" in library_calls[1:], (j, library_calls)
            assert "transform_kernel" not in library_calls, "a spectrum was made again"
        del library_calls[:]


# ------------------------------------------------------------------------------------------------ 8. module
def test_module_stream_agrees_with_the_modules_forward_and_reset_replays():
    B, cin, cout, groups = GROUPED
    L, K = 300, 300
    x, w, b, _, _, want, _ = row(B, cin, cout, groups, L, K)
    layer = FFTLongConv1d(cin, cout, K, groups=groups, causal=True).to(DEV).eval()
    with torch.no_grad():
        layer.weight.copy_(w)
        layer.bias.copy_(b)
        whole = layer(x)
    stream = layer.stream(B, L, head=16)
    assert isinstance(stream, FFTLongConvStream) and (stream.head, stream.max_len, stream.position) == (16, L, 0)
    got = decode(stream, x, 48)
    au.check("module stream against the module's forward", got, want, whole, F32)
    with torch.no_grad():
        layer.weight.zero_()                            # the stream holds a snapshot
    stream.reset()
    assert stream.position == 0 and not stream.hist.any() and not stream.acc.any()
    gu.same_bits(decode(stream, x, 48), got, "replay after reset()")
    assert layer.stream(B, L).head == 64                # the default head
