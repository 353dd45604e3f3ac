"""``FFTLongConvStream.speculate`` / ``accept`` on the GPU: draft tokens verified without the accumulator being touched,
then committed or dropped.

Inputs, truth and baseline are those of ``tests/test_gpu_long_stream.py`` (integers in [-8, 8], an exact float64 causal
convolution, the plain-FFT baseline in the same precision; its ``row`` cache is shared).  Every column ``speculate``
returns is held to ``accuracy_util.check`` against that truth (``exact=True`` where no transform has run), a column below
the multiple M of the head inside the draft to the bits of a twin stream's ``push`` of the same chunk besides, and the
state after ``accept(a)`` to the bits of a twin that pushed the accepted tokens alone (``guard_util.same_bits``).  No other
tolerance is used: the only place ``speculate`` may differ in bits from ``push`` are the columns t >= M, whose late pairs
the kernel sums directly where a push runs blocks."""
import functools

import numpy as np
import pytest
import torch

from fft_conv_pytorch_amd import FFTLongConvStream, _native
from fft_conv_pytorch_amd import functional as F_
from tests import accuracy_util as au
from tests import guard_util as gu
from tests.test_gpu_long_stream import GROUPED, exact_causal, fft_baseline, normal_row, row

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
WIDE_GROUPS = (2, 4, 12, 2)      # 4 -> 12 channels in 2 groups: six outputs per group, more than the four waves of a workgroup


@pytest.fixture(autouse=True, scope="module")
def _fresh_cache():
    _native.clear_plan_cache()
    yield
    _native.clear_plan_cache()


@pytest.fixture
def library_calls(monkeypatch):
    """Names of the library calls made: the step, the push, the draft, and every launch entry of the two plan classes."""
    seen = []

    def spy(owner, name):
        real = getattr(owner, name)

        def wrapped(*a, **k):
            seen.append(name)
            return real(*a, **k)
        monkeypatch.setattr(owner, name, wrapped)
    for name in ("long_step", "long_push", "long_spec"):
        spy(_native, name)
    for cls in (_native.LongPlan, _native.Plan):
        for name in ("forward", "forward_lay", "transform_kernel"):
            spy(cls, name)
    return seen


# ------------------------------------------------------------------------------------------------ helpers
def ran_blocks(calls):
    """Whether a block convolution (a forward launch of either plan class) is among the library calls."""
    return any(name in ("forward", "forward_lay") for name in calls)


def cut(t, lo, hi):
    return None if t is None else t[:, :, lo:hi]      # (non-contiguous: the stream copies)


def bring(w, b, groups, B, max_len, head, x, p, prefill, pre=None):
    """A fresh stream at position ``p``: ``prefill`` columns at once (ungated), the rest by one ``push``."""
    stream = FFTLongConvStream(w, b, groups, batch=B, max_len=max_len, head=head)
    if prefill:
        stream.prefill(x[:, :, :prefill])
    if p > prefill:
        stream.push(cut(x, prefill, p), cut(pre, prefill, p))
    assert stream.position == p
    return stream


def draft(what, tensors, groups, head, max_len, prefill, p, T, exact=False):
    """One draft of T tokens at p on a fresh stream, next to a twin that pushes the same chunk; the checks every draft gets:
    all columns within the bound of the truth, the columns below M with the bits of the push, position, ``acc`` and
    ``hist`` outside [p, p + T) untouched, ``hist[..., p:p + T]`` = z.  -> (the stream, its twin, y, M or None)."""
    x, w, b, pre, post, want, base = tensors
    B, K = int(x.shape[0]), int(w.shape[2])
    spec, twin = (bring(w, b, groups, B, max_len, head, x, p, prefill, pre) for _ in range(2))
    gu.same_bits(spec.acc, twin.acc, f"{what}: the twins' acc before the draft")
    hist, acc = spec.hist.clone(), spec.acc.clone()
    chunk = [cut(t, p, p + T) for t in (x, pre, post)]
    y = spec.speculate(*chunk)
    assert tuple(y.shape) == (B, int(w.shape[0]), T) and y.is_contiguous() and y.dtype == x.dtype and not y.requires_grad
    assert spec.position == p and spec._draft == (p, T)
    ref = twin.push(*chunk)
    M, blocks = F_._long_spec_plan(p, T, head, K, prefill, max_len)
    au.check(what, y, want[:, :, p:p + T], base[:, :, p:p + T], F32, exact=exact)
    same = T if M is None or not blocks else M - p
    gu.same_bits(y[:, :, :same], ref[:, :, :same], f"{what}: the columns below M = {M} against the push")
    gu.same_bits(spec.acc, acc, f"{what}: acc across speculate")
    gu.same_bits(spec.hist[:, :, :p], hist[:, :, :p], f"{what}: hist below the draft")
    gu.same_bits(spec.hist[:, :, p + T:], hist[:, :, p + T:], f"{what}: hist behind the draft")
    z = x if pre is None else pre * x
    gu.same_bits(spec.hist[:, :, p:p + T], z[:, :, p:p + T].contiguous(), f"{what}: hist of the draft = z")
    return spec, twin, y, M


def state_equal(what, a, b):
    assert a.position == b.position, (what, a.position, b.position)
    gu.same_bits(a.acc, b.acc, f"{what}: acc")
    gu.same_bits(a.hist[:, :, :a.position], b.hist[:, :, :b.position], f"{what}: hist below the position")


# ------------------------------------------------------------------------------------------------ 1. exact, empty acc
def test_one_level_on_integers_with_an_empty_accumulator_is_exact():
    """head 8, K 16: one level.  Five steps, then a draft of 8: M = 8, and the late pairs are the samples [0, 8) against
    the taps [8, 16).  No transform has run (``acc`` is all zeros before and after), so every column is exact."""
    B, cin, cout, groups = GROUPED
    x, w, b, _, _, want, base = row(B, cin, cout, groups, 64, 16)
    stream = FFTLongConvStream(w, b, groups, batch=B, max_len=64, head=8)
    for t in range(5):
        stream.step(x[:, :, t].contiguous())
    assert F_._long_spec_plan(5, 8, 8, 16, 0, 64) == (8, [(8, 0, 8, 16)]) and not stream.acc.any()
    y = stream.speculate(x[:, :, 5:13])
    au.check("head 8 K 16, draft (5, 8)", y, want[:, :, 5:13], base[:, :, 5:13], F32, exact=True)
    assert not stream.acc.any() and stream.position == 5
    gu.same_bits(stream.hist[:, :, :13], x[:, :, :13].contiguous(), "hist")
    stream.accept(8)
    assert stream.position == 13 and stream.acc[:, :, 8:].any() and not stream.acc[:, :, :8].any()


# ------------------------------------------------------------------------------------------------ 2. the grid
GRID = [(17, 1), (17, 7), (17, 8), (24, 8), (60, 8), (61, 8), (121, 8), (125, 8), (248, 8), (250, 6)]


@pytest.mark.parametrize("layer", [GROUPED, WIDE_GROUPS], ids=["grouped", "six-outputs-per-group"])
@pytest.mark.parametrize("p,T", GRID, ids=["p%d-T%d" % d for d in GRID])
def test_every_way_a_draft_can_meet_the_grid(layer, p, T):
    """head 8, K 100: levels 8, 16, 32 and 64, the top one cut at the taps; max_len 256; a prefill of 13 leaves partial
    blocks (M - n < first).  (125, 8): M = 128, all four levels; (248, 8) ends at max_len; (250, 6): M = max_len is not due."""
    B, cin, cout, groups = layer
    assert F_._long_spec_plan(125, 8, 8, 100, 13, 256)[1][-1] == (64, 64, 64, 100)
    assert F_._long_spec_plan(61, 8, 8, 100, 13, 256)[1][-1] == (64, 13, 64, 100)
    draft(f"draft ({p}, {T})", row(B, cin, cout, groups, 256, 100), groups, 8, 256, 13, p, T)


# ------------------------------------------------------------------------------------------------ 3. accept
@pytest.mark.parametrize("p,T", [(61, 8), (125, 8)])
def test_accept_leaves_the_state_of_a_push_of_the_accepted_tokens(p, T, library_calls):
    B, cin, cout, groups = GROUPED
    tensors = row(B, cin, cout, groups, 256, 100)
    x = tensors[0]
    M = F_._long_spec_plan(p, T, 8, 100, 13, 256)[0]
    for a in sorted({min(max(a, 0), T) for a in (0, 1, M - p - 1, M - p, M - p + 1, T)}):
        spec, twin = (bring(tensors[1], tensors[2], groups, B, 256, 8, x, p, 13) for _ in range(2))
        spec.speculate(x[:, :, p:p + T])
        del library_calls[:]
        assert spec.accept(a) is None and spec._draft is None
        assert not {"long_step", "long_push", "long_spec"} & set(library_calls), library_calls
        assert ran_blocks(library_calls) == (M <= p + a), (a, library_calls)      # the blocks run iff M was passed
        if a:
            twin.push(x[:, :, p:p + a])
        state_equal(f"accept({a}) of ({p}, {T})", spec, twin)
        for t in range(p + a, p + a + 20):
            col = x[:, :, t].contiguous()
            gu.same_bits(spec.step(col), twin.step(col), f"step {t} after accept({a}) of ({p}, {T})")
        state_equal(f"20 steps after accept({a}) of ({p}, {T})", spec, twin)


def test_ten_rounds_of_speculate_and_accept():
    """Speculate 8, accept a seeded 0 ... 8 of them, ten times over, next to a twin that pushes the accepted tokens only:
    the same state bit for bit at the end, and the accepted columns within the bound of the truth."""
    B, cin, cout, groups = GROUPED
    x, w, b, _, _, want, base = row(B, cin, cout, groups, 256, 100)
    spec, twin = (bring(w, b, groups, B, 256, 8, x, 13, 13) for _ in range(2))
    rng = np.random.default_rng(5)
    out = torch.empty((B, cout, 256), dtype=F32, device=DEV)
    counts = []
    for _ in range(10):
        p = spec.position
        y = spec.speculate(x[:, :, p:p + 8])
        a = int(rng.integers(0, 9))
        counts.append(a)
        spec.accept(a)
        out[:, :, p:p + a] = y[:, :, :a]
        if a:
            twin.push(x[:, :, p:p + a])
    end = spec.position
    assert end == 13 + sum(counts) and 0 in counts and 8 in counts and end > 13 + 24, counts
    state_equal("after ten rounds", spec, twin)
    au.check("the accepted columns of ten rounds", out[:, :, 13:end], want[:, :, 13:end], base[:, :, 13:end], F32)
    for t in range(end, end + 20):
        col = x[:, :, t].contiguous()
        gu.same_bits(spec.step(col), twin.step(col), f"step {t} after the rounds")


# ------------------------------------------------------------------------------------------------ 4. a poisoned draft
def test_a_poisoned_draft_leaves_no_trace():
    """A draft full of inf and nan, rejected whole; then real tokens by ``step`` and ``push`` past the next two multiples
    of the top level (128 and 192): every output and ``acc`` have the bits of a twin that never speculated."""
    B, cin, cout, groups = GROUPED
    x, w, b, _, _, _, _ = row(B, cin, cout, groups, 256, 100)
    spec, twin = (bring(w, b, groups, B, 256, 8, x, 61, 13) for _ in range(2))
    poison = torch.full((B, cin, 8), float("inf"), dtype=F32, device=DEV)
    poison[:, :, ::2] = float("nan")
    poison[:, 1::2] *= -1
    y = spec.speculate(poison)
    assert not au.finite(y) and not au.finite(spec.hist[:, :, 61:69]) and au.finite(spec.acc)
    spec.accept(0)
    assert spec.position == 61
    for s in (spec, twin):
        s.outs = [s.step(x[:, :, t].contiguous()) for t in range(61, 70)]
        s.outs += [s.push(x[:, :, 70:130]), s.push(x[:, :, 130:200])]
    for i, (got, ref) in enumerate(zip(spec.outs, twin.outs)):
        assert au.finite(got)
        gu.same_bits(got, ref, f"output {i} after the rejected draft")
    assert spec.position == twin.position == 200
    gu.same_bits(spec.acc, twin.acc, "acc")
    gu.same_bits(spec.hist, twin.hist, "hist")


# ------------------------------------------------------------------------------------------------ 5. more than one tile
@pytest.mark.parametrize("p,T", [(200, 128), (250, 128)])
def test_two_tiles_and_late_runs_longer_than_a_tile(p, T):
    """head 128, K 300 (levels 128 and 256), max_len 700: M = 256 lies inside the first tile of 64 columns, and the second
    tile's columns have up to 72 (p = 200) late terms per level."""
    layer = (2, 2, 2, 2)
    B, cin, cout, groups = layer
    assert F_._long_spec_plan(p, T, 128, 300, 13, 700) == (256, [(128, 128, 128, 256), (256, 13, 256, 300)])
    draft(f"head 128, draft ({p}, {T})", row(B, cin, cout, groups, 700, 300), groups, 128, 700, 13, p, T)


# ------------------------------------------------------------------------------------------------ 6. LDS blocks
def test_input_channels_beyond_one_lds_block():
    """head 1024: one channel's staged samples take 4348 bytes, so one 32 KiB block holds 7 of the 9 input channels and
    the staging runs twice per round of outputs.  Draft (1000, 100): M = 1024, one level (1024, taps 1024 ... 1500)."""
    B, cin, cout, groups = 1, 9, 2, 1
    assert 32 * 1024 // ((64 + 1024 - 1) * 4) == 7 < cin
    assert F_._long_spec_plan(1000, 100, 1024, 1500, 13, 2304) == (1024, [(1024, 13, 1024, 1500)])
    draft("head 1024, nine channels, draft (1000, 100)", row(B, cin, cout, groups, 2304, 1500), groups, 1024, 2304, 13, 1000, 100)


# ------------------------------------------------------------------------------------------------ 7. gates
@functools.lru_cache(maxsize=None)
def gated_row(which):
    """The (125, 8) layer with gates that are all ones on the prefill's 13 columns (a prefill is ungated)."""
    B, cin, cout, groups = GROUPED
    x, w, b, pre, post, _, _ = row(B, cin, cout, groups, 256, 100, True)
    pre, post = pre.clone(), post.clone()
    pre[:, :, :13] = 1.0
    post[:, :, :13] = 1.0
    pre, post = (pre if which != "postgate" else None), (post if which != "pregate" else None)
    return x, w, b, pre, post, exact_causal(x, w, b, groups, pre, post), fft_baseline(x, w, b, groups, pre, post)


@pytest.mark.parametrize("which", ["both", "pregate", "postgate"])
def test_gates(which):
    """Gated bring-up, then the gated (125, 8) draft: within the bound of the gated truth, the columns below M = 128 with
    the bits of the gated push, ``hist`` = pregate * x."""
    draft(f"gates: {which}, draft (125, 8)", gated_row(which), GROUPED[3], 8, 256, 13, 125, 8)


# ------------------------------------------------------------------------------------------------ 8. 16-bit streams
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["float16", "bfloat16"])
def test_16_bit_drafts_have_the_bits_of_the_widened_float32_stream(dtype):
    """Every column of ``speculate``: the float32 stream's on the widened tensors, rounded once with ``.to(dtype)``; the
    state after ``accept`` is the same float32 state."""
    B, cin, cout, groups = GROUPED
    x, w, b, pre, post = normal_row(B, cin, cout, groups, 256, 100, dtype)
    wide_of = lambda t: None if t is None else t.float()      # noqa: E731
    half = bring(w, b, groups, B, 256, 8, x, 125, 13)
    wide = bring(w.float(), b.float(), groups, B, 256, 8, x.float(), 125, 13)
    state_equal(f"{dtype} before the drafts", half, wide)
    for T, gated, a in ((8, True, 5), (8, False, 0), (6, True, 6), (8, True, 8)):
        p = half.position
        chunk = [cut(t, p, p + T).contiguous() if gated or t is x else None for t in (x, pre, post)]
        y = half.speculate(*chunk)
        ref = wide.speculate(*(wide_of(t) for t in chunk))
        assert y.dtype == dtype and ref.dtype == F32
        gu.same_bits(y, ref.to(dtype), f"{dtype} draft of {T} at {p}")
        half.accept(a)
        wide.accept(a)
        state_equal(f"{dtype} after accept({a}) at {p}", half, wide)
    assert half.position == 125 + 19 and half.hist.dtype == half.acc.dtype == F32


# ------------------------------------------------------------------------------------------------ 9. memory discipline
def test_a_draft_writes_its_columns_of_hist_and_its_own_output(library_calls):
    """Every tensor the call is given lies between NaN-filled guard bands, y is served poisoned: nothing outside y and
    ``hist[..., p:p + T]`` changes, every sample of y is written, a second run from the same state has the same bits,
    ``speculate`` is ONE library call and ``accept`` makes none of the step, the push or the draft."""
    B, cin, cout, groups = GROUPED
    x, w, b, pre, post, _, _ = gated_row("both")
    p, T = 125, 8
    stream = bring(w, b, groups, B, 256, 8, x, p, 13, pre)
    checks = {}
    for name in ("hist", "acc", "_flipped", "_head_taps", "_bias"):
        view, checks[name] = gu.guarded(getattr(stream, name), 0xFF)
        setattr(stream, name, view)
    chunk = []
    for name, t in (("x", x), ("pregate", pre), ("postgate", post)):
        view, checks[name] = gu.guarded(t[:, :, p:p + T], 0xFF, offset=1)      # (only element-aligned)
        chunk.append(view)
    hist, acc = stream.hist.clone(), stream.acc.clone()
    del library_calls[:]
    with gu.guarded_empty(0xFF) as guard:
        y = stream.speculate(*chunk)
    assert library_calls == ["long_spec"], library_calls
    assert guard.violations() == [] and guard.served == [((B, cout, T), F32)]
    assert au.finite(y), "a sample of y was not written"
    for name, check in checks.items():
        found = check()
        if name == "hist":                               # its payload changes, in the draft's columns only (below)
            found = [v for v in found if v[2] != "payload"]
        assert found == [], (name, found)
    gu.same_bits(stream.acc, acc, "acc")
    gu.same_bits(stream.hist[:, :, :p], hist[:, :, :p], "hist below the draft")
    gu.same_bits(stream.hist[:, :, p + T:], hist[:, :, p + T:], "hist behind the draft")
    gu.same_bits(stream.hist[:, :, p:p + T], (pre * x)[:, :, p:p + T].contiguous(), "hist of the draft: pregate * x")
    assert stream.position == p
    again = stream.speculate(*chunk)
    gu.same_bits(again, y, "a second draft from the same state")
    del library_calls[:]
    stream.accept(T)
    assert not {"long_step", "long_push", "long_spec"} & set(library_calls) and ran_blocks(library_calls), library_calls
    assert "transform_kernel" not in library_calls, "a spectrum was made again"
    assert stream.position == p + T


def test_a_refused_draft_touches_nothing(library_calls):
    B, cin, cout, groups = GROUPED
    x, w, b, _, _, _, _ = row(B, cin, cout, groups, 256, 100)
    stream = bring(w, b, groups, B, 60, 8, x, 55, 13)
    stream.speculate(x[:, :, 55:58])
    hist, acc, calls = stream.hist.clone(), stream.acc.clone(), len(library_calls)
    with pytest.raises(ValueError, match="T = 9 tokens exceeds head = 8"):
        stream.speculate(x[:, :, 55:64])
    with pytest.raises(RuntimeError, match="T = 8 tokens at position p = 55 passes max_len = 60"):
        stream.speculate(x[:, :, 55:63])
    with pytest.raises(ValueError, match="`x` must have shape"):
        stream.speculate(x[:, :1, 55:58])
    with pytest.raises(ValueError, match="count must lie in"):
        stream.accept(4)
    assert len(library_calls) == calls and stream.position == 55 and stream._draft == (55, 3)
    gu.same_bits(stream.hist, hist, "hist after the refused calls")
    gu.same_bits(stream.acc, acc, "acc after the refused calls")
    stream.accept(3)
    assert stream.position == 58
    with pytest.raises(RuntimeError, match="without a pending draft"):
        stream.accept(0)
    stream.speculate(x[:, :, 58:60])                  # up to max_len exactly
    stream.accept(2)
    assert stream.position == 60


# ------------------------------------------------------------------------------------------------ 10. head only
@pytest.mark.parametrize("K", [5, 16])
def test_head_only_drafts_have_the_bits_of_the_push(K, library_calls):
    """K <= head: no level exists, so a draft is the push on every column, M or not, and ``accept`` runs no block."""
    B, cin, cout, groups = GROUPED
    tensors = row(B, cin, cout, groups, 130, K)
    spec, twin, y, M = draft(f"head only K={K}, draft (21, 16)", tensors, groups, 16, 130, 0, 21, 16, exact=True)
    assert M == 32 and spec._levels == {} and F_._long_spec_plan(21, 16, 16, K, 0, 130) == (32, [])
    del library_calls[:]
    spec.accept(16)
    assert library_calls == [] and spec.position == 37 and not spec.acc.any()
    state_equal("head only after accept", spec, twin)
