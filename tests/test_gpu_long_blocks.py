"""``fft_long_conv(..., blocks=)`` on the GPU: rows in overlap-save blocks over the long transform -- the blocks builds of
``long_cols_fwd`` and ``long_cols_inv`` (csrc/long1d.hpp) in the forward and in dX, and the weight-gradient plan by blocks.

``blocks=4096`` gives 64 x 64 points, the smallest long plan; other values are stated where used.  Inputs are the integers
of tests/accuracy_util.py, so torch's float64 convolution of them is exact; the bound is ``accuracy_util.check`` with its
standard margins against the model project's formulation in float32.  Every case is the forward plus dX, dW and db against
float64 autograd, and runs between guard bands into NaN-filled and zero-filled buffers.  A truth and a baseline are
computed once per case and shared.

A case is seen through its forward view: the row padded as the call pads it (zeros in front and behind) against the taps
in the order the call reads them (flipped for ``causal``), padding 0 -- what ``accuracy_util`` takes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fft_conv_pytorch_amd import FFTLongConv1d, _native, autograd, fft_long_conv
from fft_conv_pytorch_amd import functional as F_
from tests import accuracy_util as au
from tests import big_util as bu
from tests import guard_util as gu
from tests.route_util import Case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
KNOBS = ("FFTCONV_LONG_DECIM", "FFTCONV_LONG_NLC", "FFTCONV_LONG_N", "FFTCONV_LONG_WS_MB", "FFTCONV_LONG_WGRAD",
         "FFTCONV_HALF_IO", "FFTCONV_TILE")
DIRECT_MAX_TAPS = 1100        # longer filters take the float64 FFT truth (accuracy_util.truth_by_fft)
N = 4096
BIG_L = (1 << 24) + 4096

# name -> (B, Cin, Cout, groups, L, K, padding, causal, blocks)
CASES = {
    "odd-units": (3, 1, 1, 1, 10000, 1000, 0, False, N),        # V 3097, T 3, U 9: the last unit unpaired, a short last block
    "same": (2, 2, 2, 2, 9000, 1500, "same", False, N),         # front zeros in block 0, zeros behind the data in the last
    "causal-half": (2, 1, 1, 1, 12000, 2048, 0, True, N),       # keff = N / 2 exactly
    "one-tap": (1, 1, 1, 1, 9000, 1, 0, False, N),              # V = N, no overlap
    "two-blocks": (1, 1, 1, 1, 7193, 1000, 0, False, N),        # nout = 2 V exactly
    "two-blocks+1": (1, 1, 1, 1, 7194, 1000, 0, False, N),      # nout = 2 V + 1: a one-sample last block
    "grouped": (2, 6, 4, 2, 9000, 700, 0, False, N),
    "8192": (2, 1, 1, 1, 20000, 1500, 0, False, 8192),          # under FFTCONV_LONG_N=64x128
}


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
    """The plans that ran, in order: forward long plans and weight-gradient plans."""
    seen = []
    real, real_lay, real_wg = _native.LongPlan.forward, _native.LongPlan.forward_lay, _native.LongWgradPlan.run

    def forward(plan, *args):
        seen.append(plan)
        return real(plan, *args)

    def forward_lay(plan, *args):
        seen.append(plan)
        return real_lay(plan, *args)

    def run(plan, *args):
        seen.append(plan)
        return real_wg(plan, *args)
    monkeypatch.setattr(_native.LongPlan, "forward", forward)
    monkeypatch.setattr(_native.LongPlan, "forward_lay", forward_lay)
    monkeypatch.setattr(_native.LongWgradPlan, "run", run)
    return seen


def _is_blocks(plan):
    return type(plan) is _native.LongBlocksPlan


def _points(plan):
    return plan.info["N1"] * plan.info["N2"]


def _pads(name):
    B, cin, cout, g, L, K, padding, causal, blocks = CASES[name]
    if causal:
        return K - 1, 0
    if padding == "same":
        return (K - 1) // 2, K - 1 - (K - 1) // 2
    return padding, padding


def _view(name):
    """(the forward view of the case, x -> the padded row, w -> the taps as read)."""
    B, cin, cout, g, L, K, padding, causal, blocks = CASES[name]
    pl, pr = _pads(name)
    view = Case(B, cin, cout, (L + pl + pr,), (K,), g=g, note=name)
    return view, (lambda x: F.pad(x, (pl, pr))), (lambda w: w.flip(-1) if causal else w)


_SHARED = {}


def _data(name, cls="centred"):
    """(x, w, b, gy, exact (y, dX, dW, db), float32 baseline (y, dX, dW, db)) of a case, computed once and left unchanged."""
    key = (name, cls)
    if key not in _SHARED:
        B, cin, cout, g, L, K, padding, causal, blocks = CASES[name]
        pl, pr = _pads(name)
        view, padx, taps = _view(name)
        au.assert_exact(view, cls)
        x, w, b = au.inputs(Case(B, cin, cout, (L,), (K,), g=g), cls, DEV)
        xv, wv = padx(x), taps(w)
        by_fft = K > DIRECT_MAX_TAPS
        want_y = au.truth_by_fft(view, xv, wv, b) if by_fft else au.truth(view, xv, wv, b)
        gy = au.grad_output(want_y.shape, F32, DEV)
        back = lambda dx, dw, db: (dx[..., pl:pl + L], taps(dw), db)      # noqa: E731
        want = (want_y,) + back(*au.truth_grads(view, xv, wv, b, gy, by_fft=by_fft))
        base = au.baseline_grads(view, xv, wv, b, gy)
        _SHARED[key] = (x, w, b, gy, want, (base[0],) + back(*base[1:]))
    return _SHARED[key]


def _call(name, x, w, b, **kw):
    B, cin, cout, g, L, K, padding, causal, blocks = CASES[name]
    kw.setdefault("blocks", blocks)
    return fft_long_conv(x, w, b, padding, g, causal, **kw)


def _guarded_call(name, x, w, b, **kw):
    """The call into NaN-filled and into zero-filled buffers, the inputs between guard bands of their own: no byte outside
    a tensor changes, the inputs keep their bits, the two results agree bit for bit and hold no NaN."""
    outs = []
    for pattern in (0xFF, 0x00):
        held = [gu.guarded(t, pattern, offset=1) for t in (x, w, b)]
        with gu.guarded_empty(pattern) as ge:
            y = _call(name, *(h[0] for h in held), **kw)
        assert ge.violations() == [], f"pattern {pattern:#x}: {ge.violations()}"
        assert ge.served, "no buffer of the call came from torch.empty"
        for what, h in zip("xwb", held):
            assert h[1]() == [], f"pattern {pattern:#x}, {what}: {h[1]()}"
        assert not torch.isnan(y).any(), f"pattern {pattern:#x}: NaN in y"
        outs.append(y)
    gu.same_bits(outs[0], outs[1], "NaN-filled against zero-filled buffers")
    return outs[0]


def _step(fn, x, w, b, gy):
    xs, ws, bs = (t.detach().clone().requires_grad_() for t in (x, w, b))
    y = fn(xs, ws, bs)
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), xs.grad, ws.grad, bs.grad


def _guarded_step(name, x, w, b, gy, **kw):
    """A training step with every buffer of forward and backward between guard bands, NaN-filled then zero-filled."""
    outs = []
    for pattern in (0xFF, 0x00):
        held = [gu.guarded(t, pattern, offset=1) for t in (x, w, b, gy)]
        with gu.guarded_empty(pattern) as ge:
            got = _step(lambda *t: _call(name, *t, **kw), *(h[0] for h in held))
        assert ge.violations() == [], f"pattern {pattern:#x}: {ge.violations()}"
        for what, h in zip(("x", "w", "b", "dY"), held):
            assert h[1]() == [], f"pattern {pattern:#x}, {what}: {h[1]()}"
        outs.append(got)
    for what, a, c in zip(("y", "dX", "dW", "db"), *outs):
        assert not torch.isnan(a).any(), f"NaN in {what}"
        gu.same_bits(a, c, f"{what}: NaN-filled against zero-filled buffers")
    return outs[0]


def _check_all(name, got, want, base, dtype=F32):
    for q, got_, want_, base_ in zip(("y", "dX", "dW", "db"), got, want, base):
        assert got_.shape == want_.shape and got_.dtype == dtype, (q, got_.shape, want_.shape, got_.dtype)
        au.check(f"{name} {q}", got_, want_, base_, F32)


def _assert_step_ran_by_blocks(ran, points):
    """forward, dX (blocks plans of ``points`` points) and dW (the weight-gradient plan by blocks), in that order"""
    assert len(ran) == 3, ran
    assert _is_blocks(ran[0]) and _is_blocks(ran[1]) and type(ran[2]) is _native.LongWgradBlocksPlan, ran
    assert _points(ran[0]) == _points(ran[1]) == ran[2].info["N1"] * ran[2].info["N2"] == points, [p.info for p in ran]


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", ["odd-units", "same", "causal-half", "one-tap", "two-blocks", "two-blocks+1", "grouped"])
def test_forward_and_gradients_against_float64_autograd(name, ran):
    B, cin, cout, g, L, K, padding, causal, blocks = CASES[name]
    x, w, b, gy, want, base = _data(name)
    y = _guarded_call(name, x, w, b)
    assert len(ran) == 2 and ran[0] is ran[1] and _is_blocks(ran[0]) and _points(ran[0]) == N, ran
    plan = ran[0]
    keff = min(K, L) if causal else K
    V = N - keff + 1
    T = -(-want[0].shape[2] // V)
    assert plan.blocks == {"V": V, "T": T, "U": B * T, "pairs": (B * T + 1) // 2}, plan.blocks
    assert plan.out_len == want[0].shape[2] and plan.spectrum_bytes == cout * (cin // g) * N * 8
    au.check(f"{name} y (forward alone)", y, want[0], base[0], F32)
    del ran[:]
    got = _guarded_step(name, x, w, b, gy)
    _assert_step_ran_by_blocks(ran[:3], N)
    _assert_step_ran_by_blocks(ran[3:], N)
    gu.same_bits(got[0], y, "the forward of the training step against the forward alone")
    _check_all(name, got, want, base)


def test_the_geometry_of_the_first_cases():
    """V 3097, T 3, U 9 (odd, the last unit unpaired, a short last block); nout = 2 V and 2 V + 1."""
    geo = lambda name: _native.blocks_geometry(_key(name))      # noqa: E731
    assert {k: geo("odd-units")[k] for k in _native.LONG_BLOCKS_WORDS} == {"V": 3097, "T": 3, "U": 9, "pairs": 5}
    assert geo("two-blocks")["out_len"] == 2 * 3097 and geo("two-blocks")["T"] == 2
    assert geo("two-blocks+1")["out_len"] == 2 * 3097 + 1 and geo("two-blocks+1")["T"] == 3
    assert geo("causal-half")["V"] == N // 2 + 1 and geo("one-tap")["V"] == N


def _key(name):
    B, cin, cout, g, L, K, padding, causal, blocks = CASES[name]
    pl, pr = _pads(name)
    return (B, cin, cout, g, L, K, pl, pr, L if causal else 0, int(causal), 1, blocks)


def test_causal_with_one_tap_more_than_half_a_block_runs_the_plain_plan_with_the_same_values(ran):
    """K 2049 on blocks of 4096 points: not eligible, so the call is the call without the keyword, bit for bit."""
    B, cin, cout, g, L, K, padding, causal, blocks = CASES["causal-half"]
    c = Case(B, cin, cout, (L,), (K + 1,))
    x, w, b = au.inputs(c, "centred", DEV)
    assert F_._long_blocks_route(x.shape, w.shape, causal=True, blocks=N) == "plain"
    got = fft_long_conv(x, w, b, causal=True, blocks=N)
    ref = fft_long_conv(x, w, b, causal=True)
    assert len(ran) == 2 and ran[0] is ran[1] and type(ran[0]) is _native.LongPlan, ran
    gu.same_bits(got, ref, "K = N / 2 + 1 with the keyword against the call without")
    view = Case(B, cin, cout, (L + K,), (K + 1,))
    xv, wv = F.pad(x, (K, 0)), w.flip(-1)
    au.check("causal K 2049", got, au.truth_by_fft(view, xv, wv, b), au.baseline(view, xv, wv, b), F32)


# ------------------------------------------------------------------------------------------------ 16 bits, slabs
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sixteen_bit_results_and_gradients_have_the_bits_of_the_cast_path(dtype, monkeypatch, ran):
    x, w, b, gy, want, base = _data("grouped")
    xh, wh, bh, gyh = (t.to(dtype) for t in (x, w, b, gy))       # (integers up to 8: exact in both formats)
    got = _guarded_step("grouped", xh, wh, bh, gyh)
    _assert_step_ran_by_blocks(ran[:3], N)
    assert all(t.dtype == dtype for t in got)
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    del ran[:]
    ref = _step(lambda *t: _call("grouped", *t), xh, wh, bh, gyh)
    _assert_step_ran_by_blocks(ran, N)                           # (the cast path carries the keyword: the same route)
    for q, a, c in zip(("y", "dX", "dW", "db"), got, ref):
        gu.same_bits(a, c, f"{dtype} {q} against FFTCONV_HALF_IO=0")
    # and they are the float32 results rounded once
    monkeypatch.delenv("FFTCONV_HALF_IO")
    f32 = _step(lambda *t: _call("grouped", *t), x, w, b, gy)
    for q, a, c in zip(("y", "dX", "dW", "db"), got, f32):
        gu.same_bits(a, c.to(dtype), f"{dtype} {q} against the float32 call rounded")


def test_a_workspace_of_one_mebibyte_splits_the_unit_pairs_into_slabs(monkeypatch, ran):
    """FFTCONV_LONG_WS_MB=1 on the grouped case: the slabs run over unit pairs, so the pairs of one batch item land in
    different slabs.  The forward and dX have the bits of the one-slab run (a unit's arithmetic does not depend on its
    slab); dW adds its slabs into W2 and stays inside ``accuracy_util.check``."""
    x, w, b, gy, want, base = _data("grouped")
    one = _step(lambda *t: _call("grouped", *t), x, w, b, gy)
    assert [p.info["slabs"] for p in ran] == [1, 1, 1]
    _clear()
    del ran[:]
    monkeypatch.setenv("FFTCONV_LONG_WS_MB", "1")
    got = _guarded_step("grouped", x, w, b, gy)
    _assert_step_ran_by_blocks(ran[:3], N)
    wg = ran[2]
    assert wg.info["slabs"] >= 2 and wg.info["slab_pairs"] < 3, wg.info       # 3 unit pairs per batch item, 6 units in all
    assert all(p.info["slab_pairs"] * (6 + 4) * N * 8 <= 1 << 20 for p in ran[:2])
    gu.same_bits(got[0], one[0], "y under FFTCONV_LONG_WS_MB=1")
    gu.same_bits(got[1], one[1], "dX under FFTCONV_LONG_WS_MB=1")
    _check_all("grouped, 1 MiB", got, want, base)
    # the forward and dX of that case still fit one slab (three pairs of 320 KiB).  On rows of 12000 samples an item has
    # four units, T = 4: four pairs, three to a slab, so the forward's and dX's second slab begins inside batch item 1
    B, cin, cout, g, L, K, padding, causal, blocks = CASES["grouped"]
    x2 = au.integers((B, cin, 12000), torch.Generator().manual_seed(5), F32, DEV)
    gy2 = au.integers((B, cout, 12000 - K + 1), torch.Generator().manual_seed(6), F32, DEV)
    del ran[:]
    split = _step(lambda *t: fft_long_conv(*t, groups=g, blocks=N), x2, w, b, gy2)
    assert [p.info["slabs"] for p in ran] == [2, 2, 2] and ran[0].blocks == {"V": N - K + 1, "T": 4, "U": 8, "pairs": 4}, ran
    monkeypatch.delenv("FFTCONV_LONG_WS_MB")
    _clear()
    whole = _step(lambda *t: fft_long_conv(*t, groups=g, blocks=N), x2, w, b, gy2)
    gu.same_bits(split[0], whole[0], "y in two slabs against one")
    gu.same_bits(split[1], whole[1], "dX in two slabs against one")
    want2 = F.conv1d(x2.double(), w.double(), b.double(), groups=g)
    assert au.is_whole(want2) and au.e_max(split[0], want2) <= 1e-5


def test_a_strided_gradient_is_routed_as_the_forward_routes_a_signal(monkeypatch, ran):
    """dX is the primitive with dY as its signal, so dY's layout is judged by the forward's rule: under FFTCONV_LONG_NLC=0 a
    dY that lies as a (B, L, C) tensor is a tensor to copy, and dX runs by blocks with the bits of the contiguous dY; with
    the channels-last reads on, such a dY is not eligible and dX runs the whole-row plan."""
    x, w, b, gy, want, base = _data("grouped")
    gy_cl = gy.transpose(1, 2).contiguous().transpose(1, 2)
    assert F_._long_layout(gy_cl) == "nlc"
    ref = _step(lambda *t: _call("grouped", *t), x, w, b, gy)
    del ran[:]
    monkeypatch.setenv("FFTCONV_LONG_NLC", "0")
    got = _step(lambda *t: _call("grouped", *t), x, w, b, gy_cl)
    _assert_step_ran_by_blocks(ran, N)
    for q, a_, c_ in zip(("y", "dX", "dW", "db"), got, ref):
        gu.same_bits(a_, c_, f"{q} from a strided dY under FFTCONV_LONG_NLC=0")
    monkeypatch.delenv("FFTCONV_LONG_NLC")
    del ran[:]
    got = _step(lambda *t: _call("grouped", *t), x, w, b, gy_cl)
    assert _is_blocks(ran[0]) and type(ran[1]) is _native.LongPlan and type(ran[2]) is _native.LongWgradBlocksPlan, ran
    _check_all("grouped, channels-last dY", got, want, base)


# ------------------------------------------------------------------------------------------------ block bounds
IMPULSE_TOL = 1e-3


def test_impulses_on_both_sides_of_every_block_bound_give_exact_outputs(ran):
    """The first case with x and dY reduced to impulses at t V - 1, t V and t V + 1 for every block bound t V: every
    sample of y, dX, dW and db is the exact integer up to the float32 transform's rounding -- within IMPULSE_TOL of it, so
    that rounding to the nearest integer gives the truth itself -- and the bounds of ``accuracy_util.check`` hold.

    IMPULSE_TOL = 1e-3 of a unit, from the number format: a cyclic convolution of a and b through float32 transforms of N
    points has an error of about eps sqrt(log2 N) |a| |b| / sqrt(N) per sample (rms; |.| the 2-norm).  Here a block holds at
    most six impulses of at most 17 (|a| <= 42), the filter 1000 taps of at most 8 (|b| <= 253), N = 4096, eps = 2**-23:
    7e-5 rms for y and dX (less for dW, whose operands are both impulses); the largest of some 3e4 samples lies near 4.5
    times the rms, and 1e-3 leaves a factor of three over that."""
    name = "odd-units"
    B, cin, cout, g, L, K, padding, causal, blocks = CASES[name]
    x0, w, b, gy0, _, _ = _data(name)
    V, nout = N - K + 1, L - K + 1
    at = [t * V + e for t in range(1, -(-nout // V)) for e in (-1, 0, 1)]
    x, gy = torch.zeros_like(x0), torch.zeros_like(gy0)
    x[..., at], gy[..., at] = x0[..., at] + 9, gy0[..., at] + 9      # (integers 1 ... 17: none is zero)
    c = Case(B, cin, cout, (L,), (K,), g=g)
    want = (au.truth(c, x, w, b),) + au.truth_grads(c, x, w, b, gy)
    base = au.baseline_grads(c, x, w, b, gy)
    got = _guarded_step(name, x, w, b, gy)
    _assert_step_ran_by_blocks(ran[:3], N)
    _check_all("impulses", got, want, base)
    for q, got_, want_ in zip(("y", "dX", "dW", "db"), got, want):
        worst = (got_.double() - want_.to(got_.device)).abs().max().item()
        print(f"    impulses {q}: max|got - truth| = {worst:.3e}")
        assert au.is_whole(want_) and worst <= IMPULSE_TOL, (q, worst)
        assert torch.equal(got_.double().round(), want_.to(got_.device)), q


# ------------------------------------------------------------------------------------------------ another N
def test_blocks_of_8192_points_under_a_forced_factorisation(monkeypatch, ran):
    monkeypatch.setenv("FFTCONV_LONG_N", "64x128")
    x, w, b, gy, want, base = _data("8192")
    got = _guarded_step("8192", x, w, b, gy)
    _assert_step_ran_by_blocks(ran[:3], 8192)
    assert all((p.info["N1"], p.info["N2"]) == (64, 128) for p in ran), [p.info for p in ran]
    assert ran[0].blocks == {"V": 8192 - 1500 + 1, "T": 3, "U": 6, "pairs": 3}
    _check_all("blocks of 8192", got, want, base)


# ------------------------------------------------------------------------------------------------ module
def test_module_cache_invalidation_and_graph_capture(monkeypatch, ran):
    B, cin, cout, g, L, K, padding, causal, blocks = CASES["grouped"]
    torch.manual_seed(0)
    ref = torch.nn.Conv1d(cin, cout, K, groups=g)
    layer = FFTLongConv1d(cin, cout, K, groups=g, blocks=N)
    assert layer.blocks == N and "blocks=4096" in repr(layer)
    assert set(layer.state_dict()) == set(ref.state_dict())
    layer.load_state_dict(ref.state_dict())
    layer = layer.to(DEV).eval()
    x = au.integers((B, cin, L), torch.Generator().manual_seed(3), F32, DEV)
    calls = []
    real = F_.transform_kernel
    monkeypatch.setattr(F_, "transform_kernel", lambda plan, kernel: calls.append(plan) or real(plan, kernel))
    with torch.no_grad():
        y1, y2 = layer(x), layer(x)
    assert len(calls) == 1 and _is_blocks(calls[0]), calls                  # one transform for two calls
    assert len(ran) == 2 and ran[0] is ran[1] is calls[0]
    want = ref.double()(x.double().cpu())
    assert y1.shape == want.shape and au.e_max(y1.cpu(), want.detach()) <= 1e-5 and torch.equal(y1, y2)
    gu.same_bits(y1, fft_long_conv(x, layer.weight.detach(), layer.bias.detach(), groups=g, blocks=N), "module against the functional")
    assert len(calls) == 2
    layer.invalidate_kernel_spectrum()
    with torch.no_grad():
        y3 = layer(x)
    assert len(calls) == 3 and torch.equal(y3, y1)

    # a warm call captures and replays with the eager call's bits
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
BIG = Case(1, 1, 1, (BIG_L,), (1000,), note="past-2^24")


BIG_V = (1 << 18) - 999       # kept samples per block of the planner's choice, 2**18 points against 1000 taps


def _sparse(length, seed):
    """``big_util.sparse_input`` of a (1, 1, length) row, plus a window on both sides of every block bound t * BIG_V."""
    xs = bu.sparse_input((1, 1, length), 4, seed=seed, tile=BIG_V, reach=1000)
    at = torch.arange(BIG_V, length - 2, BIG_V)[:, None] + torch.arange(-2, 2)[None]
    vals = au.integers((at.numel(),), torch.Generator().manual_seed(seed + 100), torch.float64).numpy().copy()
    vals[vals == 0] = au.HI
    return bu.Sparse(xs.shape, np.concatenate([xs.flat, at.reshape(-1).numpy()]), np.concatenate([xs.val, vals]))


def _big_inputs():
    xs = _sparse(BIG_L, 41)
    w = au.integers((1, 1, 1000), torch.Generator().manual_seed(42), F32, DEV)
    b = au.integers((1,), torch.Generator().manual_seed(43), F32, DEV)
    return xs, xs.dense(F32, DEV), w, b


def test_a_row_past_the_limit_raises_without_the_keyword_and_runs_with_it(ran):
    """B1 1 -> 1, L = 2**24 + 4096, K 1000, float32: every sample of y against the exact sparse truth."""
    xs, x, w, b = _big_inputs()
    with pytest.raises(NotImplementedError, match=r"2\*\*24"):
        fft_long_conv(x, w, b)
    assert ran == []
    with gu.guarded_empty(0xFF) as ge:
        y = fft_long_conv(x, w, b, blocks=True)
    assert ge.violations() == [], ge.violations()
    assert len(ran) == 1 and _is_blocks(ran[0]) and 4 * 1000 <= _points(ran[0]) <= F_.LONG_MAX_POINTS, ran
    assert ran[0].blocks["V"] == BIG_V and ran[0].blocks["T"] == 65 and y.shape == (1, 1, BIG_L - 999)
    flat, val = bu.conv_truth(BIG, xs, w.cpu().double().numpy())
    bu.check_full(y, flat, val, b.cpu().double().numpy(), what="y past 2**24 points")


def _windows(shape, seed, extra):
    """``big_util.sparse_input`` of a (1, 1, n) row plus windows of four samples that start at the positions ``extra``."""
    xs = bu.sparse_input(shape, 4, seed=seed, tile=BIG_V, reach=3)
    at = (torch.tensor(extra)[:, None] + torch.arange(4)[None]).reshape(-1).numpy()
    vals = au.integers((at.size,), torch.Generator().manual_seed(seed + 100), torch.float64).numpy().copy()
    vals[vals == 0] = au.HI
    return bu.Sparse(shape, np.concatenate([xs.flat, at]), np.concatenate([xs.val, vals]))


def test_zero_padding_wider_than_the_longest_transform(ran):
    """B1 1 -> 1, L 300000, K 3, padding 2**24 + 8 on both sides, ``blocks=True``: the data begins past position 2**24 of
    the padded row, in block 64 of 130, and a block bound (65 V) falls inside it.  The place of the data is a number like
    any other: y (every sample: the bias over the paddings, the convolution between them), dX, dW and db against exact
    sparse truths.  dX's own row is short and runs the whole-row plan; dW runs the weight-gradient plan by blocks."""
    L, K, p = 300000, 3, (1 << 24) + 8
    V = (1 << 18) - K + 1
    c = Case(1, 1, 1, (L,), (K,), p=p, note="wide-padding")
    nout = L + 2 * p - K + 1
    bound = 65 * V                                       # a block bound in y's (= the padded row's) coordinates
    assert p < bound - 8 and bound + 8 < p + L - K
    xs = _windows((1, 1, L), 51, [bound - p - 2, bound - p + V // 8, 1000])
    dys = _windows((1, 1, nout), 52, [p - 2, p + 1, bound - 2, bound + V // 8, p + L - K - 1, 64 * V - 2, 1 << 24])
    x, gy = xs.dense(F32, DEV), dys.dense(F32, DEV)
    w = au.integers((1, 1, K), torch.Generator().manual_seed(53), F32, DEV) + 9        # (no zero tap)
    b = au.integers((1,), torch.Generator().manual_seed(54), F32, DEV) + 9
    assert F_._long_blocks_route(x.shape, w.shape, padding=p, blocks=True) == "blocks"
    with pytest.raises(NotImplementedError, match=r"2\*\*24"):
        fft_long_conv(x, w, b, p)
    with gu.guarded_empty(0xFF) as ge:
        y, dx, dw, db = _step(lambda *t: fft_long_conv(*t, p, blocks=True), x, w, b, gy)
    assert ge.violations() == [], ge.violations()
    assert len(ran) == 3 and _is_blocks(ran[0]) and type(ran[1]) is _native.LongPlan, ran
    assert type(ran[2]) is _native.LongWgradBlocksPlan and ran[0].blocks == {"V": V, "T": 130, "U": 130, "pairs": 65}
    wn = w.cpu().double().numpy()
    flat, val = bu.conv_truth(c, xs, wn)
    assert flat.size and flat.min() >= p - K + 1            # (the truth has the data where the padding ends)
    bu.check_full(y, flat, val, b.cpu().double().numpy(), what="y behind a padding of 2**24 + 8")
    ct = Case(1, 1, 1, (nout,), (K,), p=p, tr=True)
    assert au.out_spatial(ct) == (L,)
    flat, val = bu.conv_truth(ct, dys, wn)
    bu.check_full(dx, flat, val, what="dX")
    flat, val = bu.wgrad_truth(c, xs, dys)
    assert flat.size and np.abs(val).max() > 0               # (windows of x and of dY meet: dW is not zero)
    bu.check_full(dw.contiguous()[None], flat, val, what="dW")
    bu.check_full(db.contiguous()[None, :, None], [0], bu.bias_grad_truth(dys), what="db")


# ------------------------------------------------------------------------------------------------ what a blocks plan refuses
def test_a_blocks_plan_is_a_real_plan_and_refuses_layouts_and_gates_without_a_launch():
    B, cin, cout, g, L, K, padding, causal, blocks = CASES["grouped"]
    x, w, b, gy, want, base = _data("grouped")
    plan = F_._long_blocks_plan(x, cout, g, K, 0, 0, False, 0, True, N)
    assert _is_blocks(plan) and plan.kind == _native.LONG_REAL and not plan.complex
    spectrum = F_.transform_kernel(plan, w)
    ws = F_.new_workspace(plan, x.device)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.full((B, cout, plan.out_len), float("nan"), device=DEV)
    args = (x.data_ptr(), spectrum.buf.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), stream, 0, 0)
    for lay in ((_native.LONG_NLC, _native.LONG_NCL), (_native.LONG_NCL, _native.LONG_NLC), (_native.LONG_NLC, _native.LONG_NLC)):
        with pytest.raises(NotImplementedError, match="blocks plan reads and writes"):
            plan.forward_lay(*args, *lay)
    with pytest.raises(NotImplementedError, match="takes no blocks plan"):
        plan.forward_gated(*args, pregate_ptr=x.data_ptr())
    with pytest.raises(NotImplementedError, match="takes no blocks plan"):
        plan.forward_gated(*args, gate_ptr=out.data_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call launched"
    plan.forward_lay(*args, _native.LONG_NCL, _native.LONG_NCL)
    torch.cuda.synchronize()
    au.check("blocks plan through forward_lay", out, want[0], base[0], F32)
    # the weight-gradient plan by blocks: no gate, no channels-last operand
    wkey = F_._long_wgrad_key(B, cin, cout, g, L, K, 0, 0, plan.out_len, False, 0, 1, 1) + (N,)
    wplan = F_._cached_plan(0, ("long_wgrad_blocks",) + wkey)
    wws = F_.new_workspace(wplan, x.device)
    dw = torch.full(tuple(w.shape), float("nan"), device=DEV)
    with pytest.raises(NotImplementedError, match="no gate on a blocks plan"):
        wplan.run_gated(x.data_ptr(), x.data_ptr(), gy.data_ptr(), None, dw.data_ptr(), wws.data_ptr(), stream)
    with pytest.raises(NotImplementedError, match="no gate on a blocks plan"):
        wplan.run_gated(x.data_ptr(), None, gy.data_ptr(), gy.data_ptr(), dw.data_ptr(), wws.data_ptr(), stream)
    for lay in ((_native.LONG_NLC, _native.LONG_NCL), (_native.LONG_NCL, _native.LONG_NLC)):
        with pytest.raises(NotImplementedError, match="by blocks reads"):
            wplan.run(x.data_ptr(), gy.data_ptr(), dw.data_ptr(), wws.data_ptr(), stream, 0, 0, 0, *lay)
    torch.cuda.synchronize()
    assert torch.isnan(dw).all(), "a refused call launched"
    wplan.run(x.data_ptr(), gy.data_ptr(), dw.data_ptr(), wws.data_ptr(), stream)
    torch.cuda.synchronize()
    au.check("weight-gradient plan by blocks, called directly", dw, want[2], base[2], F32)


def test_a_row_past_the_limit_trains(ran):
    """The training step of the same row from a sparse x and a sparse dY: dX, dW and db against exact sparse truths."""
    xs, x, w, b = _big_inputs()
    nout = BIG_L - 999
    dys = _sparse(nout, 44)
    gy = dys.dense(F32, DEV)
    with gu.guarded_empty(0xFF) as ge:
        y, dx, dw, db = _step(lambda *t: fft_long_conv(*t, blocks=True), x, w, b, gy)
    assert ge.violations() == [], ge.violations()
    assert len(ran) == 3 and _is_blocks(ran[0]) and _is_blocks(ran[1]) and type(ran[2]) is _native.LongWgradBlocksPlan, ran
    assert all(p.info["N1"] * p.info["N2"] <= F_.LONG_MAX_POINTS for p in ran)
    wn = w.cpu().double().numpy()
    flat, val = bu.conv_truth(BIG, xs, wn)
    bu.check_full(y, flat, val, b.cpu().double().numpy(), what="y")
    ct = Case(1, 1, 1, (nout,), (1000,), tr=True)
    assert au.out_spatial(ct) == (BIG_L,)
    flat, val = bu.conv_truth(ct, dys, wn)
    bu.check_full(dx, flat, val, what="dX")
    flat, val = bu.wgrad_truth(BIG, xs, dys)
    bu.check_full(dw.contiguous()[None], flat, val, what="dW")
    bu.check_full(db.contiguous()[None, :, None], [0], bu.bias_grad_truth(dys), what="db")
