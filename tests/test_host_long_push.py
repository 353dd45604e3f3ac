"""``FFTLongConvStream.push`` without a device: the push schedule (``functional._long_push_plan``, the only place it lives)
against brute force and against ``np.convolve`` under seeded cuts of a row into pushes, the pinned plans, every argument
error of ``push`` (raised before anything touches the library, the position unchanged), and the C ABI of ``fc_long_push``
(declared, exported directly after ``fc_long_step``, ABI 7, its error codes, all of which come back before a launch)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fft_conv_pytorch_amd import FFTLongConvStream, _native
from fft_conv_pytorch_amd import functional as F_
from tests.test_host_long_stream import SCHEDULES as STREAM_SCHEDULES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (L, K, U, L0): row length, taps, head, prefill
SCHEDULES = list(STREAM_SCHEDULES) + [(300, 40, 16, 0)]
IDS = ["L%d-K%d-U%d-L0_%d" % s for s in SCHEDULES]
CUTS = 12


def cuts(L, U, L0, seed):
    """One seeded cut of the columns [L0, L) into pushes: (position, tokens) in order."""
    rng = np.random.default_rng(seed)
    sizes = [1, 3, U - 1, U, U + 1, 2 * U, 5 * U + 3, 8 * U, None]      # None: the rest
    out, p = [], L0
    while p < L:
        T = sizes[rng.integers(len(sizes))]
        T = L - p if T is None else min(T, L - p)
        out.append((p, T))
        p += T
    return out


def row_ops(L, K, U, L0, seed, bulk=True):
    """The ops of the whole row under one cut, each with the number of samples delivered when it runs (the end of its push)."""
    ops = []
    for p, T in cuts(L, U, L0, seed):
        ops += [(op, p, p + T) for op in F_._long_push_plan(p, T, U, K, L0, bulk)]
    return ops


# ------------------------------------------------------------------------------------------------ coverage
@pytest.mark.parametrize("bulk", [True, False], ids=["bulk", "windows-only"])
@pytest.mark.parametrize("L,K,U,L0", SCHEDULES, ids=IDS)
def test_every_pair_is_covered_once_and_in_time(L, K, U, L0, bulk):
    t, k = np.meshgrid(np.arange(L), np.arange(K), indexing="ij")
    needed = (t >= L0) & (k >= U) & (t + k < L)
    for seed in range(CUTS):
        count = np.zeros((L, K), dtype=np.int64)
        emitted = L0                                   # columns below are out: nothing may land on them any more
        for op, p, end in row_ops(L, K, U, L0, seed, bulk):
            if op[0] == "window":
                _, at, m = op
                assert at == emitted and m >= 1 and p <= at and at + m <= end      # in order, no gap, inside the chunk
                emitted = at + m
            elif op[0] == "block":
                _, i, n, lo, tap0, tap1, out0 = op
                assert (n, lo, tap0, tap1, out0) in F_._long_stream_blocks(i, U, K, L0)
                assert L0 <= lo < i <= emitted          # reads delivered samples at or past `first` only (from hist)
                assert lo + tap0 >= emitted             # ... and lands on columns not yet emitted
                count[lo:i, tap0:tap1] += 1
            else:
                _, i, n, tap0, tap1 = op
                assert bulk and op[0] == "bulk"
                assert n >= 2 * U and n & (n - 1) == 0 and i % n == 0 and p <= i and i + n <= end and i >= L0
                assert (tap0, tap1) == (U, min(2 * n, K)) and i == emitted
                count[i:i + n, tap0:tap1] += 1
        assert emitted == L
        assert (count[needed] == 1).all(), (seed, int((count[needed] != 1).sum()))
        assert (count[(t < L0) | (k < U)] == 0).all() and count.max() <= 1


def test_bulks_occur_under_the_cuts():
    L, K, U, L0 = SCHEDULES[0]
    assert sum(op[0] == "bulk" for seed in range(CUTS) for op, _, _ in row_ops(L, K, U, L0, seed)) >= 1
    assert not any(op[0] == "bulk" for seed in range(CUTS) for op, _, _ in row_ops(L, K, U, L0, seed, False))


# ------------------------------------------------------------------------------------------------ arithmetic
def _row_by_plan(x, ker, U, L0, seed, bulk):
    """The stream's arithmetic in float64 numpy: blocks, bulks and windows taken from the plan alone."""
    L, K = len(x), len(ker)
    y, acc, hist = np.zeros(L), np.zeros(L + 2 * K), np.zeros(L)
    if L0:
        full = np.convolve(x[:L0], ker)
        y[:L0] = full[:L0]
        acc[L0:L0 + K - 1] += full[L0:]
        hist[:L0] = x[:L0]
    for op, p, end in row_ops(L, K, U, L0, seed, bulk):
        if op[0] == "window":
            _, at, m = op
            hist[at:at + m] = x[at:at + m]
            for t in range(at, at + m):
                y[t] = acc[t] + sum(ker[k] * hist[t - k] for k in range(min(U, K, t - L0 + 1)))
        elif op[0] == "block":
            _, i, n, lo, tap0, tap1, out0 = op
            block = np.convolve(hist[lo:i], ker[tap0:tap1])
            acc[out0:out0 + len(block)] += block
        else:
            _, i, n, tap0, tap1 = op
            block = np.convolve(x[i:i + n], ker[tap0:tap1])          # the chunk's samples: hist does not hold them yet
            acc[i + tap0:i + tap0 + len(block)] += block
    return y


@pytest.mark.parametrize("bulk", [True, False], ids=["bulk", "windows-only"])
@pytest.mark.parametrize("L,K,U,L0", SCHEDULES, ids=IDS)
def test_the_plan_reproduces_np_convolve(L, K, U, L0, bulk):
    rng = np.random.default_rng(L + K + U + L0)
    x, ker = (rng.integers(-8, 9, n).astype(np.float64) for n in (L, K))
    want = np.convolve(x, ker)[:L]
    for seed in range(CUTS):
        assert np.array_equal(_row_by_plan(x, ker, U, L0, seed, bulk), want), seed


# ------------------------------------------------------------------------------------------------ pinned plans
def test_pinned_plans():
    plan = F_._long_push_plan
    assert plan(0, 96, 16, 300, 0) == [("bulk", 0, 64, 16, 128), ("window", 0, 64), ("bulk", 64, 32, 16, 64), ("window", 64, 32)]
    assert plan(37, 100, 16, 300, 37) == [
        ("window", 37, 11),
        ("block", 48, 16, 37, 16, 32, 53),
        ("window", 48, 16),
        ("block", 64, 16, 48, 16, 32, 64), ("block", 64, 32, 37, 32, 64, 69), ("block", 64, 64, 37, 64, 128, 101),
        ("bulk", 64, 64, 16, 128),
        ("window", 64, 64),
        ("block", 128, 128, 37, 128, 256, 165),
        ("window", 128, 9),
    ]
    # a head-only filter: windows only, cut at the multiples of the head
    assert plan(5, 40, 16, 16, 0) == [("window", 5, 11), ("window", 16, 16), ("window", 32, 13)]
    assert plan(0, 64, 16, 5, 0) == [("window", t, 16) for t in (0, 16, 32, 48)]
    # bulk off: the step's own blocks at every multiple of the head
    assert plan(0, 32, 16, 300, 0, bulk=False) == [("window", 0, 16), ("block", 16, 16, 0, 16, 32, 16), ("window", 16, 16),
                                                   ("block", 32, 16, 16, 16, 32, 32), ("block", 32, 32, 0, 32, 64, 32)]
    # n stops doubling once it reaches the taps
    assert plan(0, 300, 16, 40, 0)[:2] == [("bulk", 0, 64, 16, 40), ("window", 0, 64)]


@pytest.mark.parametrize("bulk", [True, False], ids=["bulk", "windows-only"])
@pytest.mark.parametrize("L,K,U,L0", SCHEDULES, ids=IDS)
def test_a_push_runs_the_ops_of_its_plan_in_their_order(L, K, U, L0, bulk):
    """``_run_push`` with its three workers replaced by recorders: what runs is the plan, op for op -- every "block" op
    too, though the push takes those from the blocks due behind a window -- except the blocks at ``max_len``."""
    ran = []
    s = object.__new__(FFTLongConvStream)
    s.batch, s.out_channels, s.dtype, s.device = 1, 1, torch.float32, torch.device("meta")
    s.taps, s.head, s.max_len, s._first = K, U, L, L0
    s._push_window = lambda x, pre, post, y, p, t, m: ran.append(("window", t, m))
    s._run_bulk = lambda x, pre, p, i, n: ran.append(("bulk", i, n))
    s._run_block = lambda i, n, lo: ran.append(("block", i, n, lo))
    for seed in range(CUTS):
        for p, T in cuts(L, U, L0, seed):
            ops = F_._long_push_plan(p, T, U, K, L0, bulk)
            del ran[:]
            s._run_push(ops, None, None, None, p, T)
            assert ran == [op[:4 if op[0] == "block" else 3] for op in ops if op[0] != "block" or op[1] < L], (seed, p, T)


def test_the_switch_is_read_per_call(monkeypatch):
    monkeypatch.delenv("FFTCONV_LONG_PUSH_BULK", raising=False)
    assert F_._long_push_bulk_enabled()
    monkeypatch.setenv("FFTCONV_LONG_PUSH_BULK", "0")
    assert not F_._long_push_bulk_enabled()
    monkeypatch.setenv("FFTCONV_LONG_PUSH_BULK", "1")
    assert F_._long_push_bulk_enabled()


# ------------------------------------------------------------------------------------------------ arguments
@pytest.fixture
def no_library(monkeypatch):
    """Any call into the library (and with it any device call of the package) fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    for name in ("load_library", "long_step", "long_push", "get_plan"):
        monkeypatch.setattr(_native, name, refuse)


def _meta_stream(position=0):
    """A stream that was never constructed on a device: the fields ``push`` reads before its first device call."""
    s = object.__new__(FFTLongConvStream)
    s.batch, s.in_channels, s.out_channels, s.groups = 3, 4, 6, 2
    s.taps, s.head, s.max_len = 100, 16, 50
    s.dtype, s.device = torch.float32, torch.device("meta")
    s._position, s._first = position, 0
    return s


@pytest.mark.parametrize("which", ["x", "pregate", "postgate"])
def test_push_errors_come_before_any_device_call(which, no_library):
    shapes = dict(x=(3, 4, 7), pregate=(3, 4, 7), postgate=(3, 6, 7))
    stream = _meta_stream(11)

    def call(**bad):
        ts = {k: torch.zeros(s, device="meta") for k, s in shapes.items()}      # nothing is allocated anywhere
        ts.update(bad)
        stream.push(ts["x"], ts["pregate"], ts["postgate"])
    with pytest.raises(ValueError, match=f"`{which}` must have shape"):
        call(**{which: torch.zeros(shapes[which][::-1], device="meta")})
    with pytest.raises(ValueError, match=f"`{which}` must have shape"):
        call(**{which: torch.zeros(shapes[which][:2], device="meta")})
    with pytest.raises(TypeError, match=f"`{which}` has dtype"):
        call(**{which: torch.zeros(shapes[which], dtype=torch.bfloat16, device="meta")})
    with pytest.raises(TypeError, match=f"`{which}` must be a tensor"):
        call(**{which: 1.0})
    with pytest.raises(ValueError, match=f"`{which}` is on cpu but the stream is on meta"):
        call(**{which: torch.zeros(shapes[which])})
    assert stream.position == 11


def test_push_refuses_an_empty_chunk_a_missing_x_and_a_chunk_past_max_len(no_library):
    stream = _meta_stream(44)
    with pytest.raises(ValueError, match="T >= 1"):
        stream.push(torch.zeros((3, 4, 0), device="meta"))
    with pytest.raises(TypeError, match="`x` must be a tensor, got NoneType"):
        stream.push(None)
    with pytest.raises(RuntimeError, match="T = 7 tokens at position 44 passes max_len = 50"):
        stream.push(torch.zeros((3, 4, 7), device="meta"))
    assert stream.position == 44


# ------------------------------------------------------------------------------------------------ ABI
def test_the_header_declares_the_push_and_the_library_exports_it():
    text = open(os.path.join(ROOT, "include", "fftconv_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+fc_long_push\s*\(\s*const\s+fc_long_step_desc\s*\*", code)
    assert re.search(r"#define\s+FC_ABI_VERSION\s+7\b", code)
    lib = _native.load_library()
    assert hasattr(lib, "fc_long_push")
    exports = list(_native.EXPORTS)
    assert exports.index("fc_long_push") == exports.index("fc_long_step") + 1
    assert exports[-1] == "fc_long_forward_gated"
    assert lib.fc_version() == 7 == _native.ABI_VERSION
    assert "fc_long_push" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _push_status(desc, t0=0, count=1, first=0, null=False):
    """Status and text of ``fc_long_push`` on host memory that is never dereferenced: every refusal comes before the launch."""
    lib = _native.load_library()
    buf = ctypes.create_string_buffer(64)
    p = None if null else ctypes.addressof(buf)
    st = lib.fc_long_push(ctypes.byref(desc), p, None, None, p, None, p, p, p, t0, count, first, None)
    return st, lib.fc_last_error().decode()


def test_the_push_refuses_bad_calls_without_a_launch():
    ok = dict(batch=2, cin=4, cout=4, groups=2, taps=100, head=16, max_len=50, dtype=0)
    desc = lambda **kw: _native.long_step_desc(**{**ok, **kw})      # noqa: E731
    assert _push_status(desc(), null=True)[0] == _native.FC_ERR_INVALID
    for bad in (dict(batch=0), dict(cin=3), dict(cout=5), dict(groups=0), dict(taps=0), dict(max_len=0), dict(dtype=1),
                dict(dtype=4)):
        assert _push_status(desc(**bad))[0] == _native.FC_ERR_INVALID, bad
    st, text = _push_status(desc(), count=0)
    assert st == _native.FC_ERR_INVALID and "count" in text
    assert _push_status(desc(), count=-3)[0] == _native.FC_ERR_INVALID
    st, text = _push_status(desc(), t0=44, count=7)
    assert st == _native.FC_ERR_INVALID and "max_len" in text
    assert _push_status(desc(), t0=50, count=1)[0] == _native.FC_ERR_INVALID
    assert _push_status(desc(), t0=-1)[0] == _native.FC_ERR_INVALID
    assert _push_status(desc(), t0=5, count=3, first=6)[0] == _native.FC_ERR_INVALID
    assert _push_status(desc(), t0=5, count=3, first=-1)[0] == _native.FC_ERR_INVALID
    for head in (0, 4, 12, 48, 2048):
        st, text = _push_status(desc(head=head))
        assert st == _native.FC_ERR_UNSUPPORTED and "power of two from 8 to 1024" in text, head
    assert _push_status(desc(cin=2, cout=2, groups=1, max_len=1 << 28))[0] == _native.FC_ERR_UNSUPPORTED
    # B * groups * tiles past 2^31 workgroups: 2^20 batch items x 2^11 tiles of 64 columns
    st, text = _push_status(desc(batch=1 << 20, cin=1, cout=1, groups=1, max_len=1 << 17), count=1 << 17)
    assert st == _native.FC_ERR_UNSUPPORTED and "workgroups" in text
