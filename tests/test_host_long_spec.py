"""``FFTLongConvStream.speculate`` / ``accept`` without a device: the draft's schedule (``functional._long_spec_plan``, the
only place it lives) against ``np.convolve`` at every position of every stream schedule, the pinned plans, every argument
error of the two methods (raised before anything touches the library, position and pending draft unchanged), and the C
ABI of ``fc_long_spec`` (declared, exported, ABI 7, its error codes, all of which come back before a launch)."""
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

# (L, K, U, L0): row length = max_len, taps, head, prefill
SCHEDULES = list(STREAM_SCHEDULES) + [(256, 100, 8, 13)]
IDS = ["L%d-K%d-U%d-L0_%d" % s for s in SCHEDULES]


# ------------------------------------------------------------------------------------------------ the schedule
@pytest.mark.parametrize("L,K,U,L0", SCHEDULES, ids=IDS)
def test_the_draft_schedule_reproduces_np_convolve_at_every_position(L, K, U, L0):
    """The stream in float64 numpy on integers, its blocks taken from ``_long_stream_blocks`` as a step runs them.  At
    every position p >= L0 a draft of T = min(head, L - p) tokens is evaluated from the state as it stands -- ``acc``, the
    head pairs, and the late pairs of ``_long_spec_plan`` -- and every column equals ``np.convolve``.  The late samples
    are old ones (below p) at or past max(M - n, first), and no output has more than (T - 1) * levels late pairs."""
    rng = np.random.default_rng(L + K + U + L0)
    x, ker = (rng.integers(-8, 9, n).astype(np.float64) for n in (L, K))
    want = np.convolve(x, ker)[:L]
    acc = np.zeros(L + 2 * K)
    if L0:
        acc[L0:L0 + K - 1] += np.convolve(x[:L0], ker)[L0:]
    outputs = some_late = 0
    for p in range(L0, L):
        T = min(U, L - p)
        M, blocks = F_._long_spec_plan(p, T, U, K, L0, L)
        assert (M is None and blocks == []) or (p < M < p + T and M % U == 0 and M < L)
        for n, lo, tap0, tap1 in blocks:
            assert M % n == 0 and lo == max(M - n, L0) and (tap0, tap1) == (n, min(2 * n, K))
        for t in range(p, p + T):
            reach = min(U, K, t - L0 + 1)
            y = acc[t] + np.dot(ker[:reach], x[t - reach + 1:t + 1][::-1])
            pairs = 0
            if M is not None and t >= M:
                for n, lo, tap0, tap1 in blocks:
                    s = np.arange(lo, t - n + 1)
                    s = s[t - s < tap1]
                    assert ((s < p) & (s >= max(M - n, L0)) & (t - s >= tap0)).all()
                    pairs += len(s)
                    y += np.dot(ker[t - s], x[s])
                assert pairs <= (T - 1) * len(blocks)
            some_late += pairs > 0
            assert y == want[t], (p, t, M)
            outputs += 1
        # the step at p: nothing of the draft remains; the blocks due at p + 1 run as ``step`` runs them
        for n, lo, tap0, tap1, out0 in F_._long_stream_blocks(p + 1, U, K, L0):
            block = np.convolve(x[lo:p + 1], ker[tap0:tap1])
            acc[out0:out0 + len(block)] += block
    assert outputs > 0 and (some_late > 0) == (K > U)


def test_pinned_plans():
    plan = F_._long_spec_plan
    # (p, T, head, taps, first, max_len)
    assert plan(17, 7, 8, 100, 13, 256) == (None, [])                        # M = 24 = p + T: nothing late
    assert plan(17, 8, 8, 100, 13, 256) == (24, [(8, 16, 8, 16)])             # 16 does not divide 24
    assert plan(17, 1, 8, 100, 13, 256) == (None, [])
    assert plan(24, 8, 8, 100, 13, 256) == (None, [])                        # p on the grid: its blocks have run, M = 32 = p + T
    assert plan(61, 8, 8, 100, 13, 256) == (64, [(8, 56, 8, 16), (16, 48, 16, 32), (32, 32, 32, 64), (64, 13, 64, 100)])
    assert plan(125, 8, 8, 100, 13, 256) == (128, [(8, 120, 8, 16), (16, 112, 16, 32), (32, 96, 32, 64), (64, 64, 64, 100)])
    assert plan(14, 8, 8, 100, 13, 256) == (16, [(8, 13, 8, 16), (16, 13, 16, 32)])      # partial blocks behind the prefill
    assert plan(250, 6, 8, 100, 13, 256) == (None, [])                       # M = max_len is never due
    assert plan(250, 8, 8, 100, 13, 256) == (None, [])                       # (... even for a draft that would pass it)
    assert plan(250, 8, 8, 100, 13, 300) == (256, [(8, 248, 8, 16), (16, 240, 16, 32), (32, 224, 32, 64), (64, 192, 64, 100)])
    assert plan(17, 8, 8, 8, 0, 256) == (24, [])                             # a head-only filter: no level
    assert plan(1000, 64, 64, 65536, 0, 4096) == (1024, [(64 << j, 1024 - (64 << j), 64 << j, 128 << j) for j in range(5)])


# ------------------------------------------------------------------------------------------------ arguments
@pytest.fixture
def no_library(monkeypatch):
    """Any call into the library (and with it any device call of the package) fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    for name in ("load_library", "long_step", "long_push", "long_spec", "get_plan"):
        monkeypatch.setattr(_native, name, refuse)


def _meta_stream(position=0, draft=None):
    """A stream that was never constructed on a device: the fields the methods read before their first device call."""
    s = object.__new__(FFTLongConvStream)
    s.batch, s.in_channels, s.out_channels, s.groups = 3, 4, 6, 2
    s.taps, s.head, s.max_len = 100, 16, 50
    s.dtype, s.device = torch.float32, torch.device("meta")
    s._position, s._first, s._draft = position, 0, draft
    return s


@pytest.mark.parametrize("which", ["x", "pregate", "postgate"])
@pytest.mark.parametrize("draft", [None, (11, 5)], ids=["nothing-pending", "a-draft-pending"])
def test_speculate_errors_come_before_any_device_call(which, draft, no_library):
    shapes = dict(x=(3, 4, 7), pregate=(3, 4, 7), postgate=(3, 6, 7))
    stream = _meta_stream(11, draft)

    def call(**bad):
        ts = {k: torch.zeros(s, device="meta") for k, s in shapes.items()}      # nothing is allocated anywhere
        ts.update(bad)
        stream.speculate(ts["x"], ts["pregate"], ts["postgate"])
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
    assert stream.position == 11 and stream._draft == draft


def test_speculate_refuses_a_long_draft_an_empty_one_and_one_past_max_len(no_library):
    stream = _meta_stream(44, (44, 2))
    with pytest.raises(ValueError, match="T = 17 tokens exceeds head = 16"):
        stream.speculate(torch.zeros((3, 4, 17), device="meta"))
    with pytest.raises(ValueError, match="T >= 1"):
        stream.speculate(torch.zeros((3, 4, 0), device="meta"))
    with pytest.raises(TypeError, match="`x` must be a tensor, got NoneType"):
        stream.speculate(None)
    with pytest.raises(RuntimeError, match="T = 7 tokens at position p = 44 passes max_len = 50"):
        stream.speculate(torch.zeros((3, 4, 7), device="meta"))
    assert stream.position == 44 and stream._draft == (44, 2)
    stream = _meta_stream(10)                          # T > head is reported even where the draft would also pass max_len
    stream.max_len = 20
    with pytest.raises(ValueError, match="exceeds head"):
        stream.speculate(torch.zeros((3, 4, 17), device="meta"))
    assert stream.position == 10 and stream._draft is None


def test_accept_errors(no_library):
    stream = _meta_stream(11)
    with pytest.raises(RuntimeError, match="without a pending draft"):
        stream.accept(0)
    with pytest.raises(RuntimeError, match="without a pending draft"):
        stream.accept(True)                            # (the missing draft is reported first)
    assert stream.position == 11 and stream._draft is None
    stream = _meta_stream(11, (11, 7))
    for bad in (-1, 8):
        with pytest.raises(ValueError, match=r"count must lie in \[0, T = 7\], got " + str(bad)):
            stream.accept(bad)
    for bad, name in ((True, "bool"), (1.0, "float"), (None, "NoneType"), ("1", "str")):
        with pytest.raises(TypeError, match="count must be an int, got " + name):
            stream.accept(bad)
    assert stream.position == 11 and stream._draft == (11, 7)      # the draft stays pending


def test_accept_without_a_block_moves_the_position_and_touches_nothing(no_library):
    """p = 17, T = 9, head 16: M = 32 lies past the draft, so no block can be due and ``accept`` is host arithmetic alone."""
    for count in (0, 1, 9):
        stream = _meta_stream(17, (17, 9))
        assert stream.accept(count) is None
        assert stream.position == 17 + count and stream._draft is None
        with pytest.raises(RuntimeError, match="without a pending draft"):
            stream.accept(0)
    stream = _meta_stream(9, (9, 7))                   # M = 16 = p + T: accept(6) stops short of it
    stream.accept(6)
    assert stream.position == 15 and stream._draft is None


def test_a_step_a_push_a_prefill_and_a_reset_drop_the_draft(monkeypatch):
    """The calls are let through to the point where they would launch (their launch helpers return a marker; no block is
    due at the positions used): each one drops the pending draft, after which ``accept`` has nothing to accept.  A call
    that raises for its arguments leaves the draft pending."""
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(F_, "_device_index", lambda dev: 0)
    zeros = lambda *s: torch.zeros(s, device="meta")      # noqa: E731

    def pending():
        s = _meta_stream(3, (3, 5))
        s._launch_step = lambda *a: "y_t"
        s._run_push = lambda *a: "y"
        return s
    stream = pending()
    with pytest.raises(ValueError, match="`x_t` must have shape"):
        stream.step(zeros(3, 5))
    with pytest.raises(ValueError, match="`x` must have shape"):
        stream.push(zeros(3, 5, 2))
    with pytest.raises(RuntimeError, match="position 0 only"):
        stream.prefill(zeros(3, 4, 2))
    assert stream._draft == (3, 5) and stream.position == 3
    assert stream.step(zeros(3, 4)) == "y_t" and stream.position == 4 and stream._draft is None
    with pytest.raises(RuntimeError, match="without a pending draft"):
        stream.accept(1)
    assert stream.position == 4
    stream = pending()
    assert stream.push(zeros(3, 4, 2)) == "y" and stream.position == 5 and stream._draft is None
    with pytest.raises(RuntimeError, match="without a pending draft"):
        stream.accept(0)
    stream = pending()
    stream.hist = stream.acc = torch.zeros(1)
    stream.reset()
    assert stream.position == 0 and stream._draft is None


# ------------------------------------------------------------------------------------------------ ABI
def test_the_header_declares_the_draft_call_and_the_library_exports_it():
    text = open(os.path.join(ROOT, "include", "fftconv_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = re.search(r"\bint\s+fc_long_spec\s*\(\s*const\s+fc_long_step_desc\s*\*([^()]*)\)\s*;", code)
    assert found and len(found.group(0).split(",")) == 14 and "filter_flipped" in found.group(1)
    assert re.search(r"#define\s+FC_ABI_VERSION\s+7\b", code)
    lib = _native.load_library()
    assert hasattr(lib, "fc_long_spec") and callable(_native.long_spec)
    exports = list(_native.EXPORTS)
    assert exports.index("fc_long_spec") == exports.index("fc_long_push") + 1 == exports.index("fc_long_step") + 2
    assert exports[-1] == "fc_long_forward_gated"
    assert len(_native.SIGNATURES["fc_long_spec"][1]) == 14
    assert lib.fc_version() == 7 == _native.ABI_VERSION
    assert "fc_long_spec" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _spec_status(desc, t0=0, count=1, first=0, null=None):
    """Status and text of ``fc_long_spec`` on host memory that is never dereferenced: every refusal comes before the launch.
    ``null``: the index of one required pointer argument to pass as NULL."""
    lib = _native.load_library()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    # x, pregate, postgate, head_taps, filter_flipped, bias, hist, acc, y
    ptrs = [p, None, None, p, p, None, p, p, p]
    if isinstance(null, int):
        ptrs[null] = None
    st = lib.fc_long_spec(ctypes.byref(desc) if null != "desc" else None, *ptrs, t0, count, first, None)
    return st, lib.fc_last_error().decode()


def test_the_draft_call_refuses_bad_calls_without_a_launch():
    ok = dict(batch=2, cin=4, cout=4, groups=2, taps=100, head=16, max_len=50, dtype=0)
    desc = lambda **kw: _native.long_step_desc(**{**ok, **kw})      # noqa: E731
    for null in ("desc", 0, 3, 4, 6, 7, 8):             # the descriptor, x, head_taps, filter_flipped, hist, acc, y
        st, text = _spec_status(desc(), null=null)
        assert st == _native.FC_ERR_INVALID and "null" in text, null
    for bad in (dict(batch=0), dict(cin=3), dict(cout=5), dict(groups=0), dict(taps=0), dict(max_len=0), dict(dtype=1),
                dict(dtype=4)):
        assert _spec_status(desc(**bad))[0] == _native.FC_ERR_INVALID, bad
    st, text = _spec_status(desc(), count=0)
    assert st == _native.FC_ERR_INVALID and "count" in text
    assert _spec_status(desc(), count=-3)[0] == _native.FC_ERR_INVALID
    st, text = _spec_status(desc(), t0=3, count=17)
    assert st == _native.FC_ERR_INVALID and "count (17) exceeds head = 16" in text
    st, text = _spec_status(desc(), t0=44, count=7)
    assert st == _native.FC_ERR_INVALID and "max_len" in text
    assert _spec_status(desc(), t0=50, count=1)[0] == _native.FC_ERR_INVALID
    assert _spec_status(desc(), t0=-1)[0] == _native.FC_ERR_INVALID
    st, text = _spec_status(desc(), t0=5, count=3, first=6)
    assert st == _native.FC_ERR_INVALID and "first" in text
    assert _spec_status(desc(), t0=5, count=3, first=-1)[0] == _native.FC_ERR_INVALID
    for head in (0, 4, 12, 48, 2048):
        st, text = _spec_status(desc(head=head))
        assert st == _native.FC_ERR_UNSUPPORTED and "power of two from 8 to 1024" in text, head
    assert _spec_status(desc(cin=2, cout=2, groups=1, max_len=1 << 28))[0] == _native.FC_ERR_UNSUPPORTED
    # B * groups * tiles past 2^31 workgroups: 2^28 batch items x 16 tiles of 64 columns at head 1024
    st, text = _spec_status(desc(batch=1 << 28, cin=1, cout=1, groups=1, head=1024, max_len=1 << 12), count=1024)
    assert st == _native.FC_ERR_UNSUPPORTED and "workgroups" in text
