"""``FFTLongConvStream`` without a device: the block schedule (``functional._long_stream_blocks``, the only place it lives)
against brute force and against ``np.convolve``, every argument error of the class and of ``FFTLongConv1d.stream`` (raised
before anything touches the library), and the C ABI of the step (``fc_long_step``: declared, exported, ABI 7, its error
codes, all of which come back before a launch)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fft_conv_pytorch_amd
from fft_conv_pytorch_amd import FFTLongConv1d, FFTLongConvStream, _native
from fft_conv_pytorch_amd import functional as F_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (L, K, U, L0): row length, taps, head, prefill
SCHEDULES = [(300, 300, 16, 0), (300, 300, 16, 37), (300, 300, 16, 48), (300, 77, 16, 0), (257, 500, 8, 100),
             (130, 5, 16, 0), (200, 16, 16, 3), (200, 17, 16, 3), (1024, 1024, 64, 0), (1000, 513, 64, 129)]
IDS = ["L%d-K%d-U%d-L0_%d" % s for s in SCHEDULES]


# ------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("L,K,U,L0", SCHEDULES, ids=IDS)
def test_every_pair_is_covered_once_and_in_time(L, K, U, L0):
    """Each (sample t >= first, tap k >= head) with t + k < L lies in exactly one block, and that block is due (after the
    step at i - 1, i <= t + k) before output t + k is emitted; no block reads a sample below ``first`` or one not yet seen."""
    count = np.zeros((L, K), dtype=np.int64)
    for i in range(L0 + 1, L + 1):
        for n, lo, tap0, tap1, out0 in F_._long_stream_blocks(i, U, K, L0):
            assert n >= U and n & (n - 1) == 0 and i % n == 0 and n < K
            assert max(i - n, L0) == lo < i and (tap0, tap1) == (n, min(2 * n, K)) and out0 == lo + n >= i
            count[lo:i, tap0:tap1] += 1
            assert lo + tap0 >= i          # the earliest output the block reaches has not been emitted yet
    t, k = np.meshgrid(np.arange(L), np.arange(K), indexing="ij")
    needed = (t >= L0) & (k >= U) & (t + k < L)
    assert (count[needed] == 1).all()
    assert (count[(t < L0) | (k < U)] == 0).all() and count.max() <= 1


def _stream_by_schedule(x, ker, U, L0):
    """The stream's arithmetic in float64 numpy, the blocks taken from the schedule alone."""
    L, K = len(x), len(ker)
    y, acc = np.zeros(L), np.zeros(L + 2 * K)
    if L0:
        full = np.convolve(x[:L0], ker)
        y[:L0] = full[:L0]
        acc[L0:L0 + K - 1] += full[L0:]
    for t in range(L0, L):
        reach = min(U, K, t - L0 + 1)
        y[t] = acc[t] + sum(ker[k] * x[t - k] for k in range(reach))
        for n, lo, tap0, tap1, out0 in F_._long_stream_blocks(t + 1, U, K, L0):
            block = np.convolve(x[lo:t + 1], ker[tap0:tap1])
            acc[out0:out0 + len(block)] += block
    return y


@pytest.mark.parametrize("L,K,U,L0", SCHEDULES, ids=IDS)
def test_the_schedule_reproduces_np_convolve(L, K, U, L0):
    rng = np.random.default_rng(L + K + U + L0)
    x, ker = (rng.integers(-8, 9, n).astype(np.float64) for n in (L, K))
    want = np.convolve(x, ker)[:L]
    assert np.array_equal(_stream_by_schedule(x, ker, U, L0), want)


def test_nothing_is_due_off_the_grid_of_the_head():
    assert F_._long_stream_blocks(17, 16, 300, 0) == []
    assert F_._long_stream_blocks(16, 16, 16, 0) == []          # every tap is a head tap
    assert F_._long_stream_blocks(16, 16, 17, 0) == [(16, 0, 16, 17, 16)]
    assert F_._long_stream_blocks(64, 16, 300, 37) == [(16, 48, 16, 32, 64), (32, 37, 32, 64, 69), (64, 37, 64, 128, 101)]
    assert F_._long_stream_blocks(48, 16, 300, 48) == []        # the prefill has covered every sample seen


# ------------------------------------------------------------------------------------------------ arguments
@pytest.fixture
def no_library(monkeypatch):
    """Any call into the library (and with it any device call of the package) fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_native, "load_library", refuse)
    monkeypatch.setattr(_native, "long_step", refuse)
    monkeypatch.setattr(_native, "get_plan", refuse)


def test_the_name_is_exported():
    assert fft_conv_pytorch_amd.FFTLongConvStream is F_.FFTLongConvStream and "FFTLongConvStream" in F_.__all__
    assert F_.LONG_STREAM_HEAD == 64


@pytest.mark.parametrize("kw,error,match", [
    (dict(kernel=torch.zeros(4, 2)), ValueError, "kernel"),
    (dict(kernel=[1.0]), TypeError, "tensor"),
    (dict(groups=0), ValueError, "groups"),
    (dict(groups=3), ValueError, "channel mismatch"),
    (dict(batch=0), ValueError, "batch"),
    (dict(batch=2.0), ValueError, "batch"),
    (dict(max_len=0), ValueError, "max_len"),
    (dict(head=48), ValueError, "head"),
    (dict(head=4), ValueError, "head"),
    (dict(head=2048), ValueError, "head"),
    (dict(head=True), ValueError, "head"),
    (dict(bias=torch.zeros(5)), ValueError, "bias"),
    (dict(bias=torch.zeros(4, dtype=torch.float16)), TypeError, "bias"),
    (dict(kernel=torch.zeros(4, 2, 9, dtype=torch.float64), bias=None), TypeError, "float32, float16 or bfloat16"),
    (dict(kernel=torch.zeros(4, 2, 9, dtype=torch.complex64), bias=None), TypeError, "float32, float16 or bfloat16"),
    (dict(), ValueError, "is on cpu"),                       # everything else right: the device is what is wrong
])
def test_constructor_errors_come_before_any_device_call(kw, error, match, no_library):
    args = dict(kernel=torch.zeros(4, 2, 9), bias=torch.zeros(4), groups=2, batch=3, max_len=100, head=None)
    args.update(kw)
    with pytest.raises(error, match=match):
        FFTLongConvStream(args["kernel"], args["bias"], args["groups"], batch=args["batch"], max_len=args["max_len"],
                          head=args["head"])


def test_batch_and_max_len_are_keyword_only():
    with pytest.raises(TypeError):
        FFTLongConvStream(torch.zeros(4, 2, 9), None, 2, 3, 100)


@pytest.mark.parametrize("which", ["x_t", "pregate", "postgate"])
def test_step_errors_come_before_any_device_call(which, no_library):
    """``_long_step_args`` is what ``step`` runs first; the stream here is on (a fictitious) cuda:0 and float32."""
    dev = torch.device("cuda", 0)
    shapes = dict(x_t=(3, 4), pregate=(3, 4), postgate=(3, 6))

    def call(**bad):
        ts = {k: torch.zeros(s, device="meta") for k, s in shapes.items()}      # nothing is allocated anywhere
        ts.update(bad)
        F_._long_step_args(ts["x_t"], ts["pregate"], ts["postgate"], 3, 4, 6, torch.float32, torch.device("meta"))
    call()
    with pytest.raises(ValueError, match=f"`{which}` must have shape"):
        call(**{which: torch.zeros(shapes[which][::-1], device="meta")})
    with pytest.raises(TypeError, match=f"`{which}` has dtype"):
        call(**{which: torch.zeros(shapes[which], dtype=torch.bfloat16, device="meta")})
    with pytest.raises(TypeError, match=f"`{which}` must be a tensor"):
        call(**{which: 1.0})
    with pytest.raises(ValueError, match=f"`{which}` is on cpu but the stream is on meta"):
        call(**{which: torch.zeros(shapes[which])})
    with pytest.raises(ValueError, match="`x_t` is on cpu but the stream is on cuda:0"):
        F_._long_step_args(torch.zeros(3, 4), None, None, 3, 4, 6, torch.float32, dev)
    with pytest.raises(TypeError, match="`x_t` must be a tensor, got NoneType"):
        F_._long_step_args(None, None, None, 3, 4, 6, torch.float32, dev)


@pytest.mark.parametrize("kw", [dict(causal=False), dict(stride=2), dict(dilation=2), dict(channels_last=True)])
def test_module_stream_needs_a_plain_causal_layer(kw, no_library):
    args = dict(causal=True)
    args.update(kw)
    layer = FFTLongConv1d(4, 4, 9, groups=2, **args)
    with pytest.raises(ValueError, match="stream\\(\\) decodes a causal row"):
        layer.stream(2, 100)


def test_module_stream_of_a_padded_layer(no_library):
    layer = FFTLongConv1d(4, 4, 9, padding=4, padding_mode="reflect")
    with pytest.raises(ValueError, match="stream\\(\\) decodes a causal row"):
        layer.stream(2, 100)


def test_module_stream_passes_its_weight_on(no_library):
    """A causal module on the CPU gets as far as the stream's own device check."""
    layer = FFTLongConv1d(4, 4, 9, groups=2, causal=True)
    with pytest.raises(ValueError, match="`kernel` is on cpu"):
        layer.stream(2, 100)
    with pytest.raises(ValueError, match="head"):
        layer.stream(2, 100, head=12)


# ------------------------------------------------------------------------------------------------ ABI
def test_the_header_declares_the_step_and_the_library_exports_it():
    text = open(os.path.join(ROOT, "include", "fftconv_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+fc_long_step\s*\(\s*const\s+fc_long_step_desc\s*\*", code)
    assert re.search(r"typedef\s+struct\s+fc_long_step_desc\s*\{", code)
    assert re.search(r"#define\s+FC_ABI_VERSION\s+7\b", code)
    lib = _native.load_library()
    assert hasattr(lib, "fc_long_step") and "fc_long_step" in _native.EXPORTS
    assert lib.fc_version() == 7 == _native.ABI_VERSION
    # the struct the binding mirrors: seven 64-bit counts, the dtype code and a reserved word
    assert ctypes.sizeof(_native.FcLongStepDesc) == 7 * 8 + 2 * 4
    assert [f[0] for f in _native.FcLongStepDesc._fields_] == ["batch", "in_channels", "out_channels", "groups", "kernel",
                                                               "head", "max_len", "dtype", "reserved"]


def _step_status(desc, t=0, first=0, null=False):
    """Status and text of ``fc_long_step`` on host memory that is never dereferenced: every refusal comes before the launch."""
    lib = _native.load_library()
    buf = ctypes.create_string_buffer(64)
    p = None if null else ctypes.addressof(buf)
    st = lib.fc_long_step(ctypes.byref(desc), p, None, None, p, None, p, p, p, t, first, None)
    return st, lib.fc_last_error().decode()


def test_the_step_refuses_bad_descriptors_without_a_launch():
    ok = dict(batch=2, cin=4, cout=4, groups=2, taps=100, head=16, max_len=50, dtype=0)
    desc = lambda **kw: _native.long_step_desc(**{**ok, **kw})      # noqa: E731
    assert _step_status(desc(), null=True)[0] == _native.FC_ERR_INVALID
    for bad in (dict(batch=0), dict(cin=3), dict(cout=5), dict(groups=0), dict(taps=0), dict(max_len=0), dict(dtype=1),
                dict(dtype=4)):
        assert _step_status(desc(**bad))[0] == _native.FC_ERR_INVALID, bad
    st, text = _step_status(desc(), t=50)
    assert st == _native.FC_ERR_INVALID and "max_len" in text
    assert _step_status(desc(), t=-1)[0] == _native.FC_ERR_INVALID
    assert _step_status(desc(), t=5, first=6)[0] == _native.FC_ERR_INVALID
    for head in (0, 4, 12, 48, 2048):
        st, text = _step_status(desc(head=head))
        assert st == _native.FC_ERR_UNSUPPORTED and "power of two from 8 to 1024" in text, head
    assert _step_status(desc(cin=2, cout=2, groups=1, max_len=1 << 28))[0] == _native.FC_ERR_UNSUPPORTED
