"""``fft_long_conv(..., blocks=)`` without a device: the keyword's validation, the pure route function, the geometry of the
blocks plan and of its weight-gradient twin (include/fftconv_amd.h "Rows in overlap-save blocks"), their refusals, and the
places the new names take in the header, the export table and ``FFTLongConv1d.__init__``."""
import inspect
import os
import re

import pytest
import torch

from fft_conv_pytorch_amd import FFTLongConv1d, _native, fft_long_conv, fft_long_conv_gated
from fft_conv_pytorch_amd import functional as F_
from fft_conv_pytorch_amd.autograd import FFTLongConvFunction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("FFTCONV_LONG_DECIM", "FFTCONV_LONG_NLC", "FFTCONV_LONG_N", "FFTCONV_LONG_WS_MB", "FFTCONV_LONG_WGRAD", "FFTCONV_HALF_IO")
N = 4096
BIG = ((1, 1, (1 << 24) + 4096), (1, 1, 1000))
NEW = ("fc_long_blocks_geometry", "fc_long_blocks_plan_create", "fc_long_wgrad_blocks_geometry",
       "fc_long_wgrad_blocks_plan_create")


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _key(B, cin, cout, g, L, K, pl=0, pr=0, keep=0, flip=0, points=N):
    return (B, cin, cout, g, L, K, pl, pr, keep, flip, 0, points)


def _wkey(B, cin, cout, g, L, K, pl=0, pr=0, flip=0, mode=0, s=1, d=1, points=N):
    return (B, cin, cout, g, L, K, pl, pr, L + pl + pr - K + 1, flip, mode, s, d, points)


# ------------------------------------------------------------------------------------------------ the keyword
@pytest.mark.parametrize("bad", [0, 1, 2048, 4095, 4097, 6000, 1 << 25, -4096, 4096.0, "4096", None, (4096,)])
def test_a_bad_keyword_is_a_value_error_before_any_device_call(bad):
    x, w = torch.zeros(1, 1, 9000), torch.zeros(1, 1, 100)       # (CPU tensors: a device check would be a TypeError)
    with pytest.raises(ValueError, match="blocks must be a bool or a power of two"):
        fft_long_conv(x, w, blocks=bad)
    with pytest.raises(ValueError, match="blocks must be"):
        F_._long_blocks_route(x.shape, w.shape, blocks=bad)
    with pytest.raises(ValueError, match="blocks must be"):
        FFTLongConv1d(1, 1, 100, blocks=bad)


@pytest.mark.parametrize("good", [False, True, 4096, 8192, 1 << 18, 1 << 24])
def test_a_good_keyword_is_kept(good):
    assert F_._long_blocks_arg(good) is good or F_._long_blocks_arg(good) == good
    assert FFTLongConv1d(1, 1, 100, blocks=good).blocks == good


def test_signatures():
    sig = inspect.signature(fft_long_conv)
    assert list(sig.parameters)[-1] == "blocks" and sig.parameters["blocks"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["blocks"].default is False
    assert "blocks" not in inspect.signature(fft_long_conv_gated).parameters
    init = inspect.signature(FFTLongConv1d.__init__)
    names = list(init.parameters)
    assert names[-4:] == ["blocks", "stride", "dilation", "padding_mode"]        # inserted before stride
    assert init.parameters["blocks"].kind is inspect.Parameter.KEYWORD_ONLY and init.parameters["blocks"].default is False
    assert list(inspect.signature(FFTLongConv1d.forward).parameters) == ["self", "signal", "pregate", "postgate"]
    fwd = list(inspect.signature(FFTLongConvFunction.forward).parameters)
    assert fwd[-2:] == ["decim", "blocks"]                                       # one more trailing argument
    assert list(inspect.signature(F_._long_plan).parameters)[:9] == [
        "signal", "cout", "groups", "taps", "pad_left", "pad_right", "flip", "out_keep", "has_bias"]
    assert "blocks" in fft_long_conv.__doc__ and "overlap-save" in fft_long_conv.__doc__.lower()


def test_module_stores_the_value_and_keeps_its_state_dict():
    layer = FFTLongConv1d(2, 2, 100, groups=2, blocks=8192)
    assert layer.blocks == 8192 and "blocks=8192" in repr(layer)
    assert "blocks" not in repr(FFTLongConv1d(2, 2, 100))
    assert set(layer.state_dict()) == set(torch.nn.Conv1d(2, 2, 100, groups=2).state_dict())


# ------------------------------------------------------------------------------------------------ the route
ELIGIBLE = dict(signal_shape=(2, 4, 9000), kernel_shape=(4, 2, 700), groups=2, blocks=N)


def _route(**kw):
    args = dict(ELIGIBLE)
    args.update(kw)
    return F_._long_blocks_route(**args)


def test_route_table(monkeypatch):
    assert _route() == "blocks" and _route(causal=True) == "blocks" and _route(padding="same") == "blocks"
    assert _route(dtype=torch.float16) == "blocks" and _route(dtype=torch.bfloat16) == "blocks"
    assert _route(blocks=8192) == "blocks" and _route(blocks=16384) == "plain"          # the row needs 9000 points
    # every ineligibility alone -> what _long_route answers
    for kw in (dict(blocks=False), dict(dtype=torch.complex64), dict(stride=2), dict(dilation=2), dict(padding_mode="reflect", padding=5),
               dict(padding_mode="circular", padding=5), dict(x_layout="nlc"), dict(channels_last=True),
               dict(kernel_shape=(4, 2, N // 2 + 1)), dict(signal_shape=(2, 4, 4000)), dict(blocks=True)):
        args = dict(ELIGIBLE)
        args.update(kw)
        plain = {k: v for k, v in args.items() if k not in ("blocks", "channels_last")}
        assert F_._long_blocks_route(**args) == F_._long_route(**plain) != "blocks", kw
    assert _route(signal_shape=(2, 4, 4000)) == "handoff" and _route(stride=2) == "plain"
    assert _route(kernel_shape=(4, 2, N // 2)) == "blocks"                               # taps read = N / 2: taken
    monkeypatch.setenv("FFTCONV_LONG_DECIM", "1")
    assert _route(stride=2) == "phases"
    monkeypatch.delenv("FFTCONV_LONG_DECIM")
    monkeypatch.setenv("FFTCONV_LONG_NLC", "0")
    assert _route(x_layout="ncl") == "blocks"


def test_true_takes_blocks_only_past_the_limit():
    assert F_._long_blocks_route((1, 1, 1 << 20), (1, 1, 1000), blocks=True) == "plain"
    assert F_._long_blocks_route(*BIG, blocks=True) == "blocks"
    assert F_._long_blocks_route(*BIG, causal=True, blocks=True) == "blocks"
    assert F_._long_blocks_route(*BIG, blocks=1 << 20) == "blocks"
    # not eligible past the limit: the error of the call without the keyword
    for kw in (dict(dilation=2), dict(padding_mode="reflect", padding=3), dict(x_layout="nlc"), dict(channels_last=True),
               dict(dtype=torch.complex64), dict(stride=65)):
        with pytest.raises(NotImplementedError, match=r"2\*\*24"):
            F_._long_blocks_route(*BIG, blocks=True, **kw)
    # K > 2**23: no block keeps half of its points
    with pytest.raises(NotImplementedError, match=r"2\*\*24"):
        F_._long_blocks_route((1, 1, BIG[0][2]), (1, 1, (1 << 23) + 1), blocks=True)
    assert F_._long_blocks_route((1, 1, BIG[0][2]), (1, 1, 1 << 23), blocks=True) == "blocks"


def test_the_other_route_functions_keep_their_answers_and_rows_past_the_limit_still_raise(monkeypatch):
    """The rows of the existing tests past 2**24 points, with nothing passed."""
    assert F_._long_route(*BIG, 64) == "phases"
    with pytest.raises(NotImplementedError, match=str(BIG[0][2])):
        F_._long_route(*BIG, 65)
    with pytest.raises(NotImplementedError, match=r"2\*\*24"):
        F_._long_route(*BIG)
    with pytest.raises(NotImplementedError, match="blocks=True"):          # the text now points to the keyword
        F_._long_route(*BIG)
    with pytest.raises(NotImplementedError):
        F_._long_gated_route((1, 1, 1 << 24), (1, 1, 2), causal=True)
    with pytest.raises(NotImplementedError):
        F_._long_wgrad_route(*BIG)
    L = (1 << 23) + 1
    with pytest.raises(NotImplementedError, match=str(2 * L - 1)):
        F_.fft_long_conv(torch.zeros(1, 1, L), torch.zeros(1, 1, L), causal=True)
    with pytest.raises(NotImplementedError, match=str(2 * L - 1)):         # K = L > 2**23: not eligible either
        F_.fft_long_conv(torch.zeros(1, 1, L), torch.zeros(1, 1, L), causal=True, blocks=True)
    with pytest.raises(NotImplementedError, match=r"needs a transform of 16781312 points; the long-filter path stops at 2\^24"):
        _native.long_geometry((1, 1, 1, 1, BIG[0][2], 1000, 0, 0, 0, 0, 0))
    with pytest.raises(NotImplementedError, match=r"2\^24"):
        _native.wgrad_geometry((1, 1, 1, 1, BIG[0][2], 1000, 0, 0, BIG[0][2] - 999, 0, 0, 1, 1))
    assert F_._long_route((2, 4, 9000), (4, 2, 700), groups=2) == "plain"
    assert F_._long_gated_route((2, 4, 9000), (4, 2, 700), groups=2) == "fused"
    assert F_._long_wgrad_route((2, 4, 9000), (4, 2, 700), groups=2) == "exchanged"


def test_route_function_is_pure():
    src = "".join(inspect.getsource(f) for f in (F_._long_blocks_route, F_._long_blocks_route_of, F_._long_blocks_choice,
                                                 F_._long_blocks_arg))
    assert ".cuda" not in src and "data_ptr" not in src and "_cached_plan" not in src


# ------------------------------------------------------------------------------------------------ geometry
def test_geometry_of_the_first_case():
    g = _native.blocks_geometry(_key(3, 1, 1, 1, 10000, 1000))
    assert (g["N1"], g["N2"], g["out_len"]) == (64, 64, 9001)
    assert (g["V"], g["T"], g["U"], g["pairs"]) == (3097, 3, 9, 5)
    assert g["spectrum_bytes"] == N * 8 and g["workspace_bytes"] == 5 * 2 * N * 8 and g["slabs"] == 1 and g["slab_pairs"] == 5
    w = _native.wgrad_blocks_geometry(_wkey(3, 1, 1, 1, 10000, 1000))
    assert (w["N1"], w["N2"], w["taps"], w["lags"]) == (64, 64, 1000, 1000)
    assert (w["V"], w["T"], w["U"], w["pairs"]) == (3097, 3, 9, 5)
    assert w["workspace_bytes"] == (5 * 2 + 1) * N * 8


@pytest.mark.parametrize("L,T", [(7193, 2), (7194, 3), (4096, 1), (999 + 3097, 1), (999 + 3098, 2)])
def test_block_counts_at_the_bounds(L, T):
    g = _native.blocks_geometry(_key(1, 1, 1, 1, L, 1000))
    assert g["out_len"] == L - 999 and g["V"] == 3097 and g["T"] == T and g["U"] == T and g["pairs"] == (T + 1) // 2


def test_taps_that_meet_only_padding_are_not_read():
    # causal, K 3000 on L 5000 against 2500: the taps read are min(K, L)
    assert _native.blocks_geometry(_key(1, 1, 1, 1, 5000, 2000, pl=1999, keep=5000, flip=1))["V"] == N - 2000 + 1
    assert _native.blocks_geometry(_key(1, 1, 1, 1, 1500, 2000, pl=1999, keep=1500, flip=1))["V"] == N - 1500 + 1
    # 'same' reads every tap
    assert _native.blocks_geometry(_key(2, 2, 2, 2, 9000, 1500, pl=749, pr=750))["V"] == N - 1500 + 1


def test_zero_padding_wider_than_the_longest_transform_is_a_place_in_the_row():
    """pad_left > 2**24 on a blocks plan: the taps are read (keff = K), the blocks cover the padding and the data; only a row
    whose every kept output sees padding reads one tap against zeros."""
    p = (1 << 24) + 8
    assert F_._long_blocks_route((1, 1, 300000), (1, 1, 3), padding=p, blocks=True) == "blocks"
    g = _native.blocks_geometry(_key(1, 1, 1, 1, 300000, 3, pl=p, pr=p, points=0))
    assert g["out_len"] == 300000 + 2 * p - 2 and g["V"] == (1 << 18) - 2 and g["T"] == -(-g["out_len"] // g["V"]) == 130
    w = _native.wgrad_blocks_geometry((1, 1, 1, 1, 300000, 3, p, p, g["out_len"], 0, 0, 1, 1, 0))
    assert (w["taps"], w["lags"], w["V"], w["T"]) == (3, 3, g["V"], 130)
    # the first 1000 outputs of that row see padding only: one tap, no overlap
    only = _native.blocks_geometry(_key(1, 1, 1, 1, 300000, 3, pl=p, pr=p, keep=10000, points=N))
    assert only["out_len"] == 10000 and only["V"] == N and only["T"] == 3


def test_slabs_run_over_unit_pairs_and_the_spectrum_does_not_grow_with_the_row(monkeypatch):
    monkeypatch.setenv("FFTCONV_LONG_WS_MB", "1")
    g = _native.blocks_geometry(_key(2, 6, 4, 2, 9000, 700))
    pair = (6 + 4) * N * 8
    assert (g["T"], g["U"], g["pairs"]) == (3, 6, 3) and g["slab_pairs"] == (1 << 20) // pair == 3 and g["slabs"] == 1
    g2 = _native.blocks_geometry(_key(2, 6, 4, 2, 90000, 700))
    assert g2["pairs"] == 27 and g2["slab_pairs"] == 3 and g2["slabs"] == 9 and g2["workspace_bytes"] == 3 * pair
    assert g2["spectrum_bytes"] == g["spectrum_bytes"] == 4 * 3 * N * 8                # independent of L
    w = _native.wgrad_blocks_geometry(_wkey(2, 6, 4, 2, 9000, 700))
    rows = 4 * 3 * N * 8
    assert w["slab_pairs"] == ((1 << 20) - rows) // pair == 2 and w["slabs"] == 2       # the pairs of one batch item split
    assert w["workspace_bytes"] == 2 * pair + rows
    monkeypatch.delenv("FFTCONV_LONG_WS_MB")
    big = _native.blocks_geometry(_key(1, 1, 1, 1, BIG[0][2], 1000, points=0))
    assert big["N1"] * big["N2"] == 1 << 18 and big["spectrum_bytes"] == 8 << 18 and big["T"] == 65 and big["out_len"] == BIG[0][2] - 999


def test_the_planners_choice():
    pts = lambda K: (lambda g: g["N1"] * g["N2"])(_native.blocks_geometry(_key(1, 1, 1, 1, 1 << 25, K, points=0)))      # noqa: E731
    assert pts(1000) == 1 << 18 and pts(1 << 16) == 1 << 18 and pts((1 << 16) + 1) == 1 << 19
    assert pts(1 << 22) == 1 << 24 and pts(1 << 23) == 1 << 24
    with pytest.raises(NotImplementedError, match="8388609"):
        pts((1 << 23) + 1)


def test_forced_factorisation(monkeypatch):
    monkeypatch.setenv("FFTCONV_LONG_N", "64x128")
    g = _native.blocks_geometry(_key(2, 1, 1, 1, 20000, 1500, points=8192))
    assert (g["N1"], g["N2"]) == (64, 128)
    monkeypatch.setenv("FFTCONV_LONG_N", "128x64")
    assert (_native.blocks_geometry(_key(2, 1, 1, 1, 20000, 1500, points=8192))["N1"]) == 128
    with pytest.raises(ValueError, match="FFTCONV_LONG_N"):
        _native.blocks_geometry(_key(2, 1, 1, 1, 20000, 1500, points=N))


# ------------------------------------------------------------------------------------------------ refusals
def test_half_a_block_of_taps_is_taken_and_one_more_refused():
    assert _native.blocks_geometry(_key(2, 1, 1, 1, 12000, N // 2, pl=N // 2 - 1, keep=12000, flip=1))["V"] == N // 2 + 1
    with pytest.raises(NotImplementedError, match=r"K = 2049.*N = 4096"):
        _native.blocks_geometry(_key(2, 1, 1, 1, 12000, N // 2 + 1, pl=N // 2, keep=12000, flip=1))
    assert _native.wgrad_blocks_geometry(_wkey(2, 1, 1, 1, 12000, N // 2))["lags"] == N // 2
    with pytest.raises(NotImplementedError, match=r"K = 2049.*N = 4096"):
        _native.wgrad_blocks_geometry(_wkey(2, 1, 1, 1, 12000, N // 2 + 1))


@pytest.mark.parametrize("points", [1, 2048, 4097, 6000, 1 << 25, -1])
def test_block_points_outside_the_powers_of_two_in_range_are_invalid(points):
    with pytest.raises(ValueError, match="block_points"):
        _native.blocks_geometry(_key(1, 1, 1, 1, 9000, 100, points=points))
    with pytest.raises(ValueError, match="block_points"):
        _native.wgrad_blocks_geometry(_wkey(1, 1, 1, 1, 9000, 100, points=points))


def test_the_weight_gradient_by_blocks_takes_the_plain_layer_only():
    for kw in (dict(s=2), dict(d=2), dict(mode=1)):
        with pytest.raises(NotImplementedError, match="stride 1, dilation 1 and pad_mode constant"):
            _native.wgrad_blocks_geometry(_wkey(1, 1, 1, 1, 9000, 100, **kw))


def test_limits_of_rows_and_grids(monkeypatch):
    with pytest.raises(NotImplementedError, match=r"2\^29"):
        _native.blocks_geometry(_key(1, 1, 1, 1, (1 << 29) + 1, 100, points=0))
    ok = _native.blocks_geometry(_key(1, 1, 1, 1, 1 << 29, 100, points=0))
    assert ok["T"] == -(-((1 << 29) - 99) // ((1 << 18) - 99))
    monkeypatch.setenv("FFTCONV_LONG_WS_MB", str(1 << 24))      # (a budget that holds every unit pair: one launch over them all)
    with pytest.raises(NotImplementedError, match=r"unit pairs x .* 2\^31 workgroups"):
        _native.blocks_geometry(_key(64, 4096, 4096, 1, 1 << 24, 100, points=4096))
    monkeypatch.delenv("FFTCONV_LONG_WS_MB")
    assert _native.blocks_geometry(_key(64, 4096, 4096, 1, 1 << 24, 100, points=4096))["slabs"] > 1
    with pytest.raises(ValueError, match="divisible"):
        _native.blocks_geometry(_key(1, 3, 4, 2, 9000, 10))


# ------------------------------------------------------------------------------------------------ header, exports
def test_new_entry_points_only_and_abi_7():
    header = open(os.path.join(ROOT, "include", "fftconv_amd.h")).read()
    declared = set(re.findall(r"\b(fc_[a-z0-9_]+)\s*\(", header))
    assert set(NEW) <= declared and declared == set(_native.EXPORTS)
    assert "#define FC_ABI_VERSION 7" in header and _native.ABI_VERSION == 7
    assert _native.EXPORTS[-1] == "fc_long_forward_gated"
    assert _native.EXPORTS[_native.EXPORTS.index("fc_long_wgrad") + 1] == "fc_long_wgrad_gated"
    lib = _native.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
    assert "typedef struct fc_long_blocks_desc" in header
    import ctypes
    assert ctypes.sizeof(_native.FcLongBlocksDesc) == ctypes.sizeof(_native.FcLongDesc) + 8 == 88
    assert _native._PLAN_TAGS.keys().isdisjoint(_native._BLOCKS_PLAN_TAGS)
    assert issubclass(_native.LongBlocksPlan, _native.LongPlan) and issubclass(_native.LongWgradBlocksPlan, _native.LongWgradPlan)
