"""Stride, dilation and padding modes of the long-filter path without a GPU: the planner's geometry through
``fc_long_geometry_ext``, a float64 restatement of the generalised three passes (the row maps of csrc/long1d.hpp's mapped
builds and the host's trimming, on the transforms of tests/test_host_long_conv.py) against the float64 oracle, the dX and dW
constructions of FFTLongConvFunction on that restatement against float64 autograd, and the new symbols."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

from fft_conv_pytorch_amd import _native
from fft_conv_pytorch_amd import functional as F_
from fft_conv_pytorch_amd.autograd import _pad_adjoint
from oracle.fft_conv_oracle import fft_conv_oracle_torch, output_extent
from tests.test_host_long_conv import F64_TOL, TILE_LENGTHS, _factor, _rel, _two_passes, _two_passes_back

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"constant": 0, "reflect": 1, "replicate": 2, "circular": 3}


def _geom(L, K, pad_left, pad_right, flip, keep, mode, up, dil, step):
    """The host's row geometry (host_long.cpp long_geometry) -> nout, taps read, data offset, first tap, tap step, need."""
    span = up * (L - 1) + 1
    Lp = span + pad_left + pad_right
    full = (Lp - dil * (K - 1) - 1) // step + 1
    nout = keep or full
    klo, khi = 0, K - 1
    if mode == 0:
        lo = pad_left - step * (nout - 1)
        klo = -(-lo // dil) if lo > 0 else 0
        khi = min(K - 1, (pad_left + span - 1) // dil)
    assert khi >= klo
    keff = khi - klo + 1
    tap0, tstep = (K - 1 - klo, -1) if flip else (klo, 1)
    return nout, keff, pad_left - dil * klo, tap0, tstep, step * (nout - 1) + dil * (keff - 1) + 1


def _axis_src(pos, L, pad_left, pad_right, mode, up):
    """Source index of every row position (-1: a zero), as the mapped long_cols_fwd computes it."""
    if up > 1:
        q = torch.div(pos, up, rounding_mode="floor")
        return torch.where((pos >= 0) & (q * up == pos) & (q < L), q, torch.full_like(pos, -1))
    if mode == 0:
        return torch.where((pos >= 0) & (pos < L), pos, torch.full_like(pos, -1))
    inside = (pos >= -pad_left) & (pos < L + pad_right)
    if mode == 1:
        src = torch.where(pos < 0, -pos, torch.where(pos >= L, 2 * (L - 1) - pos, pos))
    elif mode == 2:
        src = pos.clamp(0, L - 1)
    else:
        src = torch.where(pos < 0, pos + L, torch.where(pos >= L, pos - L, pos))
    return torch.where(inside, src, torch.full_like(pos, -1))


def long_general_restated(x, w, bias, pad_left, pad_right, flip, keep, groups, mode=0, up=1, dil=1, step=1, factors=None):
    """What a plan of fc_long_plan_create_ext computes, pass for pass, in float64 on the CPU."""
    B, cin, L = x.shape
    cout, cig, K = w.shape
    cog = cout // groups
    nout, keff, padl, tap0, tstep, need = _geom(L, K, pad_left, pad_right, flip, keep, mode, up, dil, step)
    N1, N2 = factors or _factor(need)
    N = N1 * N2
    assert N >= need
    # rows: position p holds x[map(p - padl)]; two batch items per complex row
    src = _axis_src(torch.arange(N) - padl, L, pad_left, pad_right, mode, up)
    ok = src >= 0
    xr = torch.zeros(B + B % 2, cin, N, dtype=x.dtype)
    xr[:B, :, ok] = x[:, :, src[ok]]
    z = torch.complex(xr[0::2], xr[1::2])
    # filter rows: position dil*q, q < keff, holds taps[tap0 + tstep*q]
    u = torch.zeros(cout, cig, N, dtype=x.dtype)
    u[:, :, 0:dil * (keff - 1) + 1:dil] = w[:, :, [tap0 + tstep * q for q in range(keff)]]
    H = _two_passes(torch.complex(u, torch.zeros_like(u)), N1, N2).conj() / N
    Z = _two_passes(z, N1, N2).reshape(z.shape[0], groups, cig, N1, N2)
    Y = torch.einsum("pgiab,goiab->pgoab", Z, H.reshape(groups, cog, cig, N1, N2)).reshape(z.shape[0], cout, N1, N2)
    # sample t of the stride-1 result is kept at t / step where that divides
    yz = _two_passes_back(Y, N1, N2)[..., 0:step * (nout - 1) + 1:step]
    y = torch.empty(B + B % 2, cout, nout, dtype=x.dtype)
    y[0::2], y[1::2] = yz.real, yz.imag
    y = y[:B]
    return y + bias[None, :, None] if bias is not None else y


def _pads(L, K, padding, causal, s, d):
    """(pad_left, pad_right, out_keep) as fft_long_conv derives them."""
    pl, pr, _ = F_._long_geometry(torch.empty(1, 1, L), torch.empty(1, 1, K), None, padding, 1, causal, s, d)
    return pl, pr, F_._long_keep(L, causal, s)


def _expect(x, w, bias, padding, groups, causal, s, d, mode):
    K = w.shape[2]
    if causal:
        return fft_conv_oracle_torch(F.pad(x, (d * (K - 1), 0)), w.flip(-1), bias, stride=s, dilation=d, groups=groups)
    if padding == "same":
        total = d * (K - 1)
        xp = F.pad(x, (total // 2, total - total // 2), mode=mode)
        return fft_conv_oracle_torch(xp, w, bias, stride=s, dilation=d, groups=groups)
    return fft_conv_oracle_torch(x, w, bias, stride=s, padding=padding, dilation=d, groups=groups, padding_mode=mode)


CASES = [
    # B, cin, cout, groups, L, K, padding, causal, stride, dilation, mode
    (3, 4, 4, 4, 5000, 1200, 0, False, 2, 1, "constant"),
    (3, 2, 2, 2, 5001, 900, 0, False, 3, 1, "constant"),
    (2, 2, 2, 1, 5000, 1000, 0, False, 1, 2, "constant"),
    (2, 2, 3, 1, 6000, 700, 0, False, 1, 5, "constant"),
    (3, 6, 4, 2, 5000, 1200, 37, False, 2, 3, "constant"),
    (3, 2, 2, 2, 5000, 1200, 37, False, 2, 3, "reflect"),
    (1, 2, 2, 1, 4500, 800, 4499, False, 1, 1, "reflect"),
    (2, 2, 2, 2, 4500, 1000, 37, False, 1, 2, "replicate"),
    (3, 2, 2, 1, 4500, 1000, 37, False, 3, 1, "circular"),
    (2, 2, 2, 1, 4500, 2000, 4500, False, 1, 2, "circular"),
    (2, 2, 2, 2, 5000, 1000, "same", False, 1, 3, "constant"),      # 2997 zeros: 1498 + 1499
    (2, 2, 2, 2, 5000, 600, "same", False, 1, 3, "reflect"),
    (3, 3, 3, 3, 5000, 2000, 0, True, 3, 1, "constant"),
    (2, 2, 2, 1, 3000, 1500, 0, True, 1, 4, "constant"),            # dilated extent 5997 > L
    (2, 2, 2, 2, 4501, 1500, 0, True, 2, 5, "constant"),
    (2, 2, 2, 1, 5000, 10, 3000, False, 2, 3, "constant"),          # padding wider than the filter: leading taps dropped
]


@pytest.mark.parametrize("B,cin,cout,g,L,K,pad,causal,s,d,mode", CASES)
def test_generalised_passes_restated_match_the_oracle(B, cin, cout, g, L, K, pad, causal, s, d, mode):
    torch.manual_seed(L + K + s + d)
    x = torch.randn(B, cin, L, dtype=torch.float64)
    w = torch.randn(cout, cin // g, K, dtype=torch.float64)
    bias = torch.randn(cout, dtype=torch.float64)
    pl, pr, keep = _pads(L, K, pad, causal, s, d)
    got = long_general_restated(x, w, bias, pl, pr, causal, keep, g, MODES[mode], 1, d, s)
    want = _expect(x, w, bias, pad, g, causal, s, d, mode)
    assert got.shape == want.shape
    assert _rel(got, want) <= F64_TOL


def test_defaults_restate_the_existing_primitive():
    from tests.test_host_long_conv import long_restated
    torch.manual_seed(1)
    x = torch.randn(3, 2, 4500, dtype=torch.float64)
    w = torch.randn(2, 1, 900, dtype=torch.float64)
    for pl, pr, flip, keep in ((899, 0, True, 4500), (100, 100, False, 0), (2000, 0, False, 1500)):
        assert torch.equal(long_general_restated(x, w, None, pl, pr, flip, keep, 2), long_restated(x, w, None, pl, pr, flip, keep, 2))


def _backward(gy, x, w, pl, pr, flip, g, s, d, mode):
    """dX and dW as FFTLongConvFunction.backward forms them, on the restated primitive."""
    B, cin, L = x.shape
    cout, cig, K = w.shape
    cog = cout // g
    code = MODES[mode]
    wt = w.view(g, cog, cig, K).transpose(1, 2).reshape(cin, cog, K)
    keep, lead, dy = (L, d * (K - 1) - pl, gy) if code == 0 else (L + pl + pr, d * (K - 1), gy)
    if lead < 0:
        drop = -(lead // s)
        dy, lead = dy[..., drop:], lead + drop * s
    tail = keep + d * (K - 1) - lead - (s * (dy.shape[2] - 1) + 1)
    if tail < 0:
        dy, tail = dy[..., :dy.shape[2] - (-tail) // s], 0
    dx = long_general_restated(dy, wt, None, lead, tail, not flip, keep, g, 0, s, d, 1)
    if code:
        p = max(pl, pr)
        dx = _pad_adjoint(F.pad(dx, (p - pl, p - pr)), (L,), (p,), mode)
    xt = x.view(B, g, cig, L).permute(2, 1, 0, 3).reshape(cig, g * B, L)
    du = long_general_restated(xt, gy.permute(1, 0, 2), None, pl, pr, False, K, g, code, 1, s, d).permute(1, 0, 2)
    return dx, (du.flip(-1) if flip else du)


@pytest.mark.parametrize("B,cin,cout,g,L,K,pad,causal,s,d,mode", [
    (3, 3, 3, 3, 3000, 700, 0, False, 2, 3, "constant"),
    (2, 6, 4, 2, 3000, 500, 37, False, 3, 2, "constant"),
    (2, 2, 2, 1, 3000, 20, 900, False, 2, 3, "constant"),          # padding wider than the filter: dY cropped
    (2, 2, 2, 1, 3000, 600, 37, False, 2, 1, "reflect"),
    (2, 2, 2, 2, 2500, 400, 100, False, 1, 3, "replicate"),
    (2, 2, 2, 1, 2500, 400, 333, False, 2, 2, "circular"),
    (2, 2, 2, 1, 2500, 400, "same", False, 1, 3, "circular"),      # unequal paddings folded
    (3, 2, 2, 2, 2500, 900, 0, True, 3, 1, "constant"),
    (2, 2, 2, 1, 1500, 700, 0, True, 2, 4, "constant"),
])
def test_gradient_constructions_match_autograd_through_the_oracle(B, cin, cout, g, L, K, pad, causal, s, d, mode):
    torch.manual_seed(K + s)
    x = torch.randn(B, cin, L, dtype=torch.float64, requires_grad=True)
    w = torch.randn(cout, cin // g, K, dtype=torch.float64, requires_grad=True)
    y = _expect(x, w, None, pad, g, causal, s, d, mode)
    gy = torch.randn_like(y)
    y.backward(gy)
    pl, pr, _ = _pads(L, K, pad, causal, s, d)
    dx, dw = _backward(gy, x.detach(), w.detach(), pl, pr, causal, g, s, d, mode)
    assert dx.shape == x.shape and dw.shape == w.shape
    assert _rel(dx, x.grad) <= F64_TOL
    assert _rel(dw, w.grad) <= F64_TOL


def _key(B, cin, cout, g, L, K, pl=0, pr=0, keep=0, flip=0, bias=0, mode=0, up=1, dil=1, step=1):
    return (B, cin, cout, g, L, K, pl, pr, keep, flip, bias, mode, up, dil, step)


GEOMETRY_GRID = [(L, K, pad, s, d, mode, causal)
                 for L in (5000, 8192, 65536)
                 for K in (1, 900, 4001)
                 for pad in (0, 37)
                 for s in (1, 2, 3)
                 for d in (1, 2, 5)
                 for mode in ("constant", "reflect", "circular")
                 for causal in (False, True)
                 if not (causal and (pad or mode != "constant")) and d * (K - 1) + 1 <= L + 2 * pad]


def test_geometry_of_the_grid(monkeypatch):
    monkeypatch.delenv("FFTCONV_LONG_N", raising=False)
    assert len(GEOMETRY_GRID) > 200
    for L, K, pad, s, d, mode, causal in GEOMETRY_GRID:
        pl, pr, keep = _pads(L, K, pad, causal, s, d)
        info = _native.long_geometry(_key(3, 4, 4, 4, L, K, pl, pr, keep, int(causal), 0, MODES[mode], 1, d, s))
        want = -(-L // s) if causal else output_extent(L, K, s, pad, d)
        assert info["out_len"] == want, (L, K, pad, s, d, mode, causal)
        need = _geom(L, K, pl, pr, causal, keep, MODES[mode], 1, d, s)[5]
        assert need <= s * (want - 1) + d * (K - 1) + 1
        N1, N2 = info["N1"], info["N2"]
        assert N1 in TILE_LENGTHS and N2 in TILE_LENGTHS and (N1, N2) == _factor(need), (L, K, pad, s, d, mode, causal)
        assert info["spectrum_bytes"] == 4 * 1 * N1 * N2 * 8


def test_trimming_counts_only_taps_that_can_meet_the_data(monkeypatch):
    monkeypatch.delenv("FFTCONV_LONG_N", raising=False)
    # causal, K > L: dilation 4 leaves ceil(L / 4) taps at lags below L
    info = _native.long_geometry(_key(1, 1, 1, 1, 6000, 6000, 4 * 5999, 0, 6000, 1, 0, 0, 1, 4, 1))
    assert (info["N1"], info["N2"]) == _factor(5999 + 4 * 1499 + 1)
    # the spread row of a strided gradient: 3 * (2000 - 1) + 1 positions of data
    info = _native.long_geometry(_key(1, 1, 1, 1, 2000, 500, 499, 499, 0, 0, 0, 0, 3, 1, 1))
    assert info["out_len"] == 3 * 1999 + 1 + 499
    # another padding mode fills every position: no tap is dropped
    a = _native.long_geometry(_key(1, 1, 1, 1, 5000, 3000, 4000, 4000, 100, 0, 0, 0))
    b = _native.long_geometry(_key(1, 1, 1, 1, 5000, 3000, 4000, 4000, 100, 0, 0, 2))
    assert a["N1"] * a["N2"] == 4096 and (b["N1"], b["N2"]) == _factor(100 + 3000 - 1)


def test_default_extension_answers_word_for_word_what_fc_long_geometry_answers(monkeypatch):
    monkeypatch.delenv("FFTCONV_LONG_N", raising=False)
    lib = _native.load_library()
    for key in ((3, 4, 4, 4, 5000, 5000, 4999, 0, 5000, 1, 1), (4, 8, 8, 1, 8192, 8192, 4096, 4096, 0, 0, 0),
                (7, 2, 2, 2, 8000, 100, 0, 0, 0, 0, 0), (2, 2, 2, 1, 70000, 9, 5000, 3, 17, 0, 1)):
        desc = _native.long_desc(key)
        old, new, null = ((ctypes.c_int64 * 8)() for _ in range(3))
        assert lib.fc_long_geometry(ctypes.byref(desc), ctypes.byref(old)) == 0
        ext = _native.long_ext(key)
        assert (ext.pad_mode, ext.src_up, ext.tap_dil, ext.out_step) == (0, 1, 1, 1)
        assert lib.fc_long_geometry_ext(ctypes.byref(desc), ctypes.byref(ext), ctypes.byref(new)) == 0
        assert lib.fc_long_geometry_ext(ctypes.byref(desc), None, ctypes.byref(null)) == 0
        assert list(old) == list(new) == list(null)
        assert _native.long_geometry(key) == _native.long_geometry(key + (0, 1, 1, 1))


@pytest.mark.parametrize("key,match", [
    (_key(1, 1, 1, 1, 5000, 10, mode=4), "pad_mode"),
    (_key(1, 1, 1, 1, 5000, 10, mode=-1), "pad_mode"),
    (_key(1, 1, 1, 1, 5000, 10, up=0), "src_up"),
    (_key(1, 1, 1, 1, 5000, 10, dil=0), "tap_dil"),
    (_key(1, 1, 1, 1, 5000, 10, step=0), "out_step"),
    (_key(1, 1, 1, 1, 5000, 10, 5, 5, mode=1, up=2), "src_up"),
    (_key(1, 1, 1, 1, 5000, 10, 5, 5, mode=3, up=3), "src_up"),
    (_key(1, 1, 1, 1, 5000, 10, 5000, 0, mode=1), "reflect"),
    (_key(1, 1, 1, 1, 5000, 10, 0, 5001, mode=3), "circular"),
    (_key(1, 1, 1, 1, 5000, 2501, dil=2), "longer than the padded row"),
    (_key(1, 1, 1, 1, 5000, 10, keep=2497, step=2), "out_keep"),
])
def test_invalid_extensions_are_refused(key, match):
    with pytest.raises(ValueError, match=match):
        _native.long_geometry(key)


def test_plan_keys_have_eleven_or_fifteen_words():
    with pytest.raises(ValueError):
        _native.long_geometry((1, 1, 1, 1, 5000, 10, 0, 0, 0, 0, 0, 0, 1, 1))
    params = inspect.signature(F_._long_plan).parameters
    assert list(params)[:9] == ["signal", "cout", "groups", "taps", "pad_left", "pad_right", "flip", "out_keep", "has_bias"]
    for name, default in (("pad_mode", 0), ("src_up", 1), ("tap_dil", 1), ("out_step", 1)):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default == default


def test_argument_errors_of_the_new_keywords_come_before_any_device_call():
    x, w = torch.zeros(2, 4, 6000), torch.zeros(4, 2, 3000)
    with pytest.raises(ValueError, match="stride"):
        F_.fft_long_conv(x, w, groups=2, stride=0)
    with pytest.raises(ValueError, match="dilation"):
        F_.fft_long_conv(x, w, groups=2, dilation=0)
    with pytest.raises(ValueError, match="padding_mode"):
        F_.fft_long_conv(x, w, groups=2, padding_mode="mirror")
    with pytest.raises(ValueError, match="strided"):
        F_.fft_long_conv(x, w, groups=2, padding="same", stride=2)
    with pytest.raises(ValueError, match="padding_mode must be 'constant'"):
        F_.fft_long_conv(x, w, groups=2, causal=True, padding_mode="reflect")
    with pytest.raises(ValueError, match="longer than the padded row"):
        F_.fft_long_conv(x, w, groups=2, dilation=3)
    with pytest.raises(ValueError, match="reflect"):
        F_.fft_long_conv(x, w[..., :5], groups=2, padding=6000, padding_mode="reflect")
    with pytest.raises(ValueError, match="circular"):
        F_.fft_long_conv(x, w[..., :5], groups=2, padding=6001, padding_mode="circular")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F_.fft_long_conv(x, w, groups=2, stride=2, dilation=2, padding=37, padding_mode="circular")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F_.fft_long_conv(x[..., :100], w[..., :20], groups=2, causal=True, stride=2, dilation=3)      # short rows too


def test_module_stores_the_arguments_as_conv1d_does():
    import copy
    import pickle
    from fft_conv_pytorch_amd import FFTConv1d, FFTLongConv1d
    layer = FFTLongConv1d(4, 6, 3000, padding=37, groups=2, stride=2, dilation=3, padding_mode="circular")
    ref = torch.nn.Conv1d(4, 6, 3000, stride=2, padding=37, dilation=3, groups=2, padding_mode="circular")
    for name in ("stride", "dilation", "padding", "padding_mode", "groups", "_reversed_padding_repeated_twice"):
        assert getattr(layer, name) == getattr(ref, name), name
    assert set(layer.state_dict()) == {"weight", "bias"}
    layer.load_state_dict(ref.state_dict())
    FFTConv1d(4, 6, 3000, stride=2, padding=37, dilation=3, groups=2, padding_mode="circular").load_state_dict(layer.state_dict())
    for clone in (copy.deepcopy(layer), pickle.loads(pickle.dumps(layer))):
        assert (clone.stride, clone.dilation, clone.padding_mode, clone.causal) == ((2,), (3,), "circular", False)
        assert torch.equal(clone.weight, layer.weight)
    params = inspect.signature(FFTLongConv1d.__init__).parameters
    assert list(params)[-3:] == ["stride", "dilation", "padding_mode"]
    assert all(params[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("stride", "dilation", "padding_mode"))
    assert (params["stride"].default, params["dilation"].default, params["padding_mode"].default) == (1, 1, "zeros")
    with pytest.raises(ValueError, match="padding_mode"):
        FFTLongConv1d(4, 6, 3000, causal=True, padding_mode="reflect")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer(torch.zeros(1, 4, 9000))


def test_new_symbols_are_declared_and_exported_and_the_abi_is_unchanged():
    header = open(os.path.join(ROOT, "include", "fftconv_amd.h")).read()
    declared = set(re.findall(r"\b(fc_[a-z0-9_]+)\s*\(", header))
    new = {"fc_long_geometry_ext", "fc_long_plan_create_ext"}
    assert new <= declared and new <= set(_native.EXPORTS) and declared == set(_native.EXPORTS)
    assert re.search(r"int fc_long_geometry_ext\(const fc_long_desc\* desc, const fc_long_ext\* ext, int64_t info\[8\]\);", header)
    assert re.search(r"int fc_long_plan_create_ext\(const fc_long_desc\* desc, const fc_long_ext\* ext, fc_long_plan\*\* out_plan\);",
                     header)
    lib = _native.load_library()
    for name in new:
        assert hasattr(lib, name), name
    m = re.search(r"#define\s+FC_ABI_VERSION\s+(\d+)", header)
    assert int(m.group(1)) == 7 == _native.ABI_VERSION == lib.fc_version()
    assert ctypes.sizeof(_native.FcLongDesc) == 80
    assert ctypes.sizeof(_native.FcLongExt) == 16
    assert [n for n, _ in _native.FcLongExt._fields_] == ["pad_mode", "src_up", "tap_dil", "out_step"]
    body = re.search(r"typedef struct fc_long_ext \{(.*?)\} fc_long_ext;", header, re.S).group(1)
    assert re.findall(r"\b(pad_mode|src_up|tap_dil|out_step)\b", body) == ["pad_mode", "src_up", "tap_dil", "out_step"]
