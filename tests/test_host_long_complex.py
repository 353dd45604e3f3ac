"""complex64 tensors through the long-filter path, without a GPU: the dtype code and the new entry points, the geometry
of a complex plan (one batch item per row of the transform where a real plan packs a pair), and a float64 restatement
on the CPU of what the complex builds of the column kernels do -- one item per row, taps conjugated as they are loaded --
against torch's own ``conv1d`` on complex128 tensors and its autograd."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from fft_conv_pytorch_amd import _native
from fft_conv_pytorch_amd import functional as F_
from tests.test_host_long_conv import _factor, _geom, _two_passes, _two_passes_back

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C128_TOL = 1e-10       # float64 restatement against complex128 conv1d: transforms of <= 2^14 points, ~1e-13 expected
NEW_SYMBOLS = ("fc_long_geometry_kind", "fc_long_plan_create_kind", "fc_long_plan_kind")


def _key(B, cin, cout, g, L, K, pl=0, pr=0, keep=0, flip=0, bias=0):
    return (B, cin, cout, g, L, K, pl, pr, keep, flip, bias)


def _complex(key, ext=_native.LONG_EXT_DEFAULT, kind=_native.LONG_COMPLEX):
    return tuple(key) + tuple(ext) + (kind,)


# ------------------------------------------------------------------------------------------------ ABI
def test_dtype_code_in_the_header_and_in_python():
    text = open(os.path.join(ROOT, "include", "fftconv_amd.h")).read()
    assert re.search(r"\bFC_C64\s*=\s*4\b", text)
    assert F_._DTYPE_CODES[torch.complex64] == 4 and _native.FC_C64 == 4
    assert [F_._DTYPE_CODES[t] for t in (torch.float32, torch.float64, torch.float16, torch.bfloat16)] == [0, 1, 2, 3]
    assert re.search(r"#define\s+FC_ABI_VERSION\s+7\b", text) and _native.load_library().fc_version() == 7
    kinds = re.search(r"enum fc_long_kind \{([^}]*)\}", text).group(1)
    assert dict(re.findall(r"(FC_LONG_\w+) = (\d+)", kinds)) == {
        "FC_LONG_REAL": "0", "FC_LONG_COMPLEX": "1", "FC_LONG_CONJ_SIGNAL": "2", "FC_LONG_CONJ_TAPS": "4"}
    assert (_native.LONG_REAL, _native.LONG_COMPLEX, _native.LONG_CONJ_SIGNAL, _native.LONG_CONJ_TAPS) == (0, 1, 2, 4)


def test_new_symbols_are_exported_and_declared():
    lib = _native.load_library()
    text = open(os.path.join(ROOT, "include", "fftconv_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _native.EXPORTS and hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\(" % name, text), name
    assert ctypes.sizeof(_native.FcLongDesc) == 80 and ctypes.sizeof(_native.FcLongExt) == 16


# ------------------------------------------------------------------------------------------------ geometry
REAL_KEYS = [
    _key(3, 4, 4, 4, 5000, 5000, pl=4999, keep=5000, flip=1, bias=1),
    _key(2, 6, 4, 2, 7000, 3000, pl=100, pr=100),
    _key(1, 3, 5, 1, 4200, 1),
    _key(7, 4, 4, 4, 16001, 9000, pl=8999, keep=16001, flip=1, bias=1),
    _key(4, 256, 256, 256, 65536, 65536, pl=65535, keep=65536, flip=1),
    _key(2, 2, 2, 1, 100, 100, pl=99, keep=100, flip=1),
    _key(3, 4, 6, 2, 5000, 1200, pl=37, pr=37) + (3, 1, 3, 2),
    _key(3, 4, 4, 2, 2500, 1200, pl=3597, pr=0, keep=4999, flip=1) + (0, 2, 3, 1),
]


@pytest.mark.parametrize("key", REAL_KEYS)
def test_complex_geometry_counts_items_where_the_real_plan_counts_pairs(key, monkeypatch):
    for knob in ("FFTCONV_LONG_N", "FFTCONV_LONG_WS_MB"):
        monkeypatch.delenv(knob, raising=False)
    B, cin, cout, g = key[:4]
    real = _native.long_geometry(key)
    cx = _native.long_geometry(_complex(key[:11], key[11:] or _native.LONG_EXT_DEFAULT))
    N = real["N1"] * real["N2"]
    for word in ("N1", "N2", "out_len", "out_block", "spectrum_bytes"):
        assert cx[word] == real[word], word
    assert real["spectrum_bytes"] == cout * (cin // g) * N * 8
    # rows of the transform per channel: B for a complex plan, ceil(B / 2) for a real one
    assert cx["slabs"] * cx["slab_pairs"] >= B and (cx["slabs"] - 1) * cx["slab_pairs"] < B
    assert real["slabs"] * real["slab_pairs"] >= (B + 1) // 2 and (real["slabs"] - 1) * real["slab_pairs"] < (B + 1) // 2
    assert cx["workspace_bytes"] == cx["slab_pairs"] * (cin + cout) * N * 8
    assert real["workspace_bytes"] == real["slab_pairs"] * (cin + cout) * N * 8
    assert cx["slab_pairs"] == B and real["slab_pairs"] == (B + 1) // 2       # (all of these fit the default budget)
    # the conjugating kinds change no number
    for kind in (3, 5, 7):
        assert _native.long_geometry(_complex(key[:11], key[11:] or _native.LONG_EXT_DEFAULT, kind)) == cx


def test_complex_slabs_follow_the_workspace_budget(monkeypatch):
    monkeypatch.delenv("FFTCONV_LONG_N", raising=False)
    monkeypatch.setenv("FFTCONV_LONG_WS_MB", "3")          # 32768 points x 8 channels x 8 bytes = 2 MiB per row
    key = _key(7, 4, 4, 4, 16001, 9000, pl=8999, keep=16001, flip=1, bias=1)
    cx, real = _native.long_geometry(_complex(key)), _native.long_geometry(key)
    assert (cx["slabs"], cx["slab_pairs"]) == (7, 1) and (real["slabs"], real["slab_pairs"]) == (4, 1)
    assert cx["workspace_bytes"] == real["workspace_bytes"] == 8 * 32768 * 8


@pytest.mark.parametrize("key", REAL_KEYS)
def test_real_keys_answer_the_same_through_every_entry_point(key, monkeypatch):
    """The calls that existed are the new one with kind = real: equal info words, word for word."""
    monkeypatch.delenv("FFTCONV_LONG_N", raising=False)
    lib = _native.load_library()
    desc, ext = _native.long_desc(key), _native.long_ext(key)
    words = []
    for call in (lambda out: lib.fc_long_geometry_ext(ctypes.byref(desc), ctypes.byref(ext), out),
                 lambda out: lib.fc_long_geometry_kind(ctypes.byref(desc), ctypes.byref(ext), 0, out)):
        info = (ctypes.c_int64 * 8)()
        assert call(ctypes.byref(info)) == 0
        words.append(list(info))
    if len(key) == 11:
        info = (ctypes.c_int64 * 8)()
        assert lib.fc_long_geometry(ctypes.byref(desc), ctypes.byref(info)) == 0
        words.append(list(info))
    assert all(w == words[0] for w in words)
    assert dict(zip(_native.LONG_INFO_WORDS, words[0])) == _native.long_geometry(key)


def test_the_smallest_complex_plan_is_64_by_64(monkeypatch):
    monkeypatch.delenv("FFTCONV_LONG_N", raising=False)
    info = _native.long_geometry(_complex(_key(2, 2, 2, 1, 100, 100, pl=99, keep=100, flip=1)))
    assert (info["N1"], info["N2"], info["out_len"]) == (64, 64, 100)


def test_complex_plans_stop_at_2_pow_28_samples_and_kinds_are_checked():
    big = 1 << 28
    for key in (_key(1, 1, 1, 1, big, 5), _key(1, 1, 1, 1, 5000, big, pl=big - 1, keep=5000, flip=1),
                _key(1, 1, 1, 1, 5000, 5, pl=big), _key(1, 1, 1, 1, 5000, 5, pr=big)):
        with pytest.raises(NotImplementedError, match=r"2\^28"):
            _native.long_geometry(_complex(key))
    # one sample less is addressed (the transform itself is what stops such a row)
    with pytest.raises(NotImplementedError, match=r"2\^24"):
        _native.long_geometry(_complex(_key(1, 1, 1, 1, big - 1, 5)))
    # a real plan of that size keeps its own limit and message
    with pytest.raises(NotImplementedError, match=r"2\^24"):
        _native.long_geometry(_key(1, 1, 1, 1, big, 5))
    key = _key(2, 2, 2, 1, 5000, 100)
    with pytest.raises(ValueError, match="complex"):
        _native.long_geometry(_complex(key, kind=_native.LONG_CONJ_SIGNAL))       # conjugated reads of a real plan
    with pytest.raises(ValueError, match="kind"):
        _native.long_geometry(_complex(key, kind=8))
    with pytest.raises(ValueError, match="16"):
        _native.long_desc(key + (0, 1))


def test_argument_checks_come_before_any_device_call():
    x = torch.randn(2, 2, 5000, dtype=torch.complex64)
    w = torch.randn(2, 2, 100, dtype=torch.complex64)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        F_.fft_long_conv(x, w)
    with pytest.raises(ValueError, match="channel mismatch"):
        F_.fft_long_conv(x, w, groups=2)


# ------------------------------------------------------------------------------------------------ restatement
def long_restated_complex(x, w, bias, pad_left, pad_right, flip, keep, groups, conj_signal=False, conj_taps=False,
                          factors=None):
    """What fc_long_forward computes on a complex plan, pass for pass, in complex128 on the CPU."""
    B, cin, L = x.shape
    cout, cig, K = w.shape
    cog = cout // groups
    nout, keff, padl, tap0, step = _geom(L, K, pad_left, pad_right, flip, keep)
    N1, N2 = factors or _factor(nout + keff - 1)
    N = N1 * N2
    assert N >= nout + keff - 1
    # rows: position p holds x[p - padl]; ONE batch item per row, read conjugated by a plan of that kind
    pos = torch.arange(N) - padl
    ok = (pos >= 0) & (pos < L)
    z = torch.zeros(B, cin, N, dtype=x.dtype)
    z[:, :, ok] = (x.conj() if conj_signal else x)[:, :, pos[ok]]
    # filter rows: position p < keff holds conj(taps[tap0 + step*p]) -- conjugated as loaded, once more by a plan that
    # reads conj(w) -- and the row pass stores conj(transform) / N: conj(FFT(conj u))[f] = U[-f]
    u = torch.zeros(cout, cig, N, dtype=x.dtype)
    taps = w[:, :, [tap0 + step * p for p in range(keff)]]
    u[:, :, :keff] = taps if conj_taps else taps.conj()
    H = _two_passes(u, N1, N2).conj() / N
    Z = _two_passes(z, N1, N2).reshape(B, groups, cig, N1, N2)
    Y = torch.einsum("pgiab,goiab->pgoab", Z, H.reshape(groups, cog, cig, N1, N2)).reshape(B, cout, N1, N2)
    y = _two_passes_back(Y, N1, N2)[..., :nout]
    return y + bias[None, :, None] if bias is not None else y


def _expect(x, w, bias, padding, groups, causal):
    if causal:
        return F.conv1d(F.pad(x, (w.shape[2] - 1, 0)), w.flip(-1), bias, groups=groups)
    return F.conv1d(x, w, bias, padding=padding, groups=groups)


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _randc(*shape):
    return torch.randn(*shape, dtype=torch.complex128)


CASES = [
    # B, cin, cout, groups, L, K, padding, causal
    (3, 4, 4, 4, 5000, 5000, 0, True),        # odd batch (nothing is paired), depthwise, K = L
    (2, 6, 4, 2, 4500, 300, 100, False),      # groups, padding
    (3, 2, 2, 1, 3000, 700, 350, False),      # the shape of the geometry sweep on the GPU
    (2, 2, 2, 1, 100, 100, 0, True),          # a row of the smallest plan
    (2, 2, 2, 1, 3000, 3007, 0, True),        # K = L + 7
]


@pytest.mark.parametrize("B,cin,cout,g,L,K,pad,causal", CASES)
def test_three_passes_restated_match_complex128_conv1d(B, cin, cout, g, L, K, pad, causal):
    torch.manual_seed(L + K)
    x, w, bias = _randc(B, cin, L), _randc(cout, cin // g, K), _randc(cout)
    got = long_restated_complex(x, w, bias, K - 1 if causal else pad, 0 if causal else pad, causal, L if causal else 0, g)
    want = _expect(x, w, bias, pad, g, causal)
    assert got.shape == want.shape and got.dtype == torch.complex128
    assert _rel(got, want) <= C128_TOL


def test_complex_conv1d_is_the_four_real_convolutions():
    """The reference itself: torch's complex conv1d is plain bilinear, no conjugate anywhere."""
    torch.manual_seed(0)
    x, w = _randc(2, 4, 600), _randc(6, 2, 70)
    want = F.conv1d(x, w, None, padding=9, groups=2)
    conv = lambda a, b: F.conv1d(a, b, None, padding=9, groups=2)      # noqa: E731
    four = torch.complex(conv(x.real, w.real) - conv(x.imag, w.imag), conv(x.real, w.imag) + conv(x.imag, w.real))
    assert _rel(four, want) <= 1e-13


def test_restatement_holds_for_an_unbalanced_factorisation():
    torch.manual_seed(3)
    x, w = _randc(3, 2, 6000), _randc(2, 1, 2000)
    for factors in ((64, 128), (128, 64), (64, 256)):
        got = long_restated_complex(x, w, None, 1999, 0, True, 6000, 2, factors=factors)
        assert _rel(got, _expect(x, w, None, 0, 2, True)) <= C128_TOL


@pytest.mark.parametrize("B,cin,cout,g,L,K,pad,causal", [
    (3, 3, 3, 3, 2500, 2500, 0, True),
    (2, 6, 4, 2, 3000, 1200, 100, False),
    (2, 2, 2, 1, 1500, 3000, 0, True),
])
def test_gradient_constructions_with_conjugates_match_complex_autograd(B, cin, cout, g, L, K, pad, causal):
    """dX, dW and db as FFTLongConvFunction.backward forms them for complex tensors, on the restated primitive: dY against
    conj(weight) (a plan that reads the taps conjugated), conj(x) as the signal against dY as the filter (a plan that reads
    the signal conjugated), dY summed."""
    torch.manual_seed(K)
    cig, cog = cin // g, cout // g
    x, w, b = (t.requires_grad_() for t in (_randc(B, cin, L), _randc(cout, cig, K), _randc(cout)))
    y = _expect(x, w, b, pad, g, causal)
    gy = torch.randn_like(y)
    y.backward(gy)
    pl, pr = (K - 1, 0) if causal else (pad, pad)
    wt = w.detach().view(g, cog, cig, K).transpose(1, 2).reshape(cin, cog, K)
    dx = long_restated_complex(gy, wt, None, K - 1 - pl, K - 1 - pr, not causal, L, g, conj_taps=True)
    xt = x.detach().view(B, g, cig, L).permute(2, 1, 0, 3).reshape(cig, g * B, L)
    du = long_restated_complex(xt, gy.permute(1, 0, 2), None, pl, pr, False, K, g, conj_signal=True).permute(1, 0, 2)
    dw = du.flip(-1) if causal else du
    assert _rel(dx, x.grad) <= C128_TOL
    assert _rel(dw, w.grad) <= C128_TOL
    assert _rel(gy.sum(dim=(0, 2)), b.grad) <= C128_TOL


@pytest.mark.parametrize("mode", ["reflect", "replicate", "circular"])
def test_pad_adjoint_folds_complex_rows(mode):
    from fft_conv_pytorch_amd.autograd import _pad_adjoint
    torch.manual_seed(1)
    n, p = 50, 7
    x = _randc(2, 3, n)
    pad = lambda t: torch.complex(F.pad(t.real, (p, p), mode=mode), F.pad(t.imag, (p, p), mode=mode))      # noqa: E731
    g = _randc(2, 3, n + 2 * p)
    folded = _pad_adjoint(g, (n,), (p,), mode)
    # <pad(x), g> = <x, adjoint(g)> for the real-linear map pad, plane by plane
    lhs = (pad(x) * g.conj()).sum()
    rhs = (x * folded.conj()).sum()
    assert folded.shape == x.shape and folded.dtype == torch.complex128
    assert abs(lhs - rhs) <= 1e-10 * abs(lhs)
