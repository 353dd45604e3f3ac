"""The long-filter path without a GPU: its three passes restated in torch on the CPU (this pins the index conventions the
kernels of csrc/long1d.hpp copy), the gradient identities of FFTLongConvFunction, the two-table twiddle, the planner's
factorisation through ``fc_long_geometry``, and the argument checks that run before any device call."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fft_conv_pytorch_amd import _native
from fft_conv_pytorch_amd import functional as F_
from oracle.fft_conv_oracle import fft_conv_oracle_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_LENGTHS = (64, 128, 256, 512, 1024, 2048, 4096)
F64_TOL = 1e-10        # float64 restatement against the float64 oracle: transforms of <= 2^14 points, ~1e-13 expected


def _geom(L, K, pad_left, pad_right, flip, keep):
    """The host's row geometry (host_long.cpp long_geometry): taps that meet the data, their order, the data's offset."""
    full = L + pad_left + pad_right - K + 1
    nout = keep or full
    klo = max(0, pad_left - nout + 1)
    khi = min(K - 1, pad_left + L - 1)
    assert khi >= klo
    keff = khi - klo + 1
    padl = pad_left - klo
    tap0, step = (K - 1 - klo, -1) if flip else (klo, 1)
    return nout, keff, padl, tap0, step


def _factor(need):
    lg = 12
    while (1 << lg) < need:
        lg += 1
    return 1 << (lg // 2), 1 << (lg - lg // 2)


def _twiddle(N1, N2):
    k1 = torch.arange(N1, dtype=torch.float64)[:, None]
    n2 = torch.arange(N2, dtype=torch.float64)[None, :]
    return torch.exp(-2j * math.pi * k1 * n2 / (N1 * N2))


def _two_passes(rows, N1, N2):
    """rows (..., N) complex -> bins in the order [k1][k2], k = k1 + N1*k2, of the row indexed n = n1*N2 + n2."""
    a = torch.fft.fft(rows.reshape(rows.shape[:-1] + (N1, N2)), dim=-2)       # columns: N1 points along n1 -> [k1][n2]
    return torch.fft.fft(a * _twiddle(N1, N2), dim=-1)                        # rows: N2 points along n2 -> [k1][k2]


def _two_passes_back(spec, N1, N2):
    a = torch.fft.ifft(spec, dim=-1, norm="forward") * _twiddle(N1, N2).conj()       # (unscaled inverses: 1/N sits in H)
    return torch.fft.ifft(a, dim=-2, norm="forward").reshape(spec.shape[:-2] + (N1 * N2,))


def long_restated(x, w, bias, pad_left, pad_right, flip, keep, groups, factors=None):
    """What fc_long_forward computes, pass for pass, in float64 on the CPU."""
    B, cin, L = x.shape
    cout, cig, K = w.shape
    cog = cout // groups
    nout, keff, padl, tap0, step = _geom(L, K, pad_left, pad_right, flip, keep)
    N1, N2 = factors or _factor(nout + keff - 1)
    N = N1 * N2
    assert N >= nout + keff - 1
    # rows: position p holds x[p - padl]; two batch items per complex row, the last of an odd batch pairs with zeros
    pos = torch.arange(N) - padl
    ok = (pos >= 0) & (pos < L)
    xr = torch.zeros(B + B % 2, cin, N, dtype=x.dtype)
    xr[:B, :, ok] = x[:, :, pos[ok]]
    z = torch.complex(xr[0::2], xr[1::2])                                   # (pairs, Cin, N)
    # filter rows: position p < keff holds taps[tap0 + step*p]; spectrum conjugated (correlation) and scaled by 1/N
    u = torch.zeros(cout, cig, N, dtype=x.dtype)
    u[:, :, :keff] = w[:, :, [tap0 + step * p for p in range(keff)]]
    H = _two_passes(torch.complex(u, torch.zeros_like(u)), N1, N2).conj() / N
    Z = _two_passes(z, N1, N2).reshape(z.shape[0], groups, cig, N1, N2)
    Y = torch.einsum("pgiab,goiab->pgoab", Z, H.reshape(groups, cog, cig, N1, N2)).reshape(z.shape[0], cout, N1, N2)
    yz = _two_passes_back(Y, N1, N2)[..., :nout]
    y = torch.empty(B + B % 2, cout, nout, dtype=x.dtype)
    y[0::2], y[1::2] = yz.real, yz.imag
    y = y[:B]
    return y + bias[None, :, None] if bias is not None else y


def _expect(x, w, bias, padding, groups, causal):
    if causal:
        K = w.shape[2]
        return fft_conv_oracle_torch(F.pad(x, (K - 1, 0)), w.flip(-1), bias, groups=groups)
    return fft_conv_oracle_torch(x, w, bias, padding=padding, groups=groups)


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


CASES = [
    # B, cin, cout, groups, L, K, padding, causal
    (3, 4, 4, 4, 5000, 5000, 0, True),        # odd batch, depthwise, K = L
    (2, 6, 4, 2, 4500, 300, 100, False),      # groups, padding
    (1, 3, 5, 1, 4200, 1, 0, True),           # K = 1
    (5, 2, 2, 2, 2500, 5000, 0, True),        # K = 2L
    (2, 2, 2, 1, 3000, 3007, 0, True),        # K = L + 7
    (2, 2, 3, 1, 5000, 2999, 1499, False),    # 'same'-sized padding
    (3, 2, 2, 1, 4097, 9, 0, False),          # one sample past 64 x 64
]


@pytest.mark.parametrize("B,cin,cout,g,L,K,pad,causal", CASES)
def test_three_passes_restated_match_the_oracle(B, cin, cout, g, L, K, pad, causal):
    torch.manual_seed(L + K)
    x = torch.randn(B, cin, L, dtype=torch.float64)
    w = torch.randn(cout, cin // g, K, dtype=torch.float64)
    bias = torch.randn(cout, dtype=torch.float64)
    got = long_restated(x, w, bias, K - 1 if causal else pad, 0 if causal else pad, causal, L if causal else 0, g)
    want = _expect(x, w, bias, pad, g, causal)
    assert got.shape == want.shape
    assert _rel(got, want) <= F64_TOL


def test_restatement_holds_for_an_unbalanced_factorisation():
    torch.manual_seed(3)
    x = torch.randn(3, 2, 6000, dtype=torch.float64)
    w = torch.randn(2, 1, 2000, dtype=torch.float64)
    for factors in ((64, 128), (128, 64), (64, 256)):
        got = long_restated(x, w, None, 1999, 0, True, 6000, 2, factors)
        assert _rel(got, _expect(x, w, None, 0, 2, True)) <= F64_TOL


def _primitive(x, w, pad_left, pad_right, flip, keep, groups):
    """y[t] = sum_k u[k] * xpad[t + k], t < keep, through the restated passes."""
    return long_restated(x, w, None, pad_left, pad_right, flip, keep, groups)


@pytest.mark.parametrize("B,cin,cout,g,L,K,pad,causal", [
    (3, 3, 3, 3, 2500, 2500, 0, True),
    (2, 6, 4, 2, 3000, 1200, 100, False),
    (2, 2, 2, 1, 1500, 3000, 0, True),
])
def test_gradient_identities_match_autograd_through_the_oracle(B, cin, cout, g, L, K, pad, causal):
    """dX and dW as FFTLongConvFunction.backward forms them, on the restated primitive."""
    torch.manual_seed(K)
    cig, cog = cin // g, cout // g
    x = torch.randn(B, cin, L, dtype=torch.float64, requires_grad=True)
    w = torch.randn(cout, cig, K, dtype=torch.float64, requires_grad=True)
    y = _expect(x, w, None, pad, g, causal)
    gy = torch.randn_like(y)
    y.backward(gy)
    pl, pr = (K - 1, 0) if causal else (pad, pad)
    wt = w.detach().view(g, cog, cig, K).transpose(1, 2).reshape(cin, cog, K)
    dx = _primitive(gy, wt, K - 1 - pl, K - 1 - pr, not causal, L, g)
    xt = x.detach().view(B, g, cig, L).permute(2, 1, 0, 3).reshape(cig, g * B, L)
    du = _primitive(xt, gy.permute(1, 0, 2), pl, pr, False, K, g).permute(1, 0, 2)
    dw = du.flip(-1) if causal else du
    assert _rel(dx, x.grad) <= F64_TOL
    assert _rel(dw, w.grad) <= F64_TOL


def test_two_table_twiddle_is_float32_accurate_at_2_pow_24():
    """w_N^m = thi[m >> 12] * tlo[m & 4095], both tables rounded once from float64 as the host builds them, the product
    taken in float32: within one float32 ulp of 1 (2^-23, the magnitude of the twiddle) of the float64 value, on sampled
    rows k1 and every n2."""
    N1 = N2 = 4096
    N = N1 * N2
    tau = 2 * math.pi
    hi = np.exp(-1j * tau * (np.arange(N >> 12, dtype=np.float64) * 4096) / N).astype(np.complex64)
    lo = np.exp(-1j * tau * np.arange(4096, dtype=np.float64) / N).astype(np.complex64)
    rng = np.random.default_rng(0)
    worst = 0.0
    for k1 in [0, 1, 2, 4095, 2048, 1365] + list(rng.integers(0, N1, 26)):
        m = np.arange(N2, dtype=np.int64) * int(k1)
        a, b = hi[m >> 12], lo[m & 4095]
        re = (a.real * b.real - a.imag * b.imag).astype(np.float32)
        im = (a.real * b.imag + a.imag * b.real).astype(np.float32)
        want = np.exp(-1j * tau * m.astype(np.float64) / N)
        worst = max(worst, float(np.abs(re - want.real).max()), float(np.abs(im - want.imag).max()))
    assert worst <= 2.0 ** -23, worst


def _key(B, cin, cout, g, L, K, pl=0, pr=0, keep=0, flip=0, bias=0):
    return (B, cin, cout, g, L, K, pl, pr, keep, flip, bias)


@pytest.mark.parametrize("L,K", [(4096, 1), (4097, 9), (5000, 5000), (8192, 8192), (16384, 9), (16385, 9), (65536, 65536),
                                 (1 << 19, 1 << 19), ((1 << 20) - 5, (1 << 19) + 6), (1 << 23, 1 << 23)])
def test_factorisation_is_the_smallest_product_of_two_tile_lengths(L, K, monkeypatch):
    monkeypatch.delenv("FFTCONV_LONG_N", raising=False)
    info = _native.long_geometry(_key(3, 4, 4, 4, L, K, pl=K - 1, keep=L, flip=1))
    need = L + min(K, L) - 1
    N1, N2 = info["N1"], info["N2"]
    assert N1 in TILE_LENGTHS and N2 in TILE_LENGTHS and N2 >= N1
    assert N1 * N2 >= need and (N1 * N2 == 4096 or N1 * N2 // 2 < need)
    assert (N1, N2) == _factor(need)
    assert info["out_len"] == L
    assert info["spectrum_bytes"] == 4 * 1 * N1 * N2 * 8
    assert info["workspace_bytes"] == info["slab_pairs"] * (4 + 4) * N1 * N2 * 8
    assert info["slabs"] * info["slab_pairs"] >= 2


def test_non_causal_geometry_and_forced_factorisation(monkeypatch):
    monkeypatch.delenv("FFTCONV_LONG_N", raising=False)
    info = _native.long_geometry(_key(4, 8, 8, 1, 8192, 8192, pl=4096, pr=4096))
    assert (info["N1"], info["N2"], info["out_len"]) == (128, 128, 8193)
    monkeypatch.setenv("FFTCONV_LONG_N", "64x4096")
    info = _native.long_geometry(_key(4, 8, 8, 1, 8192, 8192, pl=4096, pr=4096))
    assert (info["N1"], info["N2"]) == (64, 4096)
    monkeypatch.setenv("FFTCONV_LONG_N", "64x64")
    with pytest.raises(ValueError, match="FFTCONV_LONG_N"):
        _native.long_geometry(_key(4, 8, 8, 1, 8192, 8192, pl=4096, pr=4096))
    monkeypatch.setenv("FFTCONV_LONG_N", "96x128")
    with pytest.raises(ValueError, match="FFTCONV_LONG_N"):
        _native.long_geometry(_key(4, 8, 8, 1, 8192, 8192, pl=4096, pr=4096))


def test_workspace_budget_cuts_the_batch_pairs_into_slabs(monkeypatch):
    monkeypatch.delenv("FFTCONV_LONG_N", raising=False)
    monkeypatch.setenv("FFTCONV_LONG_WS_MB", "1")
    info = _native.long_geometry(_key(7, 2, 2, 2, 8000, 100))       # N = 8192: 256 KiB per pair, 4 pairs
    assert (info["slab_pairs"], info["slabs"]) == (4, 1)
    info = _native.long_geometry(_key(7, 4, 4, 4, 16000, 100))      # N = 16384: 1 MiB per pair
    assert (info["slab_pairs"], info["slabs"]) == (1, 4)
    assert info["workspace_bytes"] == 8 * 16384 * 8


def test_transform_length_is_capped_at_2_pow_24(monkeypatch):
    monkeypatch.delenv("FFTCONV_LONG_N", raising=False)
    L = (1 << 23) + 1
    with pytest.raises(NotImplementedError, match=str(2 * L - 1)):
        _native.long_geometry(_key(1, 1, 1, 1, L, L, pl=L - 1, keep=L, flip=1))
    x = torch.zeros(1, 1, L)
    with pytest.raises(NotImplementedError, match=str(2 * L - 1)):
        F_.fft_long_conv(x, torch.zeros(1, 1, L), causal=True)


@pytest.mark.parametrize("key,match", [
    (_key(0, 1, 1, 1, 5000, 10), "positive"),
    (_key(1, 3, 4, 2, 5000, 10), "divisible"),
    (_key(1, 1, 1, 1, 5000, 6000), "longer than the padded row"),
    (_key(1, 1, 1, 1, 5000, 10, pl=-1), "negative"),
    (_key(1, 1, 1, 1, 5000, 10, keep=6000), "out_keep"),
    (_key(1, 1, 1, 1, 5000, 10, flip=2), "flip"),
])
def test_descriptor_errors(key, match):
    with pytest.raises(ValueError, match=match):
        _native.long_geometry(key)


def test_argument_errors_come_before_any_device_call():
    x, w = torch.zeros(2, 4, 6000), torch.zeros(4, 2, 3000)
    with pytest.raises(ValueError, match="channel mismatch"):
        F_.fft_long_conv(x, w, groups=1)
    with pytest.raises(ValueError, match="bias"):
        F_.fft_long_conv(x, w, torch.zeros(3), groups=2)
    with pytest.raises(ValueError, match="padding must be 0"):
        F_.fft_long_conv(x, w, groups=2, padding=1, causal=True)
    with pytest.raises(ValueError, match="padding"):
        F_.fft_long_conv(x, w, groups=2, padding="full")
    with pytest.raises(ValueError, match="padding"):
        F_.fft_long_conv(x, w, groups=2, padding=-1)
    with pytest.raises(ValueError, match="longer than the padded row"):
        F_.fft_long_conv(x, torch.zeros(4, 2, 7000), groups=2)
    with pytest.raises(ValueError, match="shapes"):
        F_.fft_long_conv(torch.zeros(2, 4, 10, 10), w, groups=2)


def test_cpu_tensors_and_other_dtypes_are_refused():
    x, w = torch.zeros(2, 4, 6000), torch.zeros(4, 2, 3000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F_.fft_long_conv(x, w, groups=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F_.fft_long_conv(x[..., :100], w[..., :50], groups=2, causal=True)       # short rows too


def test_module_is_a_conv1d_and_checks_its_arguments():
    from fft_conv_pytorch_amd import FFTLongConv1d
    layer = FFTLongConv1d(4, 6, 3000, groups=2, causal=True)
    assert isinstance(layer, torch.nn.Conv1d)
    assert set(layer.state_dict()) == {"weight", "bias"}
    assert tuple(layer.weight.shape) == (6, 2, 3000)
    torch.nn.Conv1d(4, 6, 3000, groups=2).load_state_dict(layer.state_dict())
    with pytest.raises(ValueError, match="padding must be 0"):
        FFTLongConv1d(4, 6, 3000, padding=5, causal=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer(torch.zeros(1, 4, 5000))


def test_header_exports_and_abi_agree():
    header = open(os.path.join(ROOT, "include", "fftconv_amd.h")).read()
    declared = set(re.findall(r"\b(fc_[a-z0-9_]+)\s*\(", header))
    long_calls = {"fc_long_geometry", "fc_long_plan_create", "fc_long_plan_destroy", "fc_long_plan_info",
                  "fc_long_transform_kernel", "fc_long_forward"}
    assert long_calls <= declared and declared == set(_native.EXPORTS)
    lib = _native.load_library()
    for name in long_calls:
        assert hasattr(lib, name), name
    m = re.search(r"#define\s+FC_ABI_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == _native.ABI_VERSION == lib.fc_version()
    import ctypes
    assert ctypes.sizeof(_native.FcLongDesc) == 9 * 8 + 2 * 4


def test_package_stays_free_of_the_oracle_and_of_vendor_ffts():
    """The two words tests/test_host.py forbids in the package's Python files, and no vendor FFT in the new sources."""
    pkg = os.path.join(ROOT, "fft_conv_pytorch_amd")
    for name in os.listdir(pkg):
        if name.endswith(".py"):
            text = open(os.path.join(pkg, name)).read()
            assert "oracle" not in text.replace("no CPU", ""), name
            assert "torch.fft" not in text.replace("no torch.fft", ""), name
    for name in ("long1d.hpp", "long_inst.hip", "host_long.cpp"):
        text = open(os.path.join(pkg, "csrc", name)).read().lower()
        assert "rocfft" not in text and "hipfft" not in text, name
