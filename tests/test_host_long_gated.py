"""``fft_long_conv_gated`` without a GPU: argument checks of the gates, the table of ``_long_gated_route``, exports, header
and binding of ``fc_long_forward_gated``, and the dispatch of a call without gates."""
import inspect
import os
import re

import pytest
import torch

import fft_conv_pytorch_amd as pkg
from fft_conv_pytorch_amd import FFTLongConv1d, _native, fft_long_conv_gated
from fft_conv_pytorch_amd import functional as F_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, BF16, C64, F64 = torch.float32, torch.float16, torch.bfloat16, torch.complex64, torch.float64


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    for k in ("FFTCONV_LONG_DECIM", "FFTCONV_LONG_NLC", "FFTCONV_LONG_N", "FFTCONV_LONG_WS_MB", "FFTCONV_HALF_IO",
              "FFTCONV_LONG_WGRAD"):
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------------ 1. argument errors
B, CIN, COUT, G, L, K, PAD = 2, 6, 4, 2, 3000, 1801, 300
NOUT = L + 2 * PAD - K + 1


def _call(pregate=None, postgate=None, **kw):
    x, w = torch.zeros(B, CIN, L), torch.zeros(COUT, CIN // G, K)
    return fft_long_conv_gated(x, w, None, PAD, G, pregate=pregate, postgate=postgate, **kw)


@pytest.mark.parametrize("shape", [(B, CIN, L - 1), (B, CIN + 1, L), (B + 1, CIN, L), (CIN, L), (B, COUT, NOUT), (1, CIN, L),
                                   (B, CIN, 1)])
def test_pregate_of_another_shape(shape):
    with pytest.raises(ValueError, match="`pregate` must have the signal's shape"):
        _call(pregate=torch.zeros(shape))


@pytest.mark.parametrize("shape", [(B, COUT, NOUT - 1), (B, COUT, NOUT + 1), (B, CIN, NOUT), (B, CIN, L), (COUT, NOUT),
                                   (1, COUT, NOUT), (B, COUT, 1)])
def test_postgate_of_another_shape(shape):
    with pytest.raises(ValueError, match="`postgate` must have the result's shape"):
        _call(postgate=torch.zeros(shape))


def test_postgate_shape_follows_the_call():
    """The result's shape, not the signal's: causal keeps ceil(L / stride) samples, a stride and a dilation change nout."""
    x, w = torch.zeros(B, 4, 5000), torch.zeros(4, 1, 3000)
    for kw, nout in ((dict(causal=True), 5000), (dict(causal=True, stride=3), 1667), (dict(padding=0), 2001),
                     (dict(padding=10, dilation=1, stride=2), (5000 + 20 - 3000) // 2 + 1)):
        with pytest.raises(ValueError, match=rf"result's shape \({B}, 4, {nout}\)"):
            fft_long_conv_gated(x, w, None, groups=4, postgate=torch.zeros(B, 4, nout + 1), **kw)
        with pytest.raises(RuntimeError, match="ROCm devices only"):      # the right shape passes the gate checks
            fft_long_conv_gated(x, w, None, groups=4, postgate=torch.zeros(B, 4, nout), **kw)


@pytest.mark.parametrize("dtype", [F16, BF16, F64, C64, torch.int32])
@pytest.mark.parametrize("which", ["pregate", "postgate"])
def test_gate_of_another_dtype(which, dtype):
    shape = (B, CIN, L) if which == "pregate" else (B, COUT, NOUT)
    with pytest.raises(TypeError, match=f"`{which}` has dtype"):
        _call(**{which: torch.zeros(shape, dtype=dtype)})


@pytest.mark.parametrize("which", ["pregate", "postgate"])
def test_gate_on_another_device(which):
    shape = (B, CIN, L) if which == "pregate" else (B, COUT, NOUT)
    with pytest.raises(ValueError, match=f"`{which}` is on meta but the signal is on cpu"):
        _call(**{which: torch.zeros(shape, device="meta")})


def test_gate_that_is_no_tensor():
    with pytest.raises(TypeError, match="`pregate` must be a tensor or None"):
        _call(pregate=1.0)


def test_the_checks_of_fft_long_conv_come_first():
    with pytest.raises(ValueError, match="channel mismatch"):
        fft_long_conv_gated(torch.zeros(2, 5, 3000), torch.zeros(4, 3, 100), pregate=torch.zeros(2, 5, 3000))
    with pytest.raises(ValueError, match="channels_last must be a bool"):
        _call(pregate=torch.zeros(B, CIN, L), channels_last=1)


# ------------------------------------------------------------------------------------------------ 2. the route
BASE = dict(signal_shape=(3, 5, 2500), kernel_shape=(5, 1, 2500), groups=5, causal=True)


def _route(**kw):
    return F_._long_gated_route(**{**BASE, **kw})


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_fused_calls(dtype):
    assert _route(dtype=dtype) == "fused"
    assert _route(dtype=dtype, x_layout="copy") == "fused"                      # a slice: copied, then fused
    assert F_._long_gated_route((2, 6, 4000), (4, 3, 2401), padding=400, groups=2, dtype=dtype) == "fused"
    assert F_._long_gated_route((2, 6, 4000), (4, 3, 2401), padding="same", groups=2, dtype=dtype, padding_mode="zeros") == "fused"
    # (a padded row of 3600 samples is one tile of fft_conv: it hands off, gates and all)
    assert F_._long_gated_route((2, 6, 3000), (4, 3, 1801), padding=300, groups=2, dtype=dtype) == "composed"


INELIGIBLE = {
    "complex64": dict(dtype=C64),
    "stride": dict(stride=2),
    "dilation": dict(dilation=2),
    "reflect": dict(causal=False, padding=1000, padding_mode="reflect"),
    "replicate": dict(causal=False, padding=1000, padding_mode="replicate"),
    "circular": dict(causal=False, padding=1000, padding_mode="circular"),
    "channels_last result": dict(channels_last=True),
    "channels-last signal": dict(x_layout="nlc"),
    "handoff": dict(signal_shape=(3, 5, 1000), kernel_shape=(5, 1, 1000)),
}


@pytest.mark.parametrize("name", sorted(INELIGIBLE))
def test_each_ineligibility_alone_composes(name):
    kw = INELIGIBLE[name]
    if name in ("reflect", "replicate", "circular"):      # the same call with zero padding is fused
        assert _route(**{**kw, "padding_mode": "constant"}) == "fused"
    assert _route(**kw) == "composed"


def test_phases_route_composes(monkeypatch):
    monkeypatch.setenv("FFTCONV_LONG_DECIM", "1")
    assert F_._long_route(BASE["signal_shape"], BASE["kernel_shape"], stride=2, groups=5, causal=True) == "phases"
    assert _route(stride=2) == "composed"
    assert _route() == "fused"                            # (stride 1 is no phases route whatever the variable says)


def test_cast_path_composes(monkeypatch):
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    assert _route(dtype=BF16) == "composed" and _route(dtype=F16) == "composed"
    assert _route(dtype=F32) == "fused"


def test_route_is_pure_and_has_no_switch():
    src = inspect.getsource(F_._long_gated_route) + inspect.getsource(F_._long_gated_route_of)
    assert re.findall(r"FFTCONV_[A-Z_]+", src.split('"""')[-1]) == ["FFTCONV_HALF_IO"]
    with pytest.raises(NotImplementedError):
        F_._long_gated_route((1, 1, 1 << 24), (1, 1, 2), causal=True)      # as _long_route answers


# ------------------------------------------------------------------------------------------------ 3. exports, header, binding
def test_names_are_exported():
    assert pkg.fft_long_conv_gated is F_.fft_long_conv_gated and "fft_long_conv_gated" in F_.__all__
    from fft_conv_pytorch_amd.autograd import FFTLongConvGatedFunction
    assert issubclass(FFTLongConvGatedFunction, torch.autograd.Function)
    sig = inspect.signature(fft_long_conv_gated)
    assert list(sig.parameters) == ["signal", "kernel", "bias", "padding", "groups", "causal", "pregate", "postgate", "stride",
                                    "dilation", "padding_mode", "channels_last"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[6:])
    assert list(inspect.signature(FFTLongConv1d.forward).parameters) == ["self", "signal", "pregate", "postgate"]
    assert "kernel[..., 0] += D" in fft_long_conv_gated.__doc__


def test_one_new_entry_point_and_abi_7():
    header = open(os.path.join(ROOT, "include", "fftconv_amd.h")).read()
    declared = set(re.findall(r"\b(fc_[a-z0-9_]+)\s*\(", header))
    assert "fc_long_forward_gated" in declared and declared == set(_native.EXPORTS)
    assert _native.EXPORTS[-1] == "fc_long_forward_gated"                     # appended
    decl = re.search(r"int fc_long_forward_gated\((.*?)\);", header, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert params == ["const fc_long_plan* plan", "const void* x", "int x_dtype", "const void* pregate", "const void* spectrum",
                      "const float* bias", "void* y", "const void* gate", "void* y2", "const void* gate2", "int y_dtype",
                      "int y2_dtype", "void* workspace", "void* hip_stream"]
    import ctypes
    restype, argtypes = _native.SIGNATURES["fc_long_forward_gated"]
    assert restype is ctypes.c_int
    assert [a is ctypes.c_int for a in argtypes] == ["int " in p and "*" not in p for p in params]
    assert all(a is ctypes.c_void_p for a, p in zip(argtypes, params) if "*" in p)
    lib = _native.load_library()
    for name in _native.EXPORTS:
        assert hasattr(lib, name), name
    m = re.search(r"#define\s+FC_ABI_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == 7 == _native.ABI_VERSION == lib.fc_version()
    assert "fc_long_forward_gated" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_null_arguments_are_refused_without_a_device():
    lib = _native.load_library()
    assert lib.fc_long_forward_gated(None, None, 0, None, None, None, None, None, None, None, 0, 0, None, None) == _native.FC_ERR_INVALID
    assert b"null argument" in lib.fc_last_error()


# ------------------------------------------------------------------------------------------------ 4. no gates
def test_without_gates_the_call_is_fft_long_conv(monkeypatch):
    seen = []
    monkeypatch.setattr(F_, "_fft_long_conv_impl", lambda *a: seen.append(a) or "result")
    x, w, b = torch.zeros(2, 4, 5000), torch.zeros(4, 1, 100), torch.zeros(4)
    out = fft_long_conv_gated(x, w, b, 7, 4, False, stride=2, dilation=3, padding_mode="reflect", channels_last=True)
    assert out == "result"
    assert len(seen) == 1 and seen[0][0] is x and seen[0][1] is w and seen[0][2] is b
    assert seen[0][3:] == (7, 4, False, None, 2, 3, "reflect", True)


def test_module_without_gates_is_the_call_it_was(monkeypatch):
    seen = []
    monkeypatch.setattr(F_, "_fft_long_conv_impl", lambda *a: seen.append(("plain", a)) or "plain")
    monkeypatch.setattr(F_, "_fft_long_conv_gated_impl", lambda *a: seen.append(("gated", a)) or "gated")
    m = FFTLongConv1d(4, 4, 100, groups=4, causal=True)
    x, p = torch.zeros(2, 4, 5000), torch.ones(2, 4, 5000)
    assert m(x) == "plain" and seen[-1][0] == "plain"
    assert m(x, pregate=p) == "gated" and seen[-1][1][7] is p and seen[-1][1][8] is None
    assert m(x, None, p) == "gated" and seen[-1][1][7] is None and seen[-1][1][8] is p
