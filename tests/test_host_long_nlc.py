"""Host-side contract of (batch, length, channels) tensors in ``fft_long_conv`` / ``FFTLongConv1d`` (no GPU): the C
header's new entry point and layout codes, the pure function that decides how a tensor is taken, the argument checks of
``channels_last`` and the module attribute."""
import copy
import ctypes
import os
import pickle
import re

import pytest
import torch

from fft_conv_pytorch_amd import FFTLongConv1d, _native, fft_long_conv
from fft_conv_pytorch_amd import functional as F_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "fftconv_amd.h")).read()


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_layout_call_and_the_library_exports_it():
    text = _header()
    codes = re.search(r"enum fc_long_layout \{([^}]*)\}", text).group(1)
    assert re.sub(r"\s+", "", codes) == "FC_LONG_NCL=0,FC_LONG_NLC=1"
    assert (_native.LONG_NCL, _native.LONG_NLC) == (0, 1)
    assert re.search(r"int fc_long_forward_lay\(const fc_long_plan\* plan, const void\* x, int x_dtype, int x_layout, "
                     r"const void\* spectrum,\s+const float\* bias, void\* y, int y_dtype, int y_layout, void\* workspace, "
                     r"void\* hip_stream\);", text)
    declared = set(re.findall(r"\b(fc_[a-z0-9_]+)\s*\(", text))
    assert "fc_long_forward_lay" in declared and declared == set(_native.EXPORTS)
    lib = _native.load_library()
    assert hasattr(lib, "fc_long_forward_lay")
    i32 = ctypes.c_int
    assert len(lib.fc_long_forward_lay.argtypes) == 11
    assert [i for i, t in enumerate(lib.fc_long_forward_lay.argtypes) if t is i32] == [2, 3, 7, 8]
    # nothing that existed changes: the ABI version and the 9-argument call
    assert re.search(r"#define\s+FC_ABI_VERSION\s+7\b", text) and lib.fc_version() == 7 == _native.ABI_VERSION
    assert len(lib.fc_long_forward_io.argtypes) == 9
    # the null check comes first, as in the call it extends
    assert lib.fc_long_forward_lay(None, None, 0, 1, None, None, None, 0, 1, None, None) == _native.FC_ERR_INVALID
    assert b"null" in lib.fc_last_error()


# ------------------------------------------------------------------------------------------------ the decision
def test_layout_decision():
    B, L, C = 3, 7, 5
    assert F_._long_layout(torch.zeros(B, C, L)) == "ncl"
    u = torch.zeros(B, L, C)
    v = u.transpose(1, 2)
    assert tuple(v.stride()) == (L * C, 1, C) and F_._long_layout(v) == "nlc"
    big = torch.zeros(B + 1, L, C)
    w = big[1:].transpose(1, 2)
    assert w.storage_offset() == L * C and w.shape == (B, C, L) and F_._long_layout(w) == "nlc"
    flat = torch.zeros(B * L * C + 3)
    odd = flat[3:].view(B, L, C).transpose(1, 2)
    assert odd.storage_offset() == 3 and F_._long_layout(odd) == "nlc"
    assert F_._long_layout(torch.zeros(1, L, C).transpose(1, 2)) == "nlc"       # one batch item, the same strides
    # a tensor that is both is the (B, C, L) one
    assert F_._long_layout(torch.zeros(B, L, 1).transpose(1, 2)) == "ncl"       # C = 1
    assert F_._long_layout(torch.zeros(B, 1, C).transpose(1, 2)) == "ncl"       # L = 1
    # everything else is copied
    assert F_._long_layout(v[:, 1:4]) == "copy"                                  # channel-sliced view of an NLC tensor
    assert F_._long_layout(v[:, ::2]) == "copy"
    assert F_._long_layout(torch.zeros(1, C, L).expand(B, C, L)) == "copy"       # expanded
    assert F_._long_layout(torch.zeros(B, 1, L).expand(B, C, L)) == "copy"
    assert F_._long_layout(torch.zeros(B, C, 2 * L)[:, :, ::2]) == "copy"        # time-strided
    assert F_._long_layout(v[:, :, 1:]) == "copy"                                # time-sliced view of an NLC tensor
    assert F_._long_layout(torch.zeros(B, C, 2 * L)[:, :, :L]) == "copy"
    assert F_._long_layout(torch.zeros(L, B, C).permute(1, 2, 0)) == "copy"      # (L, B, C) storage
    # complex and 16-bit tensors: strides count elements, so the answers are the same
    for dtype in (torch.complex64, torch.bfloat16):
        assert F_._long_layout(torch.zeros(B, L, C, dtype=dtype).transpose(1, 2)) == "nlc"


def test_knob_is_read_per_call(monkeypatch):
    monkeypatch.delenv("FFTCONV_LONG_NLC", raising=False)
    assert F_._long_nlc_enabled()
    monkeypatch.setenv("FFTCONV_LONG_NLC", "0")
    assert not F_._long_nlc_enabled()
    monkeypatch.setenv("FFTCONV_LONG_NLC", "1")
    assert F_._long_nlc_enabled()


def test_as_channels_last_gives_the_requested_strides_without_a_second_copy():
    t = torch.arange(2 * 3 * 4, dtype=torch.float32).view(2, 3, 4)
    c = F_._as_channels_last(t)
    assert torch.equal(c, t) and tuple(c.stride()) == (12, 1, 3) and c.transpose(1, 2).is_contiguous()
    assert F_._as_channels_last(c).data_ptr() == c.data_ptr()


# ------------------------------------------------------------------------------------------------ arguments
def test_channels_last_argument_checks_come_before_the_device_gate():
    x, w, b = torch.zeros(2, 4, 5000), torch.zeros(4, 1, 5000), torch.zeros(4)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        fft_long_conv(x, w, b, groups=4, causal=True, channels_last=True)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        fft_long_conv(x.transpose(1, 2).contiguous().transpose(1, 2), w, b, groups=4, causal=True, channels_last=True)
    # the argument checks still come first
    with pytest.raises(ValueError, match="channel mismatch"):
        fft_long_conv(x, w, b, groups=2, causal=True, channels_last=True)
    for bad in (1, 0, None, "yes", torch.tensor(True)):
        with pytest.raises(ValueError, match="channels_last must be a bool"):
            fft_long_conv(x, w, b, groups=4, causal=True, channels_last=bad)
    with pytest.raises(TypeError):
        fft_long_conv(x, w, b, 0, 4, True, 1, 1, "constant", True)       # keyword-only


# ------------------------------------------------------------------------------------------------ module
def test_module_attribute_repr_copies_and_state_dict():
    layer = FFTLongConv1d(4, 4, 301, groups=2, causal=True, channels_last=True)
    assert layer.channels_last is True
    assert "causal=True" in layer.extra_repr() and layer.extra_repr().endswith("channels_last=True")
    plain = FFTLongConv1d(4, 4, 301, groups=2)
    assert plain.channels_last is False and "channels_last" not in plain.extra_repr()
    ref = torch.nn.Conv1d(4, 4, 301, groups=2)
    assert list(layer.state_dict()) == list(ref.state_dict()) == ["weight", "bias"]
    ref.load_state_dict(layer.state_dict())
    for other in (copy.deepcopy(layer), pickle.loads(pickle.dumps(layer))):
        assert other.channels_last is True and other.causal is True
        assert torch.equal(other.weight, layer.weight)
    with pytest.raises(ValueError, match="channels_last must be a bool"):
        FFTLongConv1d(4, 4, 301, channels_last=1)
    with pytest.raises(TypeError):
        FFTLongConv1d(4, 4, 301, 0, 1, True, False, None, None, True)       # keyword-only
    # a module pickled before the attribute existed reads it as False
    old = pickle.loads(pickle.dumps(plain))
    old.__dict__.pop("channels_last", None)
    old = pickle.loads(pickle.dumps(old))
    assert "channels_last" not in old.__dict__ and old.channels_last is False
    assert "channels_last" not in old.extra_repr()
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        layer(torch.zeros(1, 4, 5000))
