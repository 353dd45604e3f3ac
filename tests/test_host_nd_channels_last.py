"""Host-side contract of channels-last tensors in the 2-D / 3-D ``fft_conv`` / ``fft_conv_transpose`` and their modules (no
GPU): the C header's new entry points and layout codes, the pure function that decides how a tensor is taken, the argument
checks of ``channels_last`` and the module attribute."""
import copy
import ctypes
import os
import pickle
import re

import pytest
import torch

from fft_conv_pytorch_amd import FFTConv1d, FFTConv2d, FFTConv3d, FFTConvTranspose2d, FFTConvTranspose3d, _native, fft_conv
from fft_conv_pytorch_amd import functional as F_
from fft_conv_pytorch_amd.functional import fft_conv_transpose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "fftconv_amd.h")).read()


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_layout_calls_and_the_library_exports_them():
    text = _header()
    codes = re.search(r"enum fc_nd_layout \{([^}]*)\}", text).group(1)
    assert re.sub(r"\s+", "", codes) == "FC_ND_PLANAR=0,FC_ND_CHANNELS_LAST=1"
    assert (_native.ND_PLANAR, _native.ND_CHANNELS_LAST) == (0, 1)
    assert re.search(r"int fc_forward_lay\(const fc_plan\* plan, const float\* x, int x_layout, const void\* w_hat, "
                     r"const float\* bias, float\* y,\s+int y_layout, void\* workspace, void\* hip_stream\);", text)
    assert re.search(r"int fc_plan_takes_layout\(const fc_plan\* plan, int x_layout, int y_layout\);", text)
    declared = set(re.findall(r"\b(fc_[a-z0-9_]+)\s*\(", text))
    assert {"fc_forward_lay", "fc_plan_takes_layout"} <= declared and declared == set(_native.EXPORTS)
    lib = _native.load_library()
    i32 = ctypes.c_int
    assert len(lib.fc_forward_lay.argtypes) == 9
    assert [i for i, t in enumerate(lib.fc_forward_lay.argtypes) if t is i32] == [2, 6]
    assert lib.fc_plan_takes_layout.argtypes == [ctypes.c_void_p, i32, i32]
    # the header says in words where an element lies
    assert "((((b*SZ + z)*SY + y)*SX + x)*C + ch)" in text
    # nothing that existed changes: the ABI version, the 7-argument call, the descriptor, the route words
    assert re.search(r"#define\s+FC_ABI_VERSION\s+7\b", text) and lib.fc_version() == 7 == _native.ABI_VERSION
    assert len(lib.fc_forward.argtypes) == 7
    assert ctypes.sizeof(_native.FcDesc) == 200 and ctypes.sizeof(_native.FcLongDesc) == 80
    assert len(_native.ROUTE_KINDS) == 7 and len(_native.ROUTE_WORDS["f32_nd"]) == 15
    # the null check comes first
    assert lib.fc_forward_lay(None, None, 1, None, None, None, 1, None, None) == _native.FC_ERR_INVALID
    assert b"null" in lib.fc_last_error()
    assert lib.fc_plan_takes_layout(None, 0, 1) == _native.FC_ERR_INVALID


# ------------------------------------------------------------------------------------------------ the decision
def test_layout_decision():
    B, C, H, W = 3, 5, 4, 7
    x = torch.zeros(B, C, H, W)
    assert F_._nd_layout(x) == "planar"
    cl = x.to(memory_format=torch.channels_last)
    assert F_._nd_layout(cl) == "cl"
    assert F_._nd_layout(cl[1:]) == "cl" and cl[1:].storage_offset() != 0           # batch slice
    u = torch.zeros(B, H, W, C)
    assert F_._nd_layout(u.permute(0, 3, 1, 2)) == "cl"
    y = torch.zeros(B, C, H, W).to(memory_format=torch.channels_last)
    assert F_._nd_layout((y.permute(0, 2, 3, 1) @ torch.zeros(C, 6)).permute(0, 3, 1, 2)) == "cl"
    assert F_._nd_layout(torch.zeros(B, 1, H, W).to(memory_format=torch.channels_last)) == "planar"      # C = 1
    assert F_._nd_layout(cl[:, :3]) == "copy"                                         # channel slice
    assert F_._nd_layout(x[:, :, :, ::2]) == "copy" and F_._nd_layout(cl[:, :, ::2]) == "copy"
    assert F_._nd_layout(x[:, :3]) == "copy"
    # size-1 axes: whichever layout torch reports contiguous decides, planar first
    assert F_._nd_layout(torch.zeros(1, C, H, W).to(memory_format=torch.channels_last)) == "cl"
    assert F_._nd_layout(torch.zeros(B, C, 1, 1).to(memory_format=torch.channels_last)) == "planar"
    assert F_._nd_layout(torch.zeros(B, C, 1, W).to(memory_format=torch.channels_last)) == "cl"
    # expanded views are neither
    assert F_._nd_layout(torch.zeros(1, C, H, W).expand(B, C, H, W)) == "copy"
    assert F_._nd_layout(torch.zeros(B, H, W, 1).expand(B, H, W, C).permute(0, 3, 1, 2)) == "copy"
    # 5-D: channels_last_3d; a 4-D rule does not apply to it
    v = torch.zeros(B, C, 2, H, W)
    assert F_._nd_layout(v) == "planar"
    assert F_._nd_layout(v.to(memory_format=torch.channels_last_3d)) == "cl"
    assert F_._nd_layout(v.to(memory_format=torch.channels_last_3d)[:, 1:]) == "copy"
    # 3-D tensors have no channels-last layout here
    assert F_._nd_layout(torch.zeros(B, W, C).transpose(1, 2)) == "copy"
    assert F_._nd_layout(torch.zeros(B, C, W)) == "planar"


def test_channels_last_helpers_give_the_requested_strides():
    for shape in ((2, 5, 3, 4), (2, 1, 3, 4), (1, 5, 1, 4), (2, 5, 2, 3, 4)):
        t = torch.arange(float(torch.Size(shape).numel())).view(shape)
        out = F_._to_channels_last(t)
        n = len(shape) - 2
        assert out.shape == t.shape and torch.equal(out, t)
        assert out.permute((0,) + tuple(range(2, n + 2)) + (1,)).is_contiguous()
        e = F_._empty_channels_last(shape, torch.float16, "cpu")
        assert e.stride() == out.stride() and e.dtype == torch.float16


def test_knob_is_read_per_call(monkeypatch):
    monkeypatch.setenv("FFTCONV_ND_CL", "1")
    # which calls take layouts natively: with the keyword unless the knob is 0, without it only under the knob 1
    for knob, with_keyword, without in ((None, True, False), ("0", False, False), ("1", True, True)):
        if knob is None:
            monkeypatch.delenv("FFTCONV_ND_CL")
        else:
            monkeypatch.setenv("FFTCONV_ND_CL", knob)
        assert (F_._nd_cl_native(True), F_._nd_cl_native(False)) == (with_keyword, without)


# ------------------------------------------------------------------------------------------------ arguments
def test_channels_last_argument_checks_come_before_the_device_gate():
    x, w = torch.zeros(2, 3, 8, 9), torch.zeros(4, 3, 3, 3)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="channels_last must be a bool"):
            fft_conv(x, w, channels_last=bad)
        with pytest.raises(ValueError, match="channels_last must be a bool"):
            fft_conv_transpose(x, torch.zeros(3, 4, 3, 3), channels_last=bad)
    with pytest.raises(ValueError, match="fft_long_conv"):
        fft_conv(torch.zeros(2, 3, 50), torch.zeros(4, 3, 5), channels_last=True)
    with pytest.raises(ValueError, match="fft_long_conv"):
        fft_conv_transpose(torch.zeros(2, 3, 50), torch.zeros(3, 4, 5), channels_last=True)
    # a valid keyword reaches the device gate (CPU tensors: RuntimeError, as ever), positional use is not offered
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        fft_conv(x, w, channels_last=True)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        fft_conv(torch.zeros(2, 3, 50), torch.zeros(4, 3, 5), channels_last=False)
    with pytest.raises(TypeError):
        fft_conv(x, w, None, 1, 0, 1, 1, "constant", True)


# ------------------------------------------------------------------------------------------------ modules
@pytest.mark.parametrize("cls,args", [(FFTConv2d, (3, 4, 3)), (FFTConv3d, (3, 4, 3)), (FFTConvTranspose2d, (3, 4, 3)),
                                      (FFTConvTranspose3d, (3, 4, 3))], ids=lambda v: getattr(v, "__name__", ""))
def test_module_attribute_repr_copies_and_state_dict(cls, args):
    assert cls.channels_last is False
    plain = cls(*args)
    assert plain.channels_last is False and "channels_last" not in repr(plain)
    layer = cls(*args, channels_last=True)
    assert layer.channels_last is True and "channels_last=True" in repr(layer)
    assert set(layer.state_dict()) == {"weight", "bias"} == set(plain.state_dict())
    plain.load_state_dict(layer.state_dict())
    for other in (copy.deepcopy(layer), pickle.loads(pickle.dumps(layer))):
        assert other.channels_last is True and torch.equal(other.weight, layer.weight)
    with pytest.raises(ValueError, match="channels_last must be a bool"):
        cls(*args, channels_last=1)
    with pytest.raises(TypeError):
        cls(*args, 1, 0, 1, 1, True, "zeros", None, None, True) if "Transpose" not in cls.__name__ else \
            cls(*args, 1, 0, 0, 1, True, 1, "zeros", None, None, True)
    # a module pickled before the attribute existed: the class default
    old = cls(*args)
    del old.__dict__["channels_last"]
    assert pickle.loads(pickle.dumps(old)).channels_last is False


def test_1d_module_takes_no_such_keyword():
    with pytest.raises(TypeError):
        FFTConv1d(3, 4, 3, channels_last=True)
    assert FFTConv1d(3, 4, 3).channels_last is False
