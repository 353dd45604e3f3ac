"""float16 / bfloat16 tensors on the long-filter path, without a GPU: the two ``_io`` entry points are declared, exported
and bound; the element type is an argument of the call, so the descriptor, the plan key and the ABI version are what they
were; 16-bit CPU tensors are refused for their device, not for their dtype."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from fft_conv_pytorch_amd import FFTLongConv1d, _native
from fft_conv_pytorch_amd import functional as F_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IO_CALLS = {"fc_long_transform_kernel_io", "fc_long_forward_io"}


def _header():
    return open(os.path.join(ROOT, "include", "fftconv_amd.h")).read()


def test_header_declares_the_io_calls_with_their_dtype_arguments():
    flat = re.sub(r"\s+", " ", _header())
    assert re.search(r"int fc_long_transform_kernel_io\(const fc_long_plan\* plan, const void\* weight, int weight_dtype, "
                     r"void\* spectrum, void\* workspace, void\* hip_stream\);", flat)
    assert re.search(r"int fc_long_forward_io\(const fc_long_plan\* plan, const void\* x, int x_dtype, const void\* spectrum, "
                     r"const float\* bias, void\* y, int y_dtype, void\* workspace, void\* hip_stream\);", flat)


def test_exports_equal_the_header_and_the_library_has_them():
    declared = set(re.findall(r"\b(fc_[a-z0-9_]+)\s*\(", _header()))
    assert IO_CALLS <= declared and declared == set(_native.EXPORTS)
    lib = _native.load_library()
    for name in _native.EXPORTS:
        assert hasattr(lib, name), name
    assert lib.fc_long_transform_kernel_io.argtypes[2] is ctypes.c_int and len(lib.fc_long_transform_kernel_io.argtypes) == 6
    assert len(lib.fc_long_forward_io.argtypes) == 9
    assert lib.fc_long_forward_io.argtypes[2] is ctypes.c_int and lib.fc_long_forward_io.argtypes[6] is ctypes.c_int


def test_abi_version_descriptor_size_and_plan_key_are_unchanged():
    m = re.search(r"#define\s+FC_ABI_VERSION\s+(\d+)", _header())
    assert int(m.group(1)) == 7 == _native.ABI_VERSION == _native.load_library().fc_version()
    assert ctypes.sizeof(_native.FcLongDesc) == 80
    assert [name for name, _ in _native.FcLongDesc._fields_] == [
        "batch", "in_channels", "out_channels", "groups", "length", "kernel", "pad_left", "pad_right", "out_keep", "flip",
        "has_bias"]
    info = _native.long_geometry((3, 4, 4, 4, 5000, 5000, 4999, 0, 5000, 1, 1))      # the 11-word key
    assert (info["N1"], info["N2"], info["out_len"]) == (128, 128, 5000)
    with pytest.raises(ValueError):
        _native.long_geometry((3, 4, 4, 4, 5000, 5000, 4999, 0, 5000, 1, 1, 3))      # no twelfth (dtype) word


def test_dtype_arguments_of_the_python_handle_default_to_float32():
    tk = inspect.signature(_native.LongPlan.transform_kernel).parameters
    fw = inspect.signature(_native.LongPlan.forward).parameters
    assert tk["weight_dtype"].default == 0
    assert fw["x_dtype"].default == 0 and fw["y_dtype"].default == 0
    assert list(fw)[:7] == ["self", "x_ptr", "spectrum_ptr", "bias_ptr", "y_ptr", "workspace_ptr", "stream"]
    assert list(tk)[:5] == ["self", "weight_ptr", "spectrum_ptr", "workspace_ptr", "stream"]


def test_null_arguments_are_refused_before_the_dtype_is_read():
    lib = _native.load_library()
    assert lib.fc_long_forward_io(None, None, 2, None, None, None, 2, None, None) == _native.FC_ERR_INVALID
    assert lib.fc_long_transform_kernel_io(None, None, 3, None, None, None) == _native.FC_ERR_INVALID


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_16bit_cpu_tensors_are_refused_for_their_device(dtype):
    x, w, b = torch.zeros(2, 4, 6000, dtype=dtype), torch.zeros(4, 2, 3000, dtype=dtype), torch.zeros(4, dtype=dtype)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F_.fft_long_conv(x, w, b, groups=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F_.fft_long_conv(x, w, groups=2, causal=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F_.fft_long_conv(x[..., :100], w[..., :50], groups=2, causal=True)       # short rows too
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FFTLongConv1d(4, 4, 3000, groups=2, causal=True).to(dtype)(x)
