"""Host-side contract of float16 / bfloat16 I/O (no GPU): the C header's dtype codes and ABI version, and the Python
binding's dtype map that puts the I/O type into the plan key."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fftconv_amd.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_half_dtypes():
    text = _header()
    assert re.search(r"\bFC_F16\s*=\s*2\b", text)
    assert re.search(r"\bFC_BF16\s*=\s*3\b", text)


def test_abi_version_7_matches_binding():
    from fft_conv_pytorch_amd import _native
    m = re.search(r"#define\s+FC_ABI_VERSION\s+(\d+)", _header())
    assert m and int(m.group(1)) == 7
    assert _native.ABI_VERSION == int(m.group(1))


def test_dtype_codes_map_half_dtypes():
    from fft_conv_pytorch_amd import functional
    assert functional._DTYPE_CODES[torch.float16] == 2
    assert functional._DTYPE_CODES[torch.bfloat16] == 3
    assert functional._DTYPE_CODES[torch.float32] == 0 and functional._DTYPE_CODES[torch.float64] == 1
