#!/usr/bin/env python3
"""Eager forward calls of (a) strided in / channels_last out and (c) the (B, C, L)-contiguous call of scripts/long_nlc_bench.py,
twelve each in turn, for a kernel trace in a run of its own: README's depthwise B4 C256 K = L = 65536 in
float32 and bfloat16, then dense B4 8 -> 8 K = L = 32768.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o nlc -- python scripts/long_nlc_trace.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fft_conv_pytorch_amd as fca  # noqa: E402
for B, C, g, L, dtypes in ((4, 256, 256, 65536, (torch.float32, torch.bfloat16)), (4, 8, 1, 32768, (torch.float32,))):
    for dtype in dtypes:
        torch.manual_seed(0)
        u = torch.randn(B, L, C, device="cuda:0").to(dtype)
        layer = fca.FFTLongConv1d(C, C, L, groups=g, bias=False, causal=True).to("cuda:0").to(dtype).eval()
        nlc = fca.FFTLongConv1d(C, C, L, groups=g, bias=False, causal=True, channels_last=True).to("cuda:0").to(dtype).eval()
        x = u.transpose(1, 2).contiguous()
        with torch.no_grad():
            for _ in range(12):
                nlc(u.transpose(1, 2))
                layer(x)
        torch.cuda.synchronize()
print("done")
