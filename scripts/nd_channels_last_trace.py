#!/usr/bin/env python3
"""Forward of the depthwise B8 C256 56^2 k31 shape, channels-last (``channels_last=True``) and contiguous, float32 and
bfloat16, twenty calls each with a cached spectrum: run under ``rocprofv3 --kernel-trace --stats -- python
scripts/nd_channels_last_trace.py`` to set the channels-last builds of the first and last pass against the planar ones
(DESIGN.md 4.3g)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import fft_conv_pytorch_amd as fca
fmt = torch.channels_last
for dtype in (torch.float32, torch.bfloat16):
    layer = fca.FFTConv2d(256, 256, 31, padding=15, groups=256, channels_last=True).to("cuda:0").to(dtype).eval()
    plain = fca.FFTConv2d(256, 256, 31, padding=15, groups=256).to("cuda:0").to(dtype).eval()
    x = torch.randn(8, 256, 56, 56, device="cuda:0").to(dtype)
    xc = x.contiguous(memory_format=fmt)
    with torch.no_grad():
        for _ in range(20):
            layer(xc)
            plain(x)
    torch.cuda.synchronize()
print("traced")
