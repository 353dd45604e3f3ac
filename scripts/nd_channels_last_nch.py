#!/usr/bin/env python3
"""Channels per workgroup of the channels-last row passes: the forward with a channels-last signal and
``channels_last=True`` at one depthwise shape per row transform length, float32 and bfloat16, twenty eager calls each with a
cached spectrum.  Run once per library build (``make EXTRA="-fno-slp-vectorize -DFC_CL_NCH=2|4|8" OUT=...``, picked up
through FFTCONV_LIB) under ``rocprofv3 --kernel-trace --stats -- python scripts/nd_channels_last_nch.py``: the kernel
statistics set ``rows_r2c_cl`` / ``rows_c2r_cl`` of the builds against each other and against the planar ``rows_r2c`` /
``rows_c2r`` of the contiguous call, which this script runs too.  It prints the median time of the whole forward per
variant as well (HIP events around each eager call), one JSON line per shape."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import fft_conv_pytorch_amd as fca  # noqa: E402

DEV = "cuda:0"
# (row transform, batch, channels, side, taps): depthwise, 'same' padding
SHAPES = [(64, 8, 256, 28, 27), (128, 8, 256, 56, 31), (512, 4, 64, 448, 31), (1024, 2, 64, 960, 31)]


def timed(fn, n=20):
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return round(statistics.median(out), 1)


if __name__ == "__main__":
    for Tx, B, C, S, k in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            layer = fca.FFTConv2d(C, C, k, padding=k // 2, groups=C, channels_last=True).to(DEV).to(dtype).eval()
            plain = fca.FFTConv2d(C, C, k, padding=k // 2, groups=C).to(DEV).to(dtype).eval()
            x = torch.randn(B, C, S, S, device=DEV).to(dtype)
            xc = x.contiguous(memory_format=torch.channels_last)
            plan = fca.functional._plan_for(x, plain.weight, plain.bias, 1, k // 2, 1, C, "constant")
            assert plan.route["Tx"] == Tx and plan.route["nxt"] == 1, plan.route
            with torch.no_grad():
                layer(xc), plain(x)
                torch.cuda.synchronize()
                row = {"Tx": Tx, "dtype": str(dtype).replace("torch.", ""), "B": B, "C": C, "side": S, "k": k,
                       "lib": os.environ.get("FFTCONV_LIB", ""), "channels_last_us": timed(lambda: layer(xc)),
                       "contiguous_us": timed(lambda: plain(x))}
            print(json.dumps(row), flush=True)
