#!/usr/bin/env python3
"""Graph-replayed times of N-d kernels that run in segments of taps: this library's forward (cached kernel
spectrum, module in eval()) and a training step (forward + backward: dX, dW, db), against the reference's torch.fft
formulation (float32 rfftn / complex matmul / irfftn, fft_conv_pytorch functional.py:66-75) and torch's direct convolution
on the same GPU.  Each step is captured once into a HIP graph after a warm-up and replayed `iters` times between HIP events;
a step that cannot be captured is timed eagerly and marked so.  One JSON line per (shape, implementation).

    python scripts/time_nd_segments.py [--only train] [--iters N]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fft_conv_pytorch_amd as fca  # noqa: E402
from fft_conv_pytorch_amd import functional as fc  # noqa: E402

DEV = "cuda:0"
# (name, batch, cin, cout, spatial, kernel, stride, padding, dilation, transposed) -- the forward shapes of
# tests/test_gpu_nd_segments.py (kernels past 4096 taps)
FORWARD = [
    ("2-D x 12x9000 k 3x5000", 1, 3, 4, (12, 9000), (3, 5000), (1, 1), (1, 2000), (1, 1), False),
    ("2-D x 10x6000 k 3x1100 d4", 1, 2, 2, (10, 6000), (3, 1100), (1, 1), (1, 300), (1, 4), False),
    ("2-D x 5000x16 k 4500x3 s2", 1, 2, 2, (5000, 16), (4500, 3), (2, 1), (0, 1), (1, 1), False),
    ("3-D x 3x4500x4 k 2x4200x3", 1, 2, 2, (3, 4500, 4), (2, 4200, 3), (1, 1, 1), (0, 100, 1), (1, 1, 1), False),
    ("2-D g2 x 18ch 6x5000 k 2x4300", 1, 18, 4, (6, 5000), (2, 4300), (1, 1), (0, 2), (1, 1), False),
    ("2-D transposed x 4x600 k 3x4500 s(1,2)", 1, 2, 6, (4, 600), (3, 4500), (1, 2), (1, 3), (1, 1), True),
]


def torch_fft_conv(x, w, b, stride, padding, dilation, transposed):
    """The reference's formulation in float32 (forward plans; groups 1 or more)."""
    n = x.ndim - 2
    if any(d != 1 for d in dilation):
        wd = w.new_zeros(list(w.shape[:2]) + [(k - 1) * d + 1 for k, d in zip(w.shape[2:], dilation)])
        wd[(slice(None), slice(None)) + tuple(slice(None, None, d) for d in dilation)] = w
        w = wd
    x = F.pad(x, [p for p in padding[::-1] for _ in range(2)])
    shape = [(s + 1) // 2 * 2 for s in x.shape[2:]]
    dims = tuple(range(-n, 0))
    xf = torch.fft.rfftn(x, shape, dim=dims)
    wf = torch.fft.rfftn(w, shape, dim=dims).conj()
    g = x.shape[1] // w.shape[1]
    xf = xf.view(xf.shape[0], g, -1, *xf.shape[2:])
    wf = wf.view(g, -1, *wf.shape[1:])
    yf = torch.einsum("bgi...,goi...->bgo...", xf, wf).reshape(xf.shape[0], -1, *xf.shape[3:])
    y = torch.fft.irfftn(yf, shape, dim=dims)
    y = y[tuple([slice(None)] * 2 + [slice(0, x.size(i) - w.size(i) + 1, stride[i - 2]) for i in range(2, x.ndim)])]
    return y + b.view([1, -1] + [1] * n)


def graph_time(step, iters, capture=True):
    """us per step: a HIP graph of one step replayed `iters` times; eager launches ('eager') for torch's direct
    convolution (not captured: a failed capture would leave the process' capture stream unusable) or when the capture
    fails."""
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    try:
        if not capture:
            raise RuntimeError("not captured")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        g.replay()
        torch.cuda.synchronize()
        run, mode = g.replay, "graph"
    except Exception as exc:          # (a library that cannot be captured: time it eagerly)
        if capture:
            print(json.dumps({"note": f"capture failed, eager timing: {str(exc)[:200]}"}), flush=True)
        torch.cuda.synchronize()
        run, mode = step, "eager"
    run()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters, mode


def forward_rows(iters):
    torch.manual_seed(0)
    for name, B, ci, co, S, k, s, p, d, tr in FORWARD:
        n = len(S)
        x = torch.randn(B, ci, *S, device=DEV)
        if tr:
            layer = (fca.FFTConvTranspose2d, fca.FFTConvTranspose3d)[n - 2](ci, co, k, stride=s, padding=p, dilation=d).to(DEV)
            ref = (F.conv_transpose2d, F.conv_transpose3d)[n - 2]
            direct = lambda: ref(x, layer.weight, layer.bias, stride=s, padding=p, dilation=d)  # noqa: E731
        else:
            g = 2 if "g2" in name else 1
            layer = (fca.FFTConv2d, fca.FFTConv3d)[n - 2](ci, co, k, stride=s, padding=p, dilation=d, groups=g).to(DEV)
            ref = (F.conv2d, F.conv3d)[n - 2]
            direct = lambda: ref(x, layer.weight, layer.bias, stride=s, padding=p, dilation=d, groups=layer.groups)  # noqa: E731
        layer.eval()
        plan = fc._plan_for(x, layer.weight, layer.bias, s, p, d, layer.groups, "constant", transposed=tr,
                            output_padding=(0,) * n)
        r = plan.route
        segs = [r[f"nseg{a}"] for a in range(n)]
        with torch.no_grad():
            rows = [("fftconv_amd (cached spectrum)", lambda: layer(x))]
            if not tr:
                rows.append(("torch.fft float32", lambda: torch_fft_conv(x, layer.weight, layer.bias, s, p, d, tr)))
            rows.append(("torch direct conv (F.conv)", direct))
            for impl, fn in rows:
                us, mode = graph_time(fn, iters, capture=fn is not direct)
                print(json.dumps({"shape": name, "impl": impl, "us": round(us, 1), "mode": mode, "segments": segs,
                                  "route": {k2: v for k2, v in r.items() if k2 in ("T", "ntiles", "Tx", "nxt", "Tm", "nyt")}}),
                      flush=True)


def train_rows(iters):
    """Training step FFTConv2d B2 3->4 16x8192 k3 padding 1 (forward + backward)."""
    torch.manual_seed(0)
    layer = fca.FFTConv2d(3, 4, 3, padding=1).to(DEV)
    x = torch.randn(2, 3, 16, 8192, device=DEV, requires_grad=True)
    w2 = layer.weight.detach().clone().requires_grad_()
    b2 = layer.bias.detach().clone().requires_grad_()
    name = "train FFTConv2d B2 3->4 16x8192 k3 (fwd + bwd)"
    from fft_conv_pytorch_amd import _native
    wp = _native.WgradPlan(_native.conv_desc(2, 2, 3, 4, 1, (16, 8192), (3, 3), (1, 1), (1, 1), (1, 1), 0))
    r = _native.read_route(wp._lib, wp._h)
    print(json.dumps({"shape": name, "dW plan": {k: r[k] for k in ("T", "ntiles", "Tx", "nxt", "nseg0", "nseg1", "seg_taps1")}}),
          flush=True)

    def ours():
        (layer(x) ** 2).sum().backward()

    def tfft():
        (torch_fft_conv(x, w2, b2, (1, 1), (1, 1), (1, 1), False) ** 2).sum().backward()

    def direct():
        (F.conv2d(x, w2, b2, padding=1) ** 2).sum().backward()

    for impl, fn in (("fftconv_amd", ours), ("torch.fft float32", tfft), ("torch direct conv (F.conv2d)", direct)):
        us, mode = graph_time(fn, iters, capture=fn is not direct)
        print(json.dumps({"shape": name, "impl": impl, "us": round(us, 1), "mode": mode}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("forward", "train"), default=None)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if a.only in (None, "forward"):
        forward_rows(a.iters)
    if a.only in (None, "train"):
        train_rows(a.iters)
