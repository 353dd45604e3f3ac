#!/usr/bin/env python3
"""float16 / bfloat16 ``fft_long_conv``: the column kernels reading and writing the 16-bit tensors against the
cast path a caller had to write before -- widen, the float32 function, round -- on the shapes of scripts/long_conv_bench.py,
per dtype:

  fwd_native     eval() FFTLongConv1d in the dtype, cached kernel spectrum
  fwd_cast       the float32 module (cached kernel spectrum) between x.float() and .to(dtype)
                 (FFTCONV_HALF_IO=0 on the 16-bit module computes the same and also re-transforms the kernel on every
                 call; the cached float32 module is the faster, hence the fairer, yardstick)
  train_native   forward + backward (dX, dW) of fft_long_conv on 16-bit leaves
  train_cast     the same with FFTCONV_HALF_IO=0: float32 copies in, float32 function, gradients rounded

Every step is captured into a HIP graph after a warm-up; the graphs of one (shape, dtype) are replayed in turn between HIP
events of their own and the median replay is reported, with native / cast ratios.  The peak memory a call adds on top of
its inputs is taken from one eager call per step.  The outputs of the two forward steps are compared bit for bit.  One JSON
line per (shape, dtype) is appended to --out.

    python scripts/long_half_bench.py [--iters 20] [--out profiles/long_half.jsonl] [--only SUBSTRING] [--no-train]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fft_conv_pytorch_amd as fca  # noqa: E402
from fft_conv_pytorch_amd import functional as fc  # noqa: E402
from long_conv_bench import DEV, SHAPES, capture, timed  # noqa: E402


def added_peak(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def run_shape(name, B, ci, co, g, L, K, dtype, iters, train):
    torch.manual_seed(0)
    p = K // 2
    x = torch.randn(B, ci, L, device=DEV).to(dtype)
    plan = fc._long_plan(x, co, g, K, p, p, False, 0, False)
    row = {"shape": name, "dtype": str(dtype).replace("torch.", ""), "B": B, "cin": ci, "cout": co, "groups": g, "L": L, "K": K,
           "padding": p, "device": torch.cuda.get_device_name(0), "iters": iters,
           "long_plan": {k: plan.info[k] for k in ("N1", "N2", "slabs", "out_block")}}
    layer32 = fca.FFTLongConv1d(ci, co, K, padding=p, groups=g, bias=False).to(DEV).eval()
    with torch.no_grad():
        layer32.weight.copy_((torch.randn(co, ci // g, K, device=DEV) / K ** 0.5).to(dtype))      # (16-bit values)
    layer16 = fca.FFTLongConv1d(ci, co, K, padding=p, groups=g, bias=False).to(DEV).to(dtype).eval()
    with torch.no_grad():
        layer16.weight.copy_(layer32.weight)

    def knob(value, fn):
        def step():
            os.environ["FFTCONV_HALF_IO"] = value
            return fn()
        return step

    steps = {"fwd_native": knob("1", lambda: layer16(x)),
             "fwd_cast": knob("1", lambda: layer32(x.float()).to(dtype))}
    if train:
        xg = x.clone().requires_grad_()
        wg = layer16.weight.detach().clone().requires_grad_()
        with torch.no_grad():
            gy = torch.randn_like(layer16(x))
        grads = lambda: torch.autograd.grad(fca.fft_long_conv(xg, wg, padding=p, groups=g), (xg, wg), gy)    # noqa: E731
        steps["train_native"] = knob("1", grads)
        steps["train_cast"] = knob("0", grads)
    no_grad = {key: not key.startswith("train") for key in steps}

    def call(key):
        if no_grad[key]:
            with torch.no_grad():
                return steps[key]()
        return steps[key]()

    with torch.no_grad():
        ya, yb = steps["fwd_native"](), steps["fwd_cast"]()
        row["fwd_bits_equal"] = bool(torch.equal(ya.view(torch.int16), yb.view(torch.int16)))
        del ya, yb
    if train:
        ga, gb = steps["train_native"](), steps["train_cast"]()
        row["train_bits_equal"] = all(bool(torch.equal(a.view(torch.int16), b.view(torch.int16))) for a, b in zip(ga, gb))
        del ga, gb
    for key in steps:
        row[key + "_peak_bytes"] = added_peak(lambda: call(key))
    graphs = {key: capture(lambda: call(key)) for key in steps}
    samples = {key: [] for key in graphs}
    for _ in range(iters):
        for key, gr in graphs.items():          # in turn: native, cast, native, cast, ...
            samples[key].append(timed(gr))
    for key, vals in samples.items():
        row[key + "_us"] = round(statistics.median(vals), 1)
    row["fwd_native_over_cast"] = round(row["fwd_native_us"] / row["fwd_cast_us"], 3)
    if train:
        row["train_native_over_cast"] = round(row["train_native_us"] / row["train_cast_us"], 3)
    os.environ.pop("FFTCONV_HALF_IO", None)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "long_half.jsonl"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    for shape in SHAPES:
        if a.only and a.only not in shape[0]:
            continue
        for dtype in (torch.bfloat16, torch.float16):
            res = run_shape(*shape, dtype=dtype, iters=a.iters, train=not a.no_train)
            line = json.dumps(res)
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
            torch.cuda.empty_cache()
