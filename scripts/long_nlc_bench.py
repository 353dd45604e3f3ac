#!/usr/bin/env python3
"""(batch, length, channels) activations through ``fft_long_conv``: the channels-last builds of the column
kernels against the two torch transposes a caller had to pay before.  The user's data is u (B, L, C) contiguous on both
sides; per shape and dtype, causal K = L:

  a_nlc        this commit: eval() FFTLongConv1d(channels_last=True) on u.transpose(1, 2), the result viewed (B, L, C)
  b_knob       layer(u.transpose(1, 2)).transpose(1, 2).contiguous() under FFTCONV_LONG_NLC=0 -- the cross-check of the
               baseline on this commit, not the baseline
  c_floor      the (B, C, L)-contiguous call alone: what the convolution costs when no layout change is needed
  *_train      forward + backward (dU, dW) of the same three on leaves

``--baseline`` times only ``fft_long_conv(u.transpose(1, 2), ...).transpose(1, 2).contiguous()`` (b_parent) through what
the parent commit's public interface has, so that the same file runs on a checkout of the parent: that is the baseline.

Every step is captured into a HIP graph after a warm-up (cached kernel spectra in the forward steps); the graphs of one
(shape, dtype) are replayed in turn between HIP events and the median replay is reported.  The peak memory a call adds on
top of its inputs is taken from one eager call per step.  One JSON line per (shape, dtype) is appended to --out.

    python scripts/long_nlc_bench.py [--iters 20] [--out profiles/long_nlc.jsonl] [--only SUBSTRING] [--no-train] [--baseline]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fft_conv_pytorch_amd as fca  # noqa: E402
from long_conv_bench import DEV, capture, timed  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
# (name, batch, cin, cout, groups, L = K, dtypes)
SHAPES = [
    ("depthwise B4 C256 K=L=65536", 4, 256, 256, 256, 65536, (F32, BF16)),
    ("depthwise B4 C256 K=L=262144", 4, 256, 256, 256, 262144, (F32,)),
    ("depthwise B8 C768 K=L=8192", 8, 768, 768, 768, 8192, (BF16,)),
    ("dense B4 8->8 K=L=32768", 4, 8, 8, 1, 32768, (F32,)),
]


def added_peak(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def run_shape(name, B, ci, co, g, L, dtype, iters, train, baseline):
    torch.manual_seed(0)
    u = torch.randn(B, L, ci, device=DEV).to(dtype)
    row = {"shape": name, "dtype": str(dtype).replace("torch.", ""), "B": B, "cin": ci, "cout": co, "groups": g, "L": L, "K": L,
           "causal": True, "device": torch.cuda.get_device_name(0), "iters": iters, "mode": "baseline" if baseline else "nlc"}
    plain = fca.FFTLongConv1d(ci, co, L, groups=g, bias=False, causal=True).to(DEV)
    with torch.no_grad():
        plain.weight.copy_(torch.randn(co, ci // g, L, device=DEV) / (ci // g * L) ** 0.5)
    plain = plain.to(dtype).eval()
    wg = plain.weight.detach().clone().requires_grad_()
    ug = u.clone().requires_grad_()
    gy = torch.randn(B, L, co, device=DEV).to(dtype)

    def knob(value, fn):
        def step():
            os.environ["FFTCONV_LONG_NLC"] = value
            return fn()
        return step

    def by_hand(layer_or_w):
        # what every caller of the parent commit writes
        if isinstance(layer_or_w, torch.nn.Module):
            return lambda: layer_or_w(u.transpose(1, 2)).transpose(1, 2).contiguous()
        return lambda: torch.autograd.grad(
            fca.fft_long_conv(ug.transpose(1, 2), wg, groups=g, causal=True).transpose(1, 2).contiguous(), (ug, wg), gy)

    if baseline:
        steps = {"b_parent": by_hand(plain)}
        if train:
            steps["b_parent_train"] = by_hand(None)
    else:
        import copy
        nlc = copy.deepcopy(plain)
        nlc.channels_last = True
        x = u.transpose(1, 2).contiguous()
        xg = x.clone().requires_grad_()
        gyc = gy.transpose(1, 2).contiguous()
        steps = {"a_nlc": knob("1", lambda: nlc(u.transpose(1, 2)).transpose(1, 2)),
                 "b_knob": knob("0", by_hand(plain)),
                 "c_floor": knob("1", lambda: plain(x))}
        if train:
            steps["a_nlc_train"] = knob("1", lambda: torch.autograd.grad(
                fca.fft_long_conv(ug.transpose(1, 2), wg, groups=g, causal=True, channels_last=True).transpose(1, 2), (ug, wg), gy))
            steps["b_knob_train"] = knob("0", by_hand(None))
            steps["c_floor_train"] = knob("1", lambda: torch.autograd.grad(
                fca.fft_long_conv(xg, wg, groups=g, causal=True), (xg, wg), gyc))
    no_grad = {key: not key.endswith("train") for key in steps}

    def call(key):
        if no_grad[key]:
            with torch.no_grad():
                return steps[key]()
        return steps[key]()

    if not baseline:
        with torch.no_grad():
            ya, yb, yc = steps["a_nlc"](), steps["b_knob"](), steps["c_floor"]()
            assert ya.is_contiguous() and yb.is_contiguous()
            row["fwd_bits_equal"] = bool(torch.equal(ya, yb) and torch.equal(ya, yc.transpose(1, 2)))
            del ya, yb, yc
        if train:
            ga, gb, gc = steps["a_nlc_train"](), steps["b_knob_train"](), steps["c_floor_train"]()
            row["train_bits_equal"] = bool(torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])
                                           and torch.equal(ga[0], gc[0].transpose(1, 2)) and torch.equal(ga[1], gc[1]))
            row["du_contiguous"] = bool(ga[0].is_contiguous())
            del ga, gb, gc
    for key in steps:
        call(key)
        row[key + "_peak_bytes"] = added_peak(lambda: call(key))
    graphs = {key: capture(lambda: call(key)) for key in steps}
    samples = {key: [] for key in graphs}
    for _ in range(iters):
        for key, gr in graphs.items():          # in turn
            samples[key].append(timed(gr))
    for key, vals in samples.items():
        row[key + "_us"] = round(statistics.median(vals), 1)
        row[key + "_min_us"] = round(min(vals), 1)
    if not baseline:
        row["a_over_b_knob"] = round(row["a_nlc_us"] / row["b_knob_us"], 3)
        row["a_over_c"] = round(row["a_nlc_us"] / row["c_floor_us"], 3)
        if train:
            row["a_over_b_knob_train"] = round(row["a_nlc_train_us"] / row["b_knob_train_us"], 3)
            row["a_over_c_train"] = round(row["a_nlc_train_us"] / row["c_floor_train_us"], 3)
    os.environ.pop("FFTCONV_LONG_NLC", None)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "long_nlc.jsonl"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--tag", default=None, help="free text recorded with every row (a library variant, for instance)")
    a = ap.parse_args()
    for name, B, ci, co, g, L, dtypes in SHAPES:
        if a.only and a.only not in name:
            continue
        for dtype in dtypes:
            res = run_shape(name, B, ci, co, g, L, dtype, iters=a.iters, train=not a.no_train, baseline=a.baseline)
            if a.tag:
                res["tag"] = a.tag
            line = json.dumps(res)
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
            torch.cuda.empty_cache()
