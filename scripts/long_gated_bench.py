#!/usr/bin/env python3
"""The gated long convolution ("Gates in the column passes"): y = postgate * conv(pregate * x) + its training
step through a causal ``FFTLongConv1d`` with bias, three ways:

  a_fused      ``layer(x, pregate, postgate)``: ``fft_long_conv_gated``, the gates inside the column passes
  b_composed   ``postgate * layer(pregate * x)`` with torch multiplies, on the same tree
  c_parent     ``--baseline --root PARENT_CHECKOUT``: that same line with the package imported from a checkout of the parent
               commit (``FFTCONV_LIB`` may name its library), in a process of its own.

Per shape two things are measured: ``fwd``, the forward without autograd, and ``step``, forward and all five gradients
(x, weight, bias, pregate, postgate), each with ``torch.cuda.max_memory_allocated`` of one such call above what was allocated
before it (the forward runs on a copy of the module in eval() mode, which keeps its kernel spectrum; the step re-transforms the weight, as training does).

Every measured call is captured into a HIP graph after a warm-up; one graph holds the call once per input buffer, and the
buffers of a shape are as many as it takes to move 600 MiB through a replay (at least two, at most eight), so no call finds
its input resident.  The graphs of a shape are replayed in turn between HIP events, ``--iters`` replays in each of
``--rounds`` alternating rounds; reported are the median over all replays (60 by default), per call, the medians of the
single rounds, and their spread (largest minus smallest round median).  One JSON line per shape is appended to --out.

    python scripts/long_gated_bench.py [--iters 20] [--rounds 3] [--out profiles/long_gated.jsonl] [--only SUBSTRING]
                                       [--baseline [--root PARENT_CHECKOUT]]"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
# (name, batch, cin, cout, groups, L = K, dtype)
SHAPES = [
    ("depthwise B4 C256 L65536 f32", 4, 256, 256, 256, 65536, F32),
    ("depthwise B4 C256 L65536 bf16", 4, 256, 256, 256, 65536, BF16),
    ("depthwise B4 C256 L262144 f32", 4, 256, 256, 256, 262144, F32),
    ("depthwise B8 C768 L8192 bf16", 8, 768, 768, 768, 8192, BF16),
    ("dense B4 8->8 L32768 f32", 4, 8, 8, 1, 32768, F32),
]
ROTATE_BYTES = 600 << 20


def capture(step):
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    g.replay()
    torch.cuda.synchronize()
    return g


def timed(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def added_peak(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def run_shape(fca, name, B, ci, co, g, L, dtype, iters, rounds, baseline):
    torch.manual_seed(0)
    K = L
    es = torch.empty(0, dtype=dtype).element_size()
    nbuf = max(2, min(8, -(-ROTATE_BYTES // (B * (2 * ci + 2 * co) * L * es))))
    act = lambda channels: torch.randn(B, channels, L, device=DEV).to(dtype)      # noqa: E731
    xs, ps = [act(ci) for _ in range(nbuf)], [act(ci) for _ in range(nbuf)]
    qs, gys = [act(co) for _ in range(nbuf)], [act(co) for _ in range(nbuf)]
    layer = fca.FFTLongConv1d(ci, co, K, groups=g, bias=True, causal=True).to(DEV)
    with torch.no_grad():
        layer.weight.mul_(1.0 / (ci // g * K) ** 0.5 / layer.weight.std())
    layer = layer.to(dtype)
    # the forward is timed on a copy in eval() mode, which keeps its cached spectrum for good: a module in training mode
    # drops its cache in every step with gradients, and a captured forward would go on reading the freed buffer
    infer = copy.deepcopy(layer).eval()
    row = {"shape": name, "dtype": str(dtype).replace("torch.", ""), "B": B, "cin": ci, "cout": co, "groups": g, "L": L,
           "K": K, "causal": True, "buffers": nbuf, "device": torch.cuda.get_device_name(0), "iters": iters,
           "rounds": rounds, "mode": "baseline" if baseline else "gated"}

    fused = lambda m, x, p, q: m(x, p, q)               # noqa: E731
    line = lambda m, x, p, q: q * m(p * x)              # noqa: E731
    variants = {"c_parent": line} if baseline else {"a_fused": fused, "b_composed": line}
    leaves = [[t.detach().requires_grad_() for t in (x, p, q)] for x, p, q in zip(xs, ps, qs)]
    params = (layer.weight, layer.bias)
    steps = {}
    for key, op in variants.items():
        def fwd(op=op):
            with torch.no_grad():
                return [op(infer, x, p, q) for x, p, q in zip(xs, ps, qs)]

        def step(op=op):
            return [torch.autograd.grad(op(layer, *l), tuple(l) + params, gy) for l, gy in zip(leaves, gys)]
        steps[key + "_fwd"], steps[key + "_step"] = fwd, step

        def one_fwd(op=op):
            with torch.no_grad():
                return op(infer, xs[0], ps[0], qs[0])
        row[key + "_fwd_peak_bytes"] = added_peak(one_fwd)
        row[key + "_step_peak_bytes"] = added_peak(lambda op=op: torch.autograd.grad(op(layer, *leaves[0]), tuple(leaves[0]) + params, gys[0]))
    if not baseline:
        ya, yb = steps["a_fused_fwd"]()[0].float(), steps["b_composed_fwd"]()[0].float()
        row["a_vs_b_y_max_rel"] = float((ya - yb).abs().max() / yb.abs().max())
        del ya, yb
    graphs = {}
    for key, fn in steps.items():
        try:
            graphs[key] = capture(fn)
        except Exception as exc:       # (a step that cannot run or be captured is reported, the others are still timed)
            row[key + "_us"] = None
            row[key + "_note"] = f"not captured: {str(exc)[:160]}"
            torch.cuda.synchronize()
    per_round = {key: [] for key in graphs}
    samples = {key: [] for key in graphs}
    for _ in range(rounds):
        this = {key: [] for key in graphs}
        for _ in range(iters):
            for key, gr in graphs.items():          # in turn
                this[key].append(timed(gr) / nbuf)
        for key, vals in this.items():
            per_round[key].append(round(statistics.median(vals), 1))
            samples[key] += vals
    for key, vals in samples.items():
        row[key + "_us"] = round(statistics.median(vals), 1)
        row[key + "_rounds_us"] = per_round[key]
        row[key + "_spread_us"] = round(max(per_round[key]) - min(per_round[key]), 1)
        row[key + "_n"] = len(vals)
    for what in ("fwd", "step"):
        if row.get(f"a_fused_{what}_us") and row.get(f"b_composed_{what}_us"):
            row[f"a_over_b_{what}"] = round(row[f"a_fused_{what}_us"] / row[f"b_composed_{what}_us"], 3)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "long_gated.jsonl"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose fft_conv_pytorch_amd package is timed (default: this tree)")
    ap.add_argument("--tag", default=None, help="free text recorded with every row")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import fft_conv_pytorch_amd as fca
    assert os.path.abspath(fca.__file__).startswith(os.path.abspath(a.root)), fca.__file__
    for name, B, ci, co, g, L, dtype in SHAPES:
        if a.only and a.only not in name:
            continue
        res = run_shape(fca, name, B, ci, co, g, L, dtype, a.iters, a.rounds, a.baseline)
        if a.tag:
            res["tag"] = a.tag
        line = json.dumps(res)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()
