#!/usr/bin/env python3
"""The weight-gradient plan of the long-filter path ("Weight gradient: x and dY where they lie"): the
training step of ``FFTLongConv1d`` and its weight gradient alone, with dW from the plan against the exchanged route on the
same tree and on the parent commit:

  a_wgrad      FFTCONV_LONG_WGRAD=1
  b_unset      the variable unset, on the same tree
  c_parent     ``--baseline --root PARENT_CHECKOUT``: the same public calls with the package imported from a checkout of the
               parent commit (``FFTCONV_LIB`` may name its library), in a process of its own.

Per shape two things are measured: ``step``, forward + dX + dW of a causal ``FFTLongConv1d`` without bias (the module keeps
its kernel spectrum while the weight is unchanged), and ``dw``, the backward of that layer (``FFTLongConvFunction.backward``
on the tensors the forward saves) asked for the weight gradient alone, together with ``torch.cuda.max_memory_allocated`` of one such backward above what
was allocated before it.  Channels-last shapes pass the signal as the transpose of a contiguous (B, L, C) tensor and ask
for a channels-last result, so dY lies that way too.

Every measured call is captured into a HIP graph after a warm-up; one graph holds the call once per input buffer, and the
buffers of a shape are as many as it takes to move 600 MiB through a replay (at least two, at most eight), so no call finds
its input resident.  The graphs of a shape are replayed in turn between HIP events, ``--iters`` replays in each of
``--rounds`` alternating rounds; reported are the median over all replays (60 by default), per call, the medians of the
single rounds, and their spread (largest minus smallest round median).  One JSON line per shape is appended to --out.

    python scripts/long_wgrad_bench.py [--iters 20] [--rounds 3] [--out profiles/long_wgrad.jsonl] [--only SUBSTRING]
                                       [--baseline [--root PARENT_CHECKOUT]]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import types

import torch

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
# (name, batch, cin, cout, groups, L = K, dtype, channels-last activations)
SHAPES = [
    ("depthwise B4 C256 L65536 f32", 4, 256, 256, 256, 65536, F32, False),
    ("depthwise B4 C256 L65536 bf16", 4, 256, 256, 256, 65536, BF16, False),
    ("depthwise B4 C256 L65536 f32 nlc", 4, 256, 256, 256, 65536, F32, True),
    ("depthwise B4 C256 L65536 bf16 nlc", 4, 256, 256, 256, 65536, BF16, True),
    ("depthwise B4 C256 L262144 f32", 4, 256, 256, 256, 262144, F32, False),
    ("depthwise B8 C768 L8192 bf16", 8, 768, 768, 768, 8192, BF16, False),
    ("dense B4 8->8 L32768 f32", 4, 8, 8, 1, 32768, F32, False),
    ("dense B4 64->64 L8192 f32", 4, 64, 64, 1, 8192, F32, False),
]
ROTATE_BYTES = 600 << 20
KNOB = "FFTCONV_LONG_WGRAD"


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


def run_shape(fca, name, B, ci, co, g, L, dtype, nlc, iters, rounds, baseline):
    torch.manual_seed(0)
    K = L
    es = torch.empty(0, dtype=dtype).element_size()
    nbuf = max(2, min(8, -(-ROTATE_BYTES // (B * (ci + co) * L * es))))

    def activation(channels):
        if nlc:
            return torch.randn(B, L, channels, device=DEV).to(dtype).transpose(1, 2)
        return torch.randn(B, channels, L, device=DEV).to(dtype)

    xs = [activation(ci) for _ in range(nbuf)]
    gys = [activation(co) for _ in range(nbuf)]
    layer = fca.FFTLongConv1d(ci, co, K, groups=g, bias=False, causal=True, channels_last=nlc).to(DEV)
    with torch.no_grad():
        layer.weight.mul_(1.0 / (ci // g * K) ** 0.5 / layer.weight.std())
    layer = layer.to(dtype)
    row = {"shape": name, "dtype": str(dtype).replace("torch.", ""), "B": B, "cin": ci, "cout": co, "groups": g, "L": L,
           "K": K, "causal": True, "channels_last": nlc, "buffers": nbuf, "device": torch.cuda.get_device_name(0),
           "iters": iters, "rounds": rounds, "mode": "baseline" if baseline else "wgrad"}

    def knob(value, fn):
        def step():
            if value is None:
                os.environ.pop(KNOB, None)
            else:
                os.environ[KNOB] = value
            return fn()
        return step

    xg = [x.detach().requires_grad_() for x in xs]

    def train_step():
        return [torch.autograd.grad(layer(x), (x, layer.weight), gy) for x, gy in zip(xg, gys)]

    # the weight gradient alone: the backward of record (``FFTLongConvFunction.backward``) asked for dW only, on the tensors
    # the forward saves and the configuration it records for this layer
    backward = importlib.import_module(fca.__name__ + ".autograd").FFTLongConvFunction.backward

    def dw_of(x, gy):
        ctx = types.SimpleNamespace(saved_tensors=(x, layer.weight.detach()), decim=False, needs_input_grad=(False, True, False),
                                    cfg=(K - 1, 0, True, g, False, 1, 1, "constant"))
        with torch.no_grad():
            return backward(ctx, gy)[1]

    variants = {"c_parent": None} if baseline else {"a_wgrad": "1", "b_unset": None}
    steps = {}
    for key, value in variants.items():
        steps[key + "_step"] = knob(value, train_step)
        steps[key + "_dw"] = knob(value, lambda: [dw_of(x, gy) for x, gy in zip(xs, gys)])
        one = knob(value, lambda: dw_of(xs[0], gys[0]))
        one()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        one()
        torch.cuda.synchronize()
        row[key + "_dw_peak_bytes"] = torch.cuda.max_memory_allocated() - before
    if not baseline:
        da, db = steps["a_wgrad_dw"]()[0].float(), steps["b_unset_dw"]()[0].float()
        row["a_vs_b_dW_max_rel"] = float((da - db).abs().max() / db.abs().max())
        del da, db
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
    for what in ("step", "dw"):
        if row.get(f"a_wgrad_{what}_us") and row.get(f"b_unset_{what}_us"):
            row[f"a_over_b_{what}"] = round(row[f"a_wgrad_{what}_us"] / row[f"b_unset_{what}_us"], 3)
    os.environ.pop(KNOB, None)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "long_wgrad.jsonl"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose fft_conv_pytorch_amd package is timed (default: this tree)")
    ap.add_argument("--tag", default=None, help="free text recorded with every row")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import fft_conv_pytorch_amd as fca
    assert os.path.abspath(fca.__file__).startswith(os.path.abspath(a.root)), fca.__file__
    for name, B, ci, co, g, L, dtype, nlc in SHAPES:
        if a.only and a.only not in name:
            continue
        res = run_shape(fca, name, B, ci, co, g, L, dtype, nlc, a.iters, a.rounds, a.baseline)
        if a.tag:
            res["tag"] = a.tag
        line = json.dumps(res)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()
