#!/usr/bin/env python3
"""Channels-last tensors in the 2-D / 3-D path: the forward of ``FFTConv2d`` / ``FFTConv3d`` in eval mode
(cached kernel spectrum) and a training step (forward + dX + dW) whose dY lies channels-last, per shape in these variants:

  a    channels-last signal, ``channels_last=True``               (this tree)
  a0   channels-last signal, keyword off: a call that exists on the parent too
  a1   a0 under FFTCONV_ND_CL=1: the call without the keyword reads its signal and dY where they lie
  b    variant a under FFTCONV_ND_CL=0: torch copies everywhere   (this tree)
  d    contiguous signal, contiguous dY, keyword off              (either tree: the control between the two processes)
  c    ``--baseline --root PARENT_CHECKOUT``: a's call on the parent commit, i.e. the plain module on the channels-last
       signal plus ``.contiguous(memory_format=...)`` on the result
  c0   the parent commit running a0's call

Every measured call is captured into a HIP graph after a warm-up; one graph holds the call once per input buffer, and the
buffers of a shape are as many as it takes to move 600 MiB through a replay (at least two, at most eight), so no call finds
its input resident.  The graphs of a shape are replayed in turn between HIP events, ``--iters`` replays in each of
``--rounds`` alternating rounds; reported are the median over all replays (60 by default), per call, the medians of the
single rounds, and their spread (largest minus smallest round median).  One JSON line per shape is appended to --out.

    python scripts/nd_channels_last_bench.py [--iters 20] [--rounds 3] [--out profiles/nd_channels_last.jsonl]
                                             [--only SUBSTRING] [--baseline [--root PARENT_CHECKOUT]] [--tag TEXT]"""
import argparse
import json
import os
import statistics
import sys

import torch

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
# (name, batch, cin, cout, groups, spatial, kernel, padding, dtype)
SHAPES = [
    ("cfgB B16 8->8 512^2 k31 f32", 16, 8, 8, 1, (512, 512), 31, 0, F32),
    ("depthwise B8 C256 56^2 k31 same f32", 8, 256, 256, 256, (56, 56), 31, 15, F32),
    ("depthwise B8 C256 56^2 k31 same bf16", 8, 256, 256, 256, (56, 56), 31, 15, BF16),
    ("depthwise B8 C512 28^2 k27 same bf16", 8, 512, 512, 512, (28, 28), 27, 13, BF16),
    ("dense B4 64->64 128^2 k15 same f32", 4, 64, 64, 1, (128, 128), 15, 7, F32),
    ("3-D B4 4->4 64^3 k9 f32", 4, 4, 4, 1, (64, 64, 64), 9, 0, F32),
]
ROTATE_BYTES = 600 << 20
KNOB = "FFTCONV_ND_CL"


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


def run_shape(fca, name, B, ci, co, g, sp, k, pad, dtype, iters, rounds, baseline):
    torch.manual_seed(0)
    n = len(sp)
    fmt = torch.channels_last if n == 2 else torch.channels_last_3d
    cls = fca.FFTConv2d if n == 2 else fca.FFTConv3d
    es = torch.empty(0, dtype=dtype).element_size()
    out_sp = tuple(s + 2 * pad - k + 1 for s in sp)
    numel = B * (ci * torch.Size(sp).numel() + co * torch.Size(out_sp).numel())
    nbuf = max(2, min(8, -(-ROTATE_BYTES // (numel * es))))
    xs = [torch.randn((B, ci) + sp, device=DEV).to(dtype) for _ in range(nbuf)]
    gys = [torch.randn((B, co) + out_sp, device=DEV).to(dtype) for _ in range(nbuf)]
    xs_cl = [x.contiguous(memory_format=fmt) for x in xs]
    gys_cl = [gy.contiguous(memory_format=fmt) for gy in gys]

    def module(**kw):
        layer = cls(ci, co, k, padding=pad, groups=g, bias=True, **kw).to(DEV)
        with torch.no_grad():
            layer.weight.mul_(1.0 / (ci // g * k ** n) ** 0.5 / layer.weight.std())
        return layer.to(dtype)

    # One module per captured mode, never switched afterwards: an eval-mode graph reads the module's cached kernel spectrum
    # by address, and a later train() on the same module would drop that cache (torch.cuda.graph empties the allocator's
    # cache when the next capture begins, which unmaps the block under the graph).
    plain = {mode: module() for mode in ("eval", "train")}
    cl_out = None if baseline else {mode: module(channels_last=True) for mode in ("eval", "train")}
    for mode in ("eval", "train"):
        plain[mode].load_state_dict(plain["eval"].state_dict())
        plain[mode].train(mode == "train")
        if cl_out is not None:
            cl_out[mode].load_state_dict(plain["eval"].state_dict())
            cl_out[mode].train(mode == "train")
    row = {"shape": name, "dtype": str(dtype).replace("torch.", ""), "B": B, "cin": ci, "cout": co, "groups": g,
           "spatial": list(sp), "k": k, "padding": pad, "buffers": nbuf, "device": torch.cuda.get_device_name(0),
           "iters": iters, "rounds": rounds, "mode": "baseline" if baseline else "branch"}
    probe = fca.functional._plan_for(xs[0], plain["eval"].weight, plain["eval"].bias, 1, pad, 1, g, "constant")
    row["route"] = {key: probe.route[key] for key in ("T", "Tx", "nxt", "planes")}

    def knob(value, fn):
        def step():
            if value is None:
                os.environ.pop(KNOB, None)
            else:
                os.environ[KNOB] = value
            return fn()
        return step

    def forward(layers, inputs, to_cl=False):
        layer = layers["eval"]

        def run():
            with torch.no_grad():
                ys = [layer(x) for x in inputs]
                return [y.contiguous(memory_format=fmt) for y in ys] if to_cl else ys
        return run

    def train(layers, inputs, grads, to_cl=False):
        layer = layers["train"]
        leaves = [x.detach().requires_grad_() for x in inputs]

        def run():
            out = []
            for x, gy in zip(leaves, grads):
                y = layer(x)
                if to_cl:
                    y = y.contiguous(memory_format=fmt)
                out.append(torch.autograd.grad(y, (x, layer.weight), gy))
            return out
        return run

    steps = {}
    if baseline:
        steps["c_fwd"], steps["c_step"] = forward(plain, xs_cl, True), train(plain, xs_cl, gys_cl, True)
        steps["c0_fwd"], steps["c0_step"] = forward(plain, xs_cl), train(plain, xs_cl, gys_cl)
        steps["d_fwd"], steps["d_step"] = forward(plain, xs), train(plain, xs, gys)
    else:
        steps["a_fwd"], steps["a_step"] = knob(None, forward(cl_out, xs_cl)), knob(None, train(cl_out, xs_cl, gys_cl))
        steps["a0_fwd"], steps["a0_step"] = knob(None, forward(plain, xs_cl)), knob(None, train(plain, xs_cl, gys_cl))
        steps["a1_fwd"], steps["a1_step"] = knob("1", forward(plain, xs_cl)), knob("1", train(plain, xs_cl, gys_cl))
        steps["b_fwd"], steps["b_step"] = knob("0", forward(cl_out, xs_cl)), knob("0", train(cl_out, xs_cl, gys_cl))
        steps["d_fwd"], steps["d_step"] = knob(None, forward(plain, xs)), knob(None, train(plain, xs, gys))
        ya, yb, yd = steps["a_fwd"]()[0], steps["b_fwd"]()[0], steps["d_fwd"]()[0]
        row["a_equals_b_equals_d"] = bool(torch.equal(ya, yb) and torch.equal(ya, yd))
        row["a_strides_channels_last"] = bool(ya.is_contiguous(memory_format=fmt))
        del ya, yb, yd
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
    os.environ.pop(KNOB, None)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "nd_channels_last.jsonl"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose fft_conv_pytorch_amd package is timed (default: this tree)")
    ap.add_argument("--tag", default=None, help="free text recorded with every row")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import fft_conv_pytorch_amd as fca
    assert os.path.abspath(fca.__file__).startswith(os.path.abspath(a.root)), fca.__file__
    for name, B, ci, co, g, sp, k, pad, dtype in SHAPES:
        if a.only and a.only not in name:
            continue
        res = run_shape(fca, name, B, ci, co, g, sp, k, pad, dtype, a.iters, a.rounds, a.baseline)
        if a.tag:
            res["tag"] = a.tag
        line = json.dumps(res)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()
