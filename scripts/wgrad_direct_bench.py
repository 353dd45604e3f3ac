#!/usr/bin/env python3
"""The direct small-kernel weight gradient (``fc_wgrad_direct``): the weight gradient alone and the
training step of ``FFTConv2d`` / ``FFTConv3d`` layers with a few taps and 'same' padding,

  a_direct     FFTCONV_WGRAD_DIRECT=1
  b_unset      the variable unset, on the same tree
  c_parent     ``--baseline --root PARENT_CHECKOUT``: the same calls with the package imported from a checkout of the
               parent commit, in a process of its own.

Per shape two things are measured: ``dw``, ``autograd._grad_weight`` on x and dY (the call both backward functions make),
with ``torch.cuda.max_memory_allocated`` of one such call above what was allocated before it, and ``step``, forward + dX +
dW of the layer without bias.  For a shape the direct route covers the row also gives the read-once byte roofline, (bytes
of x + bytes of dY) / 8 TB/s, and the fraction of it that a_direct_dw reaches.

Every measured call is captured into a HIP graph after a warm-up; one graph holds the call once per input buffer, and the
buffers of a shape are as many as it takes to move 600 MiB through a replay (at least two, at most eight).  The graphs of
a shape are replayed in turn between HIP events, ``--iters`` replays in each of ``--rounds`` alternating rounds; reported
are the median over all replays (60 by default), per call, the medians of the single rounds and their spread (largest
minus smallest round median).  One JSON line per shape is appended to --out.

``--depthwise`` times the depthwise rows of DESIGN.md 4.5c instead (layers with one input channel per group, and the
sweep of the channel multiplier that the planner's rule was set by): the weight gradient alone, with two more columns

  a_mfma       FFTCONV_WGRAD_DIRECT=1 FFTCONV_WGRAD_DIRECT_BODY=mfma: the MFMA body, which must reproduce c_parent,
  a_valu       FFTCONV_WGRAD_DIRECT=1 FFTCONV_WGRAD_DIRECT_BODY=valu: the depthwise body at any channel multiplier,

and per row the kernel body that a_direct ran (``a_body``).

``--h16`` times the 16-bit MFMA body of DESIGN.md 4.5g on the bfloat16 forms of the dense shapes and one float16 shape,
weight gradient and step (the step with FFTCONV_DIRECT=1 FFTCONV_DIRECT_BODY=h16 besides, in every column), with

  a_h16        FFTCONV_WGRAD_DIRECT=1 FFTCONV_WGRAD_DIRECT_BODY=h16,
  a_direct     FFTCONV_WGRAD_DIRECT=1 alone (the float32 MFMA body); c_parent (``--baseline``) is this setting on the parent.

    python scripts/wgrad_direct_bench.py [--iters 20] [--rounds 3] [--out profiles/wgrad_direct.jsonl] [--only SUBSTRING]
                                         [--depthwise | --h16] [--baseline [--root PARENT_CHECKOUT]]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
# (name, batch, cin, cout, groups, spatial, kernel, stride, dtype); padding is kernel // 2 on every axis
SHAPES = [
    ("3-D B8 8->8 64^3 k3", 8, 8, 8, 1, (64, 64, 64), 3, 1, F32),
    ("3-D B2 8->8 128^3 k5", 2, 8, 8, 1, (128, 128, 128), 5, 1, F32),
    ("3-D B8 8->8 64^3 k9 (refused: 729 taps)", 8, 8, 8, 1, (64, 64, 64), 9, 1, F32),
    ("2-D B16 8->8 512^2 k3", 16, 8, 8, 1, (512, 512), 3, 1, F32),
    ("2-D dense B4 64->64 128^2 k3", 4, 64, 64, 1, (128, 128), 3, 1, F32),
    ("2-D depthwise B8 C256 56^2 k7 bf16", 8, 256, 256, 256, (56, 56), 7, 1, BF16),
    ("2-D B16 8->16 256^2 k3 stride 2", 16, 8, 16, 1, (256, 256), 3, 2, F32),
]
# --depthwise: Cin/groups == 1; the last four rows are the first with a channel multiplier Cout/groups of 2, 4, 8, 16
DW_SHAPES = [
    ("2-D depthwise B8 C256 56^2 k7 bf16", 8, 256, 256, 256, (56, 56), 7, 1, BF16),
    ("2-D depthwise B8 C256 56^2 k7 f32", 8, 256, 256, 256, (56, 56), 7, 1, F32),
    ("2-D depthwise B8 C512 28^2 k3 bf16", 8, 512, 512, 512, (28, 28), 3, 1, BF16),
    ("2-D depthwise B8 C96 112^2 k7 bf16", 8, 96, 96, 96, (112, 112), 7, 1, BF16),
    ("2-D depthwise B8 C256 56^2 k5 stride 2 bf16", 8, 256, 256, 256, (56, 56), 5, 2, BF16),
    ("3-D depthwise B4 C64 32^3 k3 bf16", 4, 64, 64, 64, (32, 32, 32), 3, 1, BF16),
] + [(f"2-D B8 C256 x{m} 56^2 k7 bf16", 8, 256, 256 * m, 256, (56, 56), 7, 1, BF16) for m in (2, 4, 8, 16)]
F16 = torch.float16
# --h16: the dense rows of SHAPES in bfloat16, and one in float16
H16_SHAPES = [(f"{name} bf16", B, ci, co, g, size, k, s, BF16) for name, B, ci, co, g, size, k, s, _ in SHAPES
              if g == 1 and k < 9] + [("3-D B8 8->8 64^3 k3 f16", 8, 8, 8, 1, (64, 64, 64), 3, 1, F16)]
ROTATE_BYTES = 600 << 20
HBM_BYTES_PER_US = 8e6      # 8 TB/s
KNOB = "FFTCONV_WGRAD_DIRECT"
BODY_KNOB = "FFTCONV_WGRAD_DIRECT_BODY"


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


def run_shape(fca, name, B, ci, co, g, size, k, s, dtype, iters, rounds, baseline, depthwise=False, h16=False):
    torch.manual_seed(0)
    nd = len(size)
    auto = importlib.import_module(fca.__name__ + ".autograd")
    es = torch.empty(0, dtype=dtype).element_size()
    out = tuple((n + 2 * (k // 2) - k) // s + 1 for n in size)
    x_bytes = B * ci * torch.Size(size).numel() * es
    dy_bytes = B * co * torch.Size(out).numel() * es
    nbuf = max(2, min(8, -(-ROTATE_BYTES // (x_bytes + dy_bytes))))
    xs = [torch.randn((B, ci) + size, device=DEV).to(dtype) for _ in range(nbuf)]
    gys = [torch.randn((B, co) + out, device=DEV).to(dtype) for _ in range(nbuf)]
    layer = (fca.FFTConv2d if nd == 2 else fca.FFTConv3d)(ci, co, k, stride=s, padding=k // 2, groups=g, bias=False).to(DEV).to(dtype)
    wshape = tuple(layer.weight.shape)
    conf = ((s,) * nd, (k // 2,) * nd, (1,) * nd, g, "constant")
    row = {"shape": name, "dtype": str(dtype).replace("torch.", ""), "B": B, "cin": ci, "cout": co, "groups": g,
           "size": list(size), "k": k, "stride": s, "buffers": nbuf, "device": torch.cuda.get_device_name(0), "iters": iters,
           "rounds": rounds, "mode": "baseline" if baseline else "direct", "roofline_us": round((x_bytes + dy_bytes) / HBM_BYTES_PER_US, 1)}

    def knob(value, fn):
        def step():
            for name, v in ((KNOB, value and value[0]), (BODY_KNOB, value and value[1:] or None)):
                if v is None:
                    os.environ.pop(name, None)
                else:
                    os.environ[name] = v
            return fn()
        return step

    xg = [x.detach().requires_grad_() for x in xs]

    def train_step():
        return [torch.autograd.grad(layer(x), (x, layer.weight), gy) for x, gy in zip(xg, gys)]

    def dw_of(x, gy):
        with torch.no_grad():
            return auto._grad_weight(x, gy, wshape, *conf)

    # (a variant's value: the switch, then the body knob)
    variants = {"c_parent": None} if baseline else {"a_direct": "1", "b_unset": None}
    if depthwise:
        variants = {"c_parent": "1"} if baseline else {**variants, "a_mfma": "1mfma", "a_valu": "1valu"}
    if h16:
        variants = {"c_parent": "1"} if baseline else {"a_h16": "1h16", **variants}
    steps = {}
    for key, value in variants.items():
        if not depthwise:
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
        if hasattr(auto, "dw_route"):
            row[key + "_route"] = knob(value, lambda: auto.dw_route(xs[0], wshape, *conf))()
    if depthwise and hasattr(auto, "dw_direct_body"):
        row["a_body"] = knob("1", lambda: auto.dw_direct_body(xs[0], wshape, *conf))()
    if h16 and not baseline:
        row["a_h16_body"] = knob("1h16", lambda: auto.dw_direct_body(xs[0], wshape, *conf))()
        dh, da = steps["a_h16_dw"]()[0].float(), steps["a_direct_dw"]()[0].float()
        row["h16_vs_direct_dW_max_rel"] = float((dh - da).abs().max() / da.abs().max())
        del dh, da
    if not baseline:
        da, db = steps["a_direct_dw"]()[0].float(), steps["b_unset_dw"]()[0].float()
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
        if row.get(f"a_direct_{what}_us") and row.get(f"b_unset_{what}_us"):
            row[f"b_over_a_{what}"] = round(row[f"b_unset_{what}_us"] / row[f"a_direct_{what}_us"], 2)
        if row.get(f"a_h16_{what}_us") and row.get(f"a_direct_{what}_us"):
            row[f"direct_over_h16_{what}"] = round(row[f"a_direct_{what}_us"] / row[f"a_h16_{what}_us"], 2)
    if row.get("a_direct_route") == "direct" and row.get("a_direct_dw_us"):
        row["a_roofline_fraction"] = round(row["roofline_us"] / row["a_direct_dw_us"], 3)
    os.environ.pop(KNOB, None)
    os.environ.pop(BODY_KNOB, None)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="default: profiles/wgrad_direct.jsonl, with --depthwise profiles/wgrad_direct_dw.jsonl")
    ap.add_argument("--depthwise", action="store_true", help="the depthwise rows and the multiplier sweep, dW alone")
    ap.add_argument("--h16", action="store_true", help="the 16-bit MFMA body on the 16-bit forms of the dense rows")
    ap.add_argument("--only", default=None)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose fft_conv_pytorch_amd package is timed (default: this tree)")
    ap.add_argument("--tag", default=None, help="free text recorded with every row")
    a = ap.parse_args()
    a.out = a.out or os.path.join("profiles", "wgrad_direct_h16.jsonl" if a.h16 else "wgrad_direct_dw.jsonl" if a.depthwise else "wgrad_direct.jsonl")
    if a.h16:      # (the forward and dX of every step on the 16-bit MFMAs too; the weight gradient alone reads neither)
        os.environ.update(FFTCONV_DIRECT="1", FFTCONV_DIRECT_BODY="h16")
    sys.path.insert(0, os.path.abspath(a.root))
    import fft_conv_pytorch_amd as fca
    assert os.path.abspath(fca.__file__).startswith(os.path.abspath(a.root)), fca.__file__
    for name, B, ci, co, g, size, k, s, dtype in (H16_SHAPES if a.h16 else DW_SHAPES if a.depthwise else SHAPES):
        if a.only and a.only not in name:
            continue
        res = run_shape(fca, name, B, ci, co, g, size, k, s, dtype, a.iters, a.rounds, a.baseline, a.depthwise, a.h16)
        if a.tag:
            res["tag"] = a.tag
        line = json.dumps(res)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()
