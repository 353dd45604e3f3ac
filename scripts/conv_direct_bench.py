#!/usr/bin/env python3
"""The direct small-kernel forward and input gradient: ``fc_conv_direct_dw`` on depthwise layers (the
default) or, with ``--dense``, ``fc_conv_direct`` on the shape list of DESIGN.md 4.5d.  Per shape, 'same' padding, no bias:

  fwd    the no-grad forward of an ``FFTConv2d`` / ``FFTConv3d`` module of its own in ``eval()`` (a training step drops
         the kernel spectrum that a module caches, and a captured no-grad forward would go on reading it),
  dx     ``autograd._grad_input`` on dY (the call the backward function makes),
  step   forward + dX + dW of a second module under FFTCONV_WGRAD_DIRECT=1,

each as  a_set  the route's switch (FFTCONV_DIRECT_DW, ``--dense``: FFTCONV_DIRECT) set to 1,  b_unset  unset on the same
tree,  d_torch  ``torch.nn.functional.conv2d/3d`` and its autograd.  ``--baseline --root PARENT_CHECKOUT`` times the
b_unset calls on the package of another checkout (the parent commit: c_parent) in a process of its own.  ``--h16`` times ``fc_conv_direct_h16`` on the first five dense shapes in bfloat16 and the
64 -> 64 shape in float16 too, fwd and dx only:  a_set  FFTCONV_DIRECT=1 FFTCONV_DIRECT_BODY=h16,  a1_f32body  FFTCONV_DIRECT=1
alone (the float32 MFMA body on the same tensors),  b_unset  and  d_torch.  The row also
gives the read-once byte roofline of forward and dX, (bytes of x + bytes of y) / 8 TB/s, and the fraction a_set reaches.

``--tr`` times ``fc_conv_direct_tr`` (FFTCONV_DIRECT_TR): the dX of the strided dense shape in float32 and
bfloat16 and the forward of ``fft_conv_transpose`` on four up-convolutions, ``d_torch`` being ``conv_transpose2d/3d``.

``--tr-h16`` times ``fc_conv_direct_tr_h16`` on the five shapes of ``--tr`` in bfloat16 and the k4 s2 p1
up-convolution in float16 too:  a_set  FFTCONV_DIRECT_TR=1 FFTCONV_DIRECT_BODY=h16,  a1_f32body  FFTCONV_DIRECT_TR=1 alone
(``fc_conv_direct_tr`` on the same tensors),  b_unset  and  d_torch.

The method is that of scripts/wgrad_direct_bench.py (its ``capture`` and ``timed``): every call is captured into a HIP
graph over rotating buffers that move 600 MiB through a replay, the graphs of a shape are replayed in turn, ``--iters``
replays in each of ``--rounds`` alternating rounds; reported are the median over all replays per call, the medians of the
rounds and their spread.  One JSON line per shape is appended to --out.

    python scripts/conv_direct_bench.py [--dense | --h16 | --tr | --tr-h16] [--iters 20] [--rounds 3] [--out FILE] [--only SUBSTRING]
                                        [--baseline [--root PARENT_CHECKOUT]]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wgrad_direct_bench import DEV, DW_SHAPES, F32, HBM_BYTES_PER_US, ROTATE_BYTES, capture, timed  # noqa: E402

# (name, batch, cin, cout, groups, spatial, kernel, stride, dtype); padding is kernel // 2 on every axis
DW = [s for s in DW_SHAPES if "x16" not in s[0]]      # (multiplier 16 is fc_conv_direct's)
DENSE = [
    ("3-D B8 8->8 64^3 k3", 8, 8, 8, 1, (64, 64, 64), 3, 1, F32),
    ("3-D B2 8->8 128^3 k5", 2, 8, 8, 1, (128, 128, 128), 5, 1, F32),
    ("2-D B16 8->8 512^2 k3", 16, 8, 8, 1, (512, 512), 3, 1, F32),
    ("2-D dense B4 64->64 128^2 k3", 4, 64, 64, 1, (128, 128), 3, 1, F32),
    ("2-D B16 8->16 256^2 k3 stride 2", 16, 8, 16, 1, (256, 256), 3, 2, F32),
    ("2-D B16 8->8 512^2 k31 (refused)", 16, 8, 8, 1, (512, 512), 31, 1, F32),
    ("2-D B1 16->16 16x8192 k3", 1, 16, 16, 1, (16, 8192), 3, 1, F32),
]
H16 = [s[:-1] + (torch.bfloat16,) for s in DENSE[:5]] + [DENSE[3][:-1] + (torch.float16,)]
KNOBS = ("FFTCONV_DIRECT", "FFTCONV_DIRECT_DW", "FFTCONV_DIRECT_BODY", "FFTCONV_WGRAD_DIRECT", "FFTCONV_DIRECT_TR")
# (name, what, batch, cin, cout, spatial of x, kernel, stride, padding, output padding, dtype); "dx": x is the layer's input,
# the timed call its input gradient; "fwd": x is the signal of fft_conv_transpose
TR = [
    ("dX of 2-D B16 8->16 256^2 k3 stride 2", "dx", 16, 8, 16, (256, 256), 3, 2, 1, 0, F32),
    ("dX of 2-D B16 8->16 256^2 k3 stride 2", "dx", 16, 8, 16, (256, 256), 3, 2, 1, 0, torch.bfloat16),
    ("convT 2-D B8 64->32 64^2 k4 s2 p1", "fwd", 8, 64, 32, (64, 64), 4, 2, 1, 0, F32),
    ("convT 2-D B8 64->32 64^2 k2 s2", "fwd", 8, 64, 32, (64, 64), 2, 2, 0, 0, F32),
    ("convT 2-D B8 32->16 128^2 k3 s2 p1 op1", "fwd", 8, 32, 16, (128, 128), 3, 2, 1, 1, F32),
    ("convT 3-D B2 32->16 32^3 k2 s2", "fwd", 2, 32, 16, (32, 32, 32), 2, 2, 0, 0, F32),
]
TR_H16 = [s[:-1] + (torch.bfloat16,) for s in TR[1:]] + [TR[2][:-1] + (torch.float16,)]


def run_tr_shape(fca, name, what, B, ci, co, size, k, s, p, op, dtype, iters, rounds, h16=False):
    """One row of --tr: a_set (FFTCONV_DIRECT_TR=1), b_unset and d_torch of one call, timed as run_shape times its calls.
    ``h16`` (--tr-h16): a_set has FFTCONV_DIRECT_BODY=h16 too, a1_f32body is FFTCONV_DIRECT_TR=1 alone."""
    torch.manual_seed(0)
    nd = len(size)
    auto = importlib.import_module(fca.__name__ + ".autograd")
    fun = importlib.import_module(fca.__name__ + ".functional")
    es = torch.empty(0, dtype=dtype).element_size()
    if what == "dx":      # the transposed convolution runs from dY (B, co, out) to dX (B, ci, size)
        out = tuple((n + 2 * p - k) // s + 1 for n in size)
        src, dst, wshape = (B, co) + out, (B, ci) + size, (co, ci) + (k,) * nd
    else:
        out = tuple((n - 1) * s - 2 * p + k + op for n in size)
        src, dst, wshape = (B, ci) + size, (B, co) + out, (ci, co) + (k,) * nd
    io_bytes = (torch.Size(src).numel() + torch.Size(dst).numel()) * es
    nbuf = max(2, min(8, -(-ROTATE_BYTES // io_bytes)))
    srcs = [torch.randn(src, device=DEV).to(dtype) for _ in range(nbuf)]
    w = (torch.randn(wshape, device=DEV) / (k ** nd * ci) ** 0.5).to(dtype)
    conf = ((s,) * nd, (p,) * nd, (1,) * nd, 1, "constant")
    row = {"shape": name, "what": what, "dtype": str(dtype).replace("torch.", ""), "B": B, "cin": ci, "cout": co, "size": list(size),
           "k": k, "stride": s, "padding": p, "output_padding": op, "buffers": nbuf, "device": torch.cuda.get_device_name(0),
           "iters": iters, "rounds": rounds, "roofline_us": round(io_bytes / HBM_BYTES_PER_US, 1)}
    tconvt = torch.nn.functional.conv_transpose2d if nd == 2 else torch.nn.functional.conv_transpose3d
    tdx = torch.nn.grad.conv2d_input if nd == 2 else torch.nn.grad.conv3d_input

    def ours():
        with torch.no_grad():
            if what == "dx":
                return [auto._grad_input(t, w, size, *conf) for t in srcs]
            return [fun.fft_conv_transpose(t, w, None, stride=s, padding=p, output_padding=op) for t in srcs]

    def under(env, fn=ours):
        def step():
            for var in KNOBS:
                os.environ.pop(var, None)
            os.environ.update(env)
            return fn()
        return step

    def route():
        if what == "dx":
            return auto.dx_route(torch.empty(dst, device=DEV, dtype=dtype), wshape, *conf)
        return fun.conv_route(srcs[0], wshape, s, p, transposed=True, output_padding=op)

    a_env = {"FFTCONV_DIRECT_TR": "1", "FFTCONV_DIRECT_BODY": "h16"} if h16 else {"FFTCONV_DIRECT_TR": "1"}
    steps = {"a_set": under(a_env), **({"a1_f32body": under({"FFTCONV_DIRECT_TR": "1"})} if h16 else {}), "b_unset": under({}),
             "d_torch": (lambda: [tdx(dst, w, t, s, p, 1, 1) for t in srcs]) if what == "dx" else
                        (lambda: [tconvt(t, w, None, s, p, op) for t in srcs])}
    row["a_set_route"] = under(a_env, route)()
    if h16:
        row["a1_f32body_route"] = under({"FFTCONV_DIRECT_TR": "1"}, route)()
    row["b_unset_route"] = under({}, route)()
    graphs = {}
    for key, fn in steps.items():
        try:
            graphs[key] = capture(fn)
        except Exception as exc:       # (a step that cannot run or be captured is reported, the others are still timed)
            row[key + "_us"] = None
            row[key + "_note"] = f"not captured: {str(exc)[:160]}"
            torch.cuda.synchronize()
    per_round, samples = {key: [] for key in graphs}, {key: [] for key in graphs}
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
    if row.get("a_set_us") and row.get("b_unset_us"):
        row["b_over_a"] = round(row["b_unset_us"] / row["a_set_us"], 2)
        row["a_roofline_fraction"] = round(row["roofline_us"] / row["a_set_us"], 3)
    if row.get("a_set_us") and row.get("a1_f32body_us"):
        row["a1_over_a"] = round(row["a1_f32body_us"] / row["a_set_us"], 2)
    for var in KNOBS:
        os.environ.pop(var, None)
    return row


def run_shape(fca, variants, whats, name, B, ci, co, g, size, k, s, dtype, iters, rounds, baseline):
    torch.manual_seed(0)
    nd = len(size)
    auto = importlib.import_module(fca.__name__ + ".autograd")
    fun = importlib.import_module(fca.__name__ + ".functional")
    tconv = torch.nn.functional.conv2d if nd == 2 else torch.nn.functional.conv3d
    es = torch.empty(0, dtype=dtype).element_size()
    out = tuple((n + 2 * (k // 2) - k) // s + 1 for n in size)
    io_bytes = B * (ci * torch.Size(size).numel() + co * torch.Size(out).numel()) * es
    nbuf = max(2, min(8, -(-ROTATE_BYTES // io_bytes)))
    xs = [torch.randn((B, ci) + size, device=DEV).to(dtype) for _ in range(nbuf)]
    gys = [torch.randn((B, co) + out, device=DEV).to(dtype) for _ in range(nbuf)]
    make = lambda: (fca.FFTConv2d if nd == 2 else fca.FFTConv3d)(ci, co, k, stride=s, padding=k // 2, groups=g,  # noqa: E731
                                                                bias=False).to(DEV).to(dtype)
    infer, train = make().eval(), make()
    w = train.weight.detach()
    conf = ((s,) * nd, (k // 2,) * nd, (1,) * nd, g, "constant")
    xg = [x.detach().requires_grad_() for x in xs]
    row = {"shape": name, "dtype": str(dtype).replace("torch.", ""), "B": B, "cin": ci, "cout": co, "groups": g, "size": list(size),
           "k": k, "stride": s, "buffers": nbuf, "device": torch.cuda.get_device_name(0), "iters": iters, "rounds": rounds,
           "knob": variants, "mode": "baseline" if baseline else "direct", "roofline_us": round(io_bytes / HBM_BYTES_PER_US, 1)}

    def under(env, fn):
        def step():
            for var in KNOBS:
                v = {"FFTCONV_WGRAD_DIRECT": "1", **env}.get(var)
                os.environ.pop(var, None) if v is None else os.environ.__setitem__(var, v)
            return fn()
        return step

    def fwd():
        with torch.no_grad():
            return [infer(x) for x in xs]

    def dx():
        with torch.no_grad():
            return [auto._grad_input(gy, w, size, *conf) for gy in gys]

    def torch_step():
        return [torch.autograd.grad(tconv(x, train.weight, None, s, k // 2, 1, g), (x, train.weight), gy) for x, gy in zip(xg, gys)]

    steps = {}
    for key, value in variants.items():
        steps[key + "_fwd"] = under(value, fwd)
        steps[key + "_dx"] = under(value, dx)
        steps[key + "_step"] = under(value, lambda: [torch.autograd.grad(train(x), (x, train.weight), gy) for x, gy in zip(xg, gys)])
        if hasattr(fun, "conv_route"):
            row[key + "_routes"] = under(value, lambda: [fun.conv_route(xs[0], tuple(w.shape), *conf[:4]),
                                                         auto.dx_route(xs[0], tuple(w.shape), *conf)])()
    if not baseline:
        tdx = torch.nn.grad.conv2d_input if nd == 2 else torch.nn.grad.conv3d_input
        steps["d_torch_fwd"] = lambda: [tconv(x, w, None, s, k // 2, 1, g) for x in xs]
        steps["d_torch_dx"] = lambda: [tdx(x.shape, w, gy, s, k // 2, 1, g) for x, gy in zip(xs, gys)]
        steps["d_torch_step"] = torch_step
    steps = {key: fn for key, fn in steps.items() if key.rsplit("_", 1)[1] in whats}
    graphs = {}
    for key, fn in steps.items():
        try:
            graphs[key] = capture(fn)
        except Exception as exc:       # (a step that cannot run or be captured is reported, the others are still timed)
            row[key + "_us"] = None
            row[key + "_note"] = f"not captured: {str(exc)[:160]}"
            torch.cuda.synchronize()
    per_round, samples = {key: [] for key in graphs}, {key: [] for key in graphs}
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
    for what in ("fwd", "dx", "step"):
        if row.get(f"a_set_{what}_us") and row.get(f"a1_f32body_{what}_us"):
            row[f"a1_over_a_{what}"] = round(row[f"a1_f32body_{what}_us"] / row[f"a_set_{what}_us"], 2)
        if row.get(f"a_set_{what}_us") and row.get(f"b_unset_{what}_us"):
            row[f"b_over_a_{what}"] = round(row[f"b_unset_{what}_us"] / row[f"a_set_{what}_us"], 2)
            if what != "step":
                row[f"a_roofline_fraction_{what}"] = round(row["roofline_us"] / row[f"a_set_{what}_us"], 3)
    for var in KNOBS:
        os.environ.pop(var, None)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dense", action="store_true", help="fc_conv_direct under FFTCONV_DIRECT on the shapes of DESIGN 4.5d")
    ap.add_argument("--h16", action="store_true", help="fc_conv_direct_h16 against fc_conv_direct on 16-bit tensors (DESIGN 4.5f)")
    ap.add_argument("--tr", action="store_true", help="fc_conv_direct_tr under FFTCONV_DIRECT_TR on strided transposed calls (DESIGN 4.5h)")
    ap.add_argument("--tr-h16", action="store_true", help="fc_conv_direct_tr_h16 against fc_conv_direct_tr on 16-bit tensors (DESIGN 4.5i)")
    ap.add_argument("--out", default=None, help="default: profiles/conv_direct_dw.jsonl, --dense: conv_direct.jsonl, --h16: conv_direct_h16.jsonl, "
                    "--tr: conv_direct_tr.jsonl, --tr-h16: conv_direct_tr_h16.jsonl")
    ap.add_argument("--only", default=None)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose fft_conv_pytorch_amd package is timed (default: this tree)")
    a = ap.parse_args()
    a.out = a.out or os.path.join("profiles", "conv_direct_tr_h16.jsonl" if a.tr_h16 else "conv_direct_tr.jsonl" if a.tr else "conv_direct_h16.jsonl" if a.h16 else "conv_direct.jsonl" if a.dense else "conv_direct_dw.jsonl")
    knob = "FFTCONV_DIRECT_DW" if not (a.dense or a.h16) else "FFTCONV_DIRECT"
    variants = {"c_parent": {}} if a.baseline else {"a_set": {knob: "1"}, "b_unset": {}}
    if a.h16:
        variants = {"a_set": {knob: "1", "FFTCONV_DIRECT_BODY": "h16"}, "a1_f32body": {knob: "1"}, "b_unset": {}}
    sys.path.insert(0, os.path.abspath(a.root))
    import fft_conv_pytorch_amd as fca
    assert os.path.abspath(fca.__file__).startswith(os.path.abspath(a.root)), fca.__file__
    for shape in (TR_H16 if a.tr_h16 else TR if a.tr else H16 if a.h16 else DENSE if a.dense else DW):
        if a.only and a.only not in shape[0]:
            continue
        res = run_tr_shape(fca, *shape, a.iters, a.rounds, a.tr_h16) if a.tr or a.tr_h16 else run_shape(fca, variants, ("fwd", "dx") if a.h16 else ("fwd", "dx", "step"), *shape, a.iters, a.rounds, a.baseline)
        line = json.dumps(res)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()
