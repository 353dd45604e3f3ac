#!/usr/bin/env python3
"""The decimation route of the long-filter path ("Strided: by decimated rows"): ``fft_long_conv`` with a
stride run on the ``stride`` decimated rows, and the training step of ``fft_long_conv_transpose`` with both gradients on
rows ``stride`` times shorter, against the constructions of before on the same tree and on the parent commit:

  a_decim      FFTCONV_LONG_DECIM=1
  b_plain      FFTCONV_LONG_DECIM=0 on the same tree
  c_parent     ``--baseline --root PARENT_CHECKOUT``: the same public calls with the package imported from a checkout of the
               parent commit (``FFTCONV_LIB`` may name its library).  That run is the comparison of record.

Forward: eval() ``FFTLongConv1d`` with its cached kernel spectrum (no padding).  Training step: forward + backward (dX, dW)
of ``fft_long_conv_transpose`` on leaves, the four shapes of scripts/long_transpose_bench.py.

Every step is captured into a HIP graph after a warm-up; one graph holds the step once per input buffer, and the buffers of
a shape are as many as it takes to move 600 MiB through a replay (at least two, at most eight), so no call finds its input
resident.  The graphs of a shape are replayed in turn between HIP events, ``--iters`` replays in each of ``--rounds``
alternating rounds; reported are the median over all replays (60 by default), per call, the medians of the single rounds,
and their spread (largest minus smallest round median).  One JSON line per shape is appended to --out.

    python scripts/long_decim_bench.py [--iters 20] [--rounds 3] [--out profiles/long_decim.jsonl] [--only SUBSTRING]
                                       [--baseline [--root PARENT_CHECKOUT]]"""
import argparse
import json
import os
import statistics
import sys

import torch

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
# (name, kind, batch, cin, cout, groups, L, K, stride, dtype)
SHAPES = [
    ("fwd depthwise B4 C256 L65536 K16384 s4", "forward", 4, 256, 256, 256, 65536, 16384, 4, F32),
    ("fwd dense B4 8->8 L65536 K8192 s2", "forward", 4, 8, 8, 1, 65536, 8192, 2, F32),
    ("train T depthwise B4 C256 L16384 K16384 s4", "train_transpose", 4, 256, 256, 256, 16384, 16384, 4, F32),
    ("train T depthwise B4 C256 L8192 K4096 s8", "train_transpose", 4, 256, 256, 256, 8192, 4096, 8, F32),
    ("train T dense B4 8->8 L32768 K8192 s2", "train_transpose", 4, 8, 8, 1, 32768, 8192, 2, F32),
    ("train T depthwise B8 C768 L8192 K1024 s2 bf16", "train_transpose", 8, 768, 768, 768, 8192, 1024, 2, BF16),
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


def run_shape(fca, name, kind, B, ci, co, g, L, K, s, dtype, iters, rounds, baseline):
    torch.manual_seed(0)
    fwd = kind == "forward"
    lout = (L - K) // s + 1 if fwd else (L - 1) * s + K
    es = torch.empty(0, dtype=dtype).element_size()
    nbuf = max(2, min(8, -(-ROTATE_BYTES // (B * (ci * L + co * lout) * es))))
    xs = [torch.randn(B, ci, L, device=DEV).to(dtype) for _ in range(nbuf)]
    wshape = (co, ci // g, K) if fwd else (ci, co // g, K)
    w = (torch.randn(wshape, device=DEV) / (ci // g * K) ** 0.5).to(dtype)
    row = {"shape": name, "kind": kind, "dtype": str(dtype).replace("torch.", ""), "B": B, "cin": ci, "cout": co, "groups": g,
           "L": L, "K": K, "stride": s, "out_len": lout, "buffers": nbuf, "device": torch.cuda.get_device_name(0),
           "iters": iters, "rounds": rounds, "mode": "baseline" if baseline else "decim"}

    def knob(value, fn):
        def step():
            os.environ["FFTCONV_LONG_DECIM"] = value
            return fn()
        return step

    def make_step():
        if fwd:
            layer = fca.FFTLongConv1d(ci, co, K, groups=g, bias=False, stride=s).to(DEV)
            with torch.no_grad():
                layer.weight.copy_(w)
            layer = layer.to(dtype).eval()

            def step():
                with torch.no_grad():
                    return [layer(x) for x in xs]
            return step
        xg = [x.clone().requires_grad_() for x in xs]
        wg = w.clone().requires_grad_()
        return lambda: [torch.autograd.grad(fca.fft_long_conv_transpose(x, wg, None, s, 0, 0, 1, g).float().square().sum(), (x, wg))
                        for x in xg]

    steps = {"c_parent": make_step()} if baseline else {"a_decim": knob("1", make_step()), "b_plain": knob("0", make_step())}
    if not baseline:
        ra, rb = steps["a_decim"]()[0], steps["b_plain"]()[0]
        for label, ta, tb in zip(("y",) if fwd else ("dX", "dW"), (ra,) if fwd else ra, (rb,) if fwd else rb):
            row[f"a_vs_b_{label}_max_rel"] = float((ta.float() - tb.float()).abs().max() / tb.float().abs().max())
        del ra, rb
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
    if row.get("a_decim_us") and row.get("b_plain_us"):
        row["a_over_b"] = round(row["a_decim_us"] / row["b_plain_us"], 3)
    os.environ.pop("FFTCONV_LONG_DECIM", None)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "long_decim.jsonl"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose fft_conv_pytorch_amd package is timed (default: this tree)")
    ap.add_argument("--tag", default=None, help="free text recorded with every row")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import fft_conv_pytorch_amd as fca
    assert os.path.abspath(fca.__file__).startswith(os.path.abspath(a.root)), fca.__file__
    for name, kind, B, ci, co, g, L, K, s, dtype in SHAPES:
        if a.only and a.only not in name:
            continue
        res = run_shape(fca, name, kind, B, ci, co, g, L, K, s, dtype, a.iters, a.rounds, a.baseline)
        if a.tag:
            res["tag"] = a.tag
        line = json.dumps(res)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()
