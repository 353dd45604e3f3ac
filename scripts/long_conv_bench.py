#!/usr/bin/env python3
"""Times of ``fft_long_conv`` (one transform over the whole padded row) against the segment route of
``fft_conv`` for the same numbers and against the reference's torch.fft formulation, per shape:

  a   fft_long_conv, cached kernel spectrum                       a_train   forward + backward (dX, dW)
  b   fft_conv (segments of taps), cached kernel spectrum         b_train   forward + backward
  c   torch.fft.rfft / irfft on the padded row, kernel spectrum precomputed (fft_conv_pytorch functional.py:66-75)

Every step is captured into a HIP graph after a warm-up; the graphs of one shape are replayed in turn (a, b, c, a, b, c ...)
between HIP events of their own and the median replay is reported.  A step whose first replay is slower than --cap-ms is
replayed three times only.  One JSON line per shape is appended to --out with the device's name.

    python scripts/long_conv_bench.py [--iters 20] [--out profiles/long_conv.jsonl] [--only SUBSTRING] [--no-train]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fft_conv_pytorch_amd as fca  # noqa: E402
from fft_conv_pytorch_amd import functional as fc  # noqa: E402

DEV = "cuda:0"
# (name, batch, cin, cout, groups, L, K): padding K // 2 on both sides, so that fft_conv computes the same numbers
SHAPES = [(f"depthwise B4 C256 K=L={n}", 4, 256, 256, 256, n, n) for n in (8192, 16384, 65536, 262144)]
SHAPES += [(f"depthwise B8 C64 L65536 K{k}", 8, 64, 64, 64, 65536, k) for k in (4096, 16384, 65536)]
SHAPES += [("dense B4 8->8 K=L=32768", 4, 8, 8, 1, 32768, 32768)]


def capture(step):
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(3):
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


def run_shape(name, B, ci, co, g, L, K, iters, cap_ms, train):
    torch.manual_seed(0)
    p = K // 2
    x = torch.randn(B, ci, L, device=DEV)
    w = torch.randn(co, ci // g, K, device=DEV) / K ** 0.5
    row = {"shape": name, "B": B, "cin": ci, "cout": co, "groups": g, "L": L, "K": K, "padding": p,
           "device": torch.cuda.get_device_name(0), "iters": iters}
    long_plan = fc._long_plan(x, co, g, K, p, p, False, 0, False)
    row["long_plan"] = {k: long_plan.info[k] for k in ("N1", "N2", "slabs", "out_block")}
    spec_a = fc.transform_kernel(long_plan, w)
    seg_plan = fc._plan_for(x, w, None, 1, p, 1, g, "constant")
    row["fft_conv_route"] = {k: seg_plan.route[k] for k in ("T", "ntiles", "nseg")}
    spec_b = fc.transform_kernel(seg_plan, w)
    n = L + 2 * p
    n += n % 2
    wf = torch.fft.rfft(w, n).conj()

    def step_c():
        xf = torch.fft.rfft(F.pad(x, (p, p)), n)
        yf = torch.einsum("bgif,goif->bgof", xf.view(B, g, ci // g, -1), wf.view(g, co // g, ci // g, -1))
        return torch.fft.irfft(yf.reshape(B, co, -1), n)[..., :L + 2 * p - K + 1]

    steps = {"a": lambda: fc._fft_long_conv_impl(x, w, None, p, g, False, spec_a),
             "b": lambda: fc._fft_conv_impl(x, w, None, 1, p, 1, g, "constant", spec_b, seg_plan),
             "c": step_c}
    if train:
        xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
        steps["a_train"] = lambda: torch.autograd.grad(fca.fft_long_conv(xg, wg, padding=p, groups=g).square().sum(), (xg, wg))
        steps["b_train"] = lambda: torch.autograd.grad(fca.fft_conv(xg, wg, padding=p, groups=g).square().sum(), (xg, wg))
    with torch.no_grad():
        ya, yb = steps["a"](), steps["b"]()
        row["a_vs_b_max_rel"] = float((ya - yb).abs().max() / yb.abs().max())
        del ya, yb
    graphs = {}
    for key, fn in steps.items():
        try:
            if key.endswith("_train"):
                graphs[key] = capture(fn)
            else:
                with torch.no_grad():
                    graphs[key] = capture(fn)
        except Exception as exc:
            row[key + "_us"] = None
            row[key + "_note"] = f"not captured: {str(exc)[:120]}"
            torch.cuda.synchronize()
    samples = {key: [timed(gr)] for key, gr in graphs.items()}
    reps = {key: (iters if samples[key][0] <= cap_ms * 1e3 else 3) for key in graphs}
    for i in range(1, iters):
        for key, gr in graphs.items():          # in turn: a, b, c, a, b, c, ...
            if i < reps[key]:
                samples[key].append(timed(gr))
    for key, vals in samples.items():
        row[key + "_us"] = round(statistics.median(vals), 1)
        row[key + "_n"] = len(vals)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cap-ms", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join("profiles", "long_conv.jsonl"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    for shape in SHAPES:
        if a.only and a.only not in shape[0]:
            continue
        res = run_shape(*shape, iters=a.iters, cap_ms=a.cap_ms, train=not a.no_train)
        line = json.dumps(res)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()
