#!/usr/bin/env python3
"""``fft_long_conv_transpose`` ("Transposed: by phases"): the phases route against the zero-spread route of
the same tree, against what a caller ran before, and against torch, per shape (stride s, padding 0):

  a_phases     eval() FFTLongConvTranspose1d, cached kernel spectrum, the default route
  b_spread     the same layer under FFTCONV_LONG_POLY=0: the long primitive on the zero-spread row
  d_torch      torch.nn.functional.conv_transpose1d
  d_fft        the torch.fft formulation on the zero-spread row (rfft, product with the precomputed kernel spectrum, irfft)
  *_train      forward + backward (dX, dW) of a_phases and b_spread on leaves (the first and the third shape)

``--baseline`` times only ``FFTConvTranspose1d`` (c_parent, and c_parent_train) through what the parent commit's public
interface has, so that the same file runs against a checkout of the parent commit: ``--root DIR`` imports the package from
DIR instead of from this tree (``FFTCONV_LIB`` may name its library).  That run is the comparison of record.

Every step is captured into a HIP graph after a warm-up; one graph holds the step once per input buffer, and the buffers of
a shape are as many as it takes to move 600 MiB through a replay (more than twice the Infinity Cache), so no call finds
its input resident.  The graphs of a shape are replayed in turn between HIP events, ``--iters`` replays in each of
``--rounds`` alternating rounds; reported are the median over all replays, per call, and the medians of the single rounds.
A step whose first replay takes longer than --cap-ms is replayed three times per round.  One JSON line per shape is
appended to --out.

    python scripts/long_transpose_bench.py [--iters 20] [--rounds 3] [--out profiles/long_transpose.jsonl] [--only SUBSTRING]
                                           [--no-train] [--baseline [--root PARENT_CHECKOUT]]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
# (name, batch, cin, cout, groups, L, K, stride, dtype, also timed in training)
SHAPES = [
    ("depthwise B4 C256 L16384 K16384 s4", 4, 256, 256, 256, 16384, 16384, 4, F32, True),
    ("depthwise B4 C256 L8192 K4096 s8", 4, 256, 256, 256, 8192, 4096, 8, F32, False),
    ("dense B4 8->8 L32768 K8192 s2", 4, 8, 8, 1, 32768, 8192, 2, F32, True),
    ("depthwise B8 C768 L8192 K1024 s2 bf16", 8, 768, 768, 768, 8192, 1024, 2, BF16, False),
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


def run_shape(fca, name, B, ci, co, g, L, K, s, dtype, train, iters, rounds, cap_ms, baseline, torch_direct):
    torch.manual_seed(0)
    lout = (L - 1) * s + K
    es = torch.empty(0, dtype=dtype).element_size()
    nbuf = max(2, min(8, -(-ROTATE_BYTES // (B * (ci * L + co * lout) * es))))
    xs = [torch.randn(B, ci, L, device=DEV).to(dtype) for _ in range(nbuf)]
    w = (torch.randn(ci, co // g, K, device=DEV) / (ci // g * K / s) ** 0.5).to(dtype)
    row = {"shape": name, "dtype": str(dtype).replace("torch.", ""), "B": B, "cin": ci, "cout": co, "groups": g, "L": L, "K": K,
           "stride": s, "out_len": lout, "buffers": nbuf, "device": torch.cuda.get_device_name(0), "iters": iters,
           "rounds": rounds, "mode": "baseline" if baseline else "long"}

    def layer_of(cls):
        layer = cls(ci, co, K, stride=s, groups=g, bias=False).to(DEV)
        with torch.no_grad():
            layer.weight.copy_(w)
        return layer.to(dtype).eval()

    def each(fn):                    # one graph: the step on every buffer in turn
        return lambda: [fn(x) for x in xs]

    def knob(value, fn):
        def step():
            os.environ["FFTCONV_LONG_POLY"] = value
            return fn()
        return step

    xg = [x.clone().requires_grad_() for x in xs]
    wg = w.clone().requires_grad_()
    steps = {}
    if baseline:
        parent = layer_of(fca.FFTConvTranspose1d)
        steps["c_parent"] = each(parent)
        if train:
            from fft_conv_pytorch_amd.functional import fft_conv_transpose
            steps["c_parent_train"] = lambda: [torch.autograd.grad(fft_conv_transpose(x, wg, None, s, 0, 0, 1, g).square().sum(), (x, wg))
                                               for x in xg]
    else:
        from fft_conv_pytorch_amd import functional as fc
        row["route"] = fc._long_transpose_route(xs[0].shape, w.shape, s, 0, 0, 1, g, dtype)
        spread_need, phases_need = fc._long_transpose_needs(L, K, s, 0, 0, 1)
        row["points"] = {"phases": phases_need, "spread": spread_need}
        la, lb = layer_of(fca.FFTLongConvTranspose1d), layer_of(fca.FFTLongConvTranspose1d)
        steps["a_phases"] = knob("1", each(la))
        steps["b_spread"] = knob("0", each(lb))
        n = 1 << (lout + K - 2).bit_length()      # the zero-spread row with K - 1 zeros on both sides, as the model project pads it
        if torch_direct:
            steps["d_torch"] = each(lambda x: F.conv_transpose1d(x, w, None, s, 0, 0, g))
        wf = torch.fft.rfft(w.float(), n)                               # (Cin, Cout/g, n/2 + 1): kept between calls

        def by_fft(x):
            spread = x.new_zeros(B, ci, (L - 1) * s + 1, dtype=F32)
            spread[..., ::s] = x
            xf = torch.fft.rfft(spread, n)
            yf = torch.einsum("bgif,giof->bgof", xf.view(B, g, ci // g, -1), wf.view(g, ci // g, co // g, -1))
            return torch.fft.irfft(yf.reshape(B, co, -1), n)[..., :lout].to(dtype)
        steps["d_fft"] = each(by_fft)
        if train:
            def train_step(x):
                return torch.autograd.grad(fca.fft_long_conv_transpose(x, wg, None, s, 0, 0, 1, g).square().sum(), (x, wg))
            steps["a_phases_train"] = knob("1", lambda: [train_step(x) for x in xg])
            steps["b_spread_train"] = knob("0", lambda: [train_step(x) for x in xg])
        with torch.no_grad():
            ya, yb, yd = steps["a_phases"]()[0].float(), steps["b_spread"]()[0].float(), by_fft(xs[0]).float()
            row["a_vs_b_max_rel"] = float((ya - yb).abs().max() / yb.abs().max())
            row["a_vs_fft_max_rel"] = float((ya - yd).abs().max() / yd.abs().max())
            del ya, yb, yd

    graphs = {}
    for key, fn in steps.items():
        try:
            t0 = time.time()
            if key.endswith("_train"):
                fn()
            else:
                with torch.no_grad():
                    fn()
            torch.cuda.synchronize()
            first = time.time() - t0
            if key == "d_torch" and first > 20 * cap_ms * 1e-3 * nbuf:
                row[key + "_us"] = None
                row[key + "_note"] = f"not timed: the first call took {first / nbuf * 1e3:.0f} ms"
                continue
            if key.endswith("_train"):
                graphs[key] = capture(fn)
            else:
                with torch.no_grad():
                    graphs[key] = capture(fn)
        except Exception as exc:       # (a step torch cannot capture is reported, the others are still timed)
            row[key + "_us"] = None
            row[key + "_note"] = f"not captured: {str(exc)[:120]}"
            torch.cuda.synchronize()
    per_round = {key: [] for key in graphs}
    samples = {key: [] for key in graphs}
    slow = {key: timed(gr) / nbuf > cap_ms * 1e3 for key, gr in graphs.items()}
    for _ in range(rounds):
        this = {key: [] for key in graphs}
        for i in range(iters):
            for key, gr in graphs.items():          # in turn
                if i < (3 if slow[key] else iters):
                    this[key].append(timed(gr) / nbuf)
        for key, vals in this.items():
            per_round[key].append(round(statistics.median(vals), 1))
            samples[key] += vals
    for key, vals in samples.items():
        row[key + "_us"] = round(statistics.median(vals), 1)
        row[key + "_rounds_us"] = per_round[key]
        row[key + "_n"] = len(vals)
    if not baseline and row.get("a_phases_us") and row.get("b_spread_us"):
        row["a_over_b"] = round(row["a_phases_us"] / row["b_spread_us"], 3)
        if row.get("a_phases_train_us") and row.get("b_spread_train_us"):
            row["a_over_b_train"] = round(row["a_phases_train_us"] / row["b_spread_train_us"], 3)
    os.environ.pop("FFTCONV_LONG_POLY", None)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cap-ms", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join("profiles", "long_transpose.jsonl"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--no-torch-direct", action="store_true", help="leave out torch's conv_transpose1d (d_torch)")
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose fft_conv_pytorch_amd package is timed (default: this tree)")
    ap.add_argument("--tag", default=None, help="free text recorded with every row")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import fft_conv_pytorch_amd as fca
    assert os.path.abspath(fca.__file__).startswith(os.path.abspath(a.root)), fca.__file__
    for name, B, ci, co, g, L, K, s, dtype, train in SHAPES:
        if a.only and a.only not in name:
            continue
        res = run_shape(fca, name, B, ci, co, g, L, K, s, dtype, train and not a.no_train, a.iters, a.rounds, a.cap_ms,
                        a.baseline, not a.no_torch_direct)
        if a.tag:
            res["tag"] = a.tag
        line = json.dumps(res)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()
