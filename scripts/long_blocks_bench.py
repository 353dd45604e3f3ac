#!/usr/bin/env python3
"""Rows in overlap-save blocks over the long transform ("Rows longer than the transform: by blocks"):
``fft_long_conv(..., blocks=N)`` against the whole-row transform on the same tree and on the parent commit, K << L:

  a_blocks_<N>   ``blocks=N`` for every power of two N from the smallest the filter fits (taps <= N / 2, at least 4096) up to
                 the last that is smaller than the whole row's transform
  b_plain        the same tree without the keyword (absent where the row does not fit 2**24 points)
  b_plain_wgrad  training step only: b_plain under FFTCONV_LONG_WGRAD=1, dW from the weight-gradient plan of the whole row --
                 a step by blocks always takes dW from the weight-gradient plan by blocks, so this is its like-for-like
  c_parent       ``--baseline --root PARENT_CHECKOUT``: the same public calls, no keyword, with the package imported from a
                 checkout of the parent commit (``FFTCONV_LIB`` may name its library).  b against c shows nothing regressed.

Forward: eval() ``FFTLongConv1d`` with its cached kernel spectrum (padding 0).  Training step: forward + backward (dX, dW) of
``fft_long_conv`` on leaves.  Beside the times: spectrum + workspace bytes of the forward plan, and
``torch.cuda.max_memory_allocated`` over a warm step (inputs and outputs included).

Every step is captured into a HIP graph after a warm-up; one graph holds the step once per input buffer, and the buffers of
a shape are as many as it takes to move 600 MiB through a replay (at least two, at most eight), so no call finds its input
resident.  The graphs of a shape share one memory pool and are replayed in turn, in the order of their capture, between
HIP events, ``--iters`` replays in each of ``--rounds`` alternating rounds; reported are the median over all replays (60 by
default), per call, the medians of the single rounds, and their spread (largest minus smallest round median).  One JSON line
per (shape, kind) is appended to --out.

    python scripts/long_blocks_bench.py [--iters 20] [--rounds 3] [--out profiles/long_blocks.jsonl] [--only SUBSTRING]
                                        [--kinds forward,train] [--baseline [--root PARENT_CHECKOUT]]"""
import argparse
import json
import os
import statistics
import sys

import torch

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
# (name, batch, cin, cout, groups, L, K, dtype)
SHAPES = [
    ("depthwise B4 C256 L2^20 K16384", 4, 256, 256, 256, 1 << 20, 16384, F32),
    ("depthwise B4 C256 L2^18 K4096", 4, 256, 256, 256, 1 << 18, 4096, F32),
    ("dense B4 8->8 L2^22 K65536", 4, 8, 8, 1, 1 << 22, 65536, F32),
    ("depthwise B8 C768 L65536 K8192 bf16", 8, 768, 768, 768, 65536, 8192, BF16),
    ("B1 1->1 L2^24+4096 K1000", 1, 1, 1, 1, (1 << 24) + 4096, 1000, F32),
]
ROTATE_BYTES = 600 << 20
MAX_POINTS = 1 << 24


def capture(step, pool):
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, pool=pool):
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


def block_sizes(L, K):
    """The powers of two N with K <= N / 2, N >= 4096 and N < L (padding 0: the whole row needs L points)."""
    n, out = 4096, []
    while n < min(L, 2 * MAX_POINTS):
        if 2 * K <= n and n <= MAX_POINTS:
            out.append(n)
        n *= 2
    return out


def run_shape(fca, name, kind, B, ci, co, g, L, K, dtype, iters, rounds, baseline, sizes):
    torch.manual_seed(0)
    fwd = kind == "forward"
    lout = L - K + 1
    es = torch.empty(0, dtype=dtype).element_size()
    nbuf = max(2, min(8, -(-ROTATE_BYTES // (B * (ci * L + co * lout) * es))))
    xs = [torch.randn(B, ci, L, device=DEV).to(dtype) for _ in range(nbuf)]
    w = (torch.randn(co, ci // g, K, device=DEV) / (ci // g * K) ** 0.5).to(dtype)
    row = {"shape": name, "kind": kind, "dtype": str(dtype).replace("torch.", ""), "B": B, "cin": ci, "cout": co, "groups": g,
           "L": L, "K": K, "out_len": lout, "buffers": nbuf, "device": torch.cuda.get_device_name(0),
           "iters": iters, "rounds": rounds, "mode": "baseline" if baseline else "blocks"}

    if not fwd:      # (the leaves of the training steps, shared by every column)
        xg = [x.requires_grad_() for x in xs]
        wg = w.clone().requires_grad_()

    def make_step(blocks):
        kw = {} if blocks is None else {"blocks": blocks}
        if fwd:
            layer = fca.FFTLongConv1d(ci, co, K, groups=g, bias=False, **kw).to(DEV)
            with torch.no_grad():
                layer.weight.copy_(w)
            layer = layer.to(dtype).eval()

            def step():
                with torch.no_grad():
                    return [layer(x) for x in xs]
            return step
        return lambda: [torch.autograd.grad(fca.fft_long_conv(x, wg, None, 0, g, **kw).float().square().sum(), (x, wg))
                        for x in xg]

    def knob(value, fn):
        def step():
            if value is None:
                os.environ.pop("FFTCONV_LONG_WGRAD", None)
            else:
                os.environ["FFTCONV_LONG_WGRAD"] = value
            return fn()
        return step

    fits = L <= MAX_POINTS
    if baseline:
        steps = {"c_parent": make_step(None)} if fits else {}
    else:
        steps = {f"a_blocks_{n}": knob(None, make_step(n)) for n in sizes}
        if fits:
            steps["b_plain"] = knob(None, make_step(None))
        if fits and not fwd:
            steps["b_plain_wgrad"] = knob("1", make_step(None))
        from fft_conv_pytorch_amd import _native
        for n in sizes:      # what the forward plan holds: its spectrum and one slab of workspace
            geo = _native.blocks_geometry((B, ci, co, g, L, K, 0, 0, 0, 0, 0, n))
            row[f"a_blocks_{n}_plan_bytes"] = geo["spectrum_bytes"] + geo["workspace_bytes"]
            row[f"a_blocks_{n}_units"] = geo["U"]
        if fits:
            geo = _native.long_geometry((B, ci, co, g, L, K, 0, 0, 0, 0, 0))
            row["b_plain_plan_bytes"] = geo["spectrum_bytes"] + geo["workspace_bytes"]
    # peak memory of a warm step of each column, before any graph holds memory: inputs, results, workspaces
    for key, fn in steps.items():
        try:
            fn()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            row[key + "_max_memory_allocated"] = torch.cuda.max_memory_allocated()
        except Exception as exc:
            row[key + "_note"] = f"not run: {str(exc)[:160]}"
            torch.cuda.synchronize()
    torch.cuda.empty_cache()
    graphs = {}
    pool = torch.cuda.graph_pool_handle()      # (one pool for the graphs of a shape: they replay in turn, in capture order)
    for key, fn in steps.items():
        try:
            graphs[key] = capture(fn, pool)
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
    os.environ.pop("FFTCONV_LONG_WGRAD", None)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "long_blocks.jsonl"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--kinds", default="forward,train")
    ap.add_argument("--sizes", default=None, help="comma-separated block sizes instead of every eligible power of two")
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose fft_conv_pytorch_amd package is timed (default: this tree)")
    ap.add_argument("--tag", default=None, help="free text recorded with every row")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import fft_conv_pytorch_amd as fca
    assert os.path.abspath(fca.__file__).startswith(os.path.abspath(a.root)), fca.__file__
    for name, B, ci, co, g, L, K, dtype in SHAPES:
        if a.only and a.only not in name:
            continue
        sizes = block_sizes(L, K)
        if a.sizes:
            sizes = [n for n in sizes if n in {int(v) for v in a.sizes.split(",")}]
        for kind in a.kinds.split(","):
            res = run_shape(fca, name, kind, B, ci, co, g, L, K, dtype, a.iters, a.rounds, a.baseline, sizes)
            if a.tag:
                res["tag"] = a.tag
            line = json.dumps(res)
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
            torch.cuda.empty_cache()
