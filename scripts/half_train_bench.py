"""float16 / bfloat16 training step: the kernels reading 16-bit x and dY in backward against the cast path
(FFTCONV_HALF_IO=0, which widens the signal, weight and bias and saves the float32 copy of the signal).

For cfgA-cfgD of bench.py in bfloat16 and float16: a train() module forward + backward (dX, dW, db), timed with HIP events
after a warm-up (several input buffers in rotation, > 2x the Infinity Cache in total), plus the peak memory a step adds on
top of its inputs and output gradient.  One JSON line per (config, dtype, mode) goes to stdout and to
profiles/half_train.jsonl (or --out).

    python scripts/half_train_bench.py [--configs cfgA,cfgD] [--steps 30] [--warmup 5] [--out profiles/half_train.jsonl]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (ndim, batch, cin, cout, groups, spatial, kernel, dilation), as bench.py CONFIGS
CONFIGS = {
    "cfgA": (1, 32, 8, 8, 1, (32768,), (512,), 1),
    "cfgB": (2, 16, 8, 8, 1, (512, 512), (31, 31), 1),
    "cfgC": (3, 8, 8, 8, 1, (64, 64, 64), (9, 9, 9), 1),
    "cfgD": (1, 8, 64, 64, 8, (1 << 20,), (257,), 4),
}


def run(name, dtype, mode, steps, warmup):
    import fft_conv_pytorch_amd as fca
    ndim, B, cin, cout, groups, spatial, kernel, dil = CONFIGS[name]
    os.environ["FFTCONV_HALF_IO"] = "1" if mode == "native" else "0"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    Layer = {1: fca.FFTConv1d, 2: fca.FFTConv2d, 3: fca.FFTConv3d}[ndim]
    layer = Layer(cin, cout, kernel, dilation=dil, groups=groups, bias=True).to(dev).to(dtype).train()
    in_bytes = 2 * B * cin * math.prod(spatial)
    nbuf = max(2, min(8, int(2.2 * 256 * 2**20 / (2 * in_bytes)) + 1))
    xs = [torch.randn((B, cin) + spatial, device=dev).to(dtype).requires_grad_() for _ in range(nbuf)]
    with torch.no_grad():
        gy = torch.randn(layer(xs[0]).shape, device=dev).to(dtype)

    def step(x):
        layer.zero_grad(set_to_none=True)
        x.grad = None
        layer(x).backward(gy)

    for i in range(warmup):
        step(xs[i % nbuf])
    torch.cuda.synchronize()
    layer.zero_grad(set_to_none=True)
    for x in xs:
        x.grad = None
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step(xs[0])
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    times = []
    for i in range(steps):
        x = xs[i % nbuf]
        layer.zero_grad(set_to_none=True)
        x.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        layer(x).backward(gy)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    times.sort()
    keep = max(1, len(times) - len(times) // 10)         # without the slowest 10 %
    us = sum(times[:keep]) / keep
    return {"config": name, "dtype": str(dtype).replace("torch.", ""), "mode": mode, "us": round(us, 2),
            "median_us": round(times[len(times) // 2], 2), "peak_increase_bytes": int(peak),
            "input_samples": int(xs[0].numel()), "steps": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfgA,cfgB,cfgC,cfgD")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_train.jsonl"))
    args = ap.parse_args()
    lines = []
    for name in args.configs.split(","):
        for dtype in (torch.bfloat16, torch.float16):
            res = {m: run(name, dtype, m, args.steps, args.warmup) for m in ("native", "cast")}
            res["native"]["speedup_vs_cast"] = round(res["cast"]["us"] / res["native"]["us"], 3)
            for m in ("native", "cast"):
                print(json.dumps(res[m]), flush=True)
                lines.append(res[m])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
