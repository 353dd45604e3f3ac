"""float16 / bfloat16 forward: the kernels reading and writing 16-bit tensors against the cast path (FFTCONV_HALF_IO=0).

For cfgA-cfgD of bench.py in bfloat16 and float16: an eval() module forward with its cached kernel spectrum, timed with
HIP events after a warm-up (several input buffers in rotation, > 2x the Infinity Cache in total), plus the peak memory a
call adds on top of its inputs.  One JSON line per (config, dtype, mode) goes to stdout and to profiles/half_io.jsonl
(or --out).

    python scripts/half_io_bench.py [--configs cfgA,cfgD] [--steps 50] [--warmup 10] [--out profiles/half_io.jsonl]
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
    layer = Layer(cin, cout, kernel, dilation=dil, groups=groups, bias=True).to(dev).to(dtype).eval()
    in_bytes = 2 * B * cin * math.prod(spatial)
    nbuf = max(2, min(16, int(2.2 * 256 * 2**20 / (2 * in_bytes)) + 1))
    xs = [torch.randn((B, cin) + spatial, device=dev).to(dtype) for _ in range(nbuf)]
    with torch.no_grad():
        for i in range(warmup):
            y = layer(xs[i % nbuf])
        del y
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = layer(xs[0])
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        out_samples = y.numel()
        del y
        times = []
        for i in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            layer(xs[i % nbuf])
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
    times.sort()
    us = sum(times[: max(1, len(times) - len(times) // 10)]) / max(1, len(times) - len(times) // 10)   # without the slowest 10 %
    return {"config": name, "dtype": str(dtype).replace("torch.", ""), "mode": mode, "us": round(us, 2),
            "median_us": round(times[len(times) // 2], 2), "gsamples_per_s": round(out_samples / us / 1e3, 3),
            "peak_increase_bytes": int(peak), "output_bytes": int(out_samples * 2), "steps": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfgA,cfgB,cfgC,cfgD")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_io.jsonl"))
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
