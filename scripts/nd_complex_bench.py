#!/usr/bin/env python3
"""complex64 2-D / 3-D ``fft_conv`` against what a user could run before it, on the same tree:

  a_complex    ``FFTConv2d/3d(dtype=complex64)`` in eval mode: one complex plan, its kernel spectrum cached by the module
  b_four_real  the same result from float32 modules: the two planes of x copied out, four real calls (weight.real and
               weight.imag modules, spectra cached) and two combining passes that write the planes of the complex result
  c_torch      ``torch.nn.functional.conv2d`` / ``conv3d`` on the complex tensors
  d_torch_fft  the torch.fft formulation: fftn of signal and zero-extended kernel, product summed over the input
               channels, ifftn, crop

and one training step (forward, dX and dW from a given dY, no bias) of a and b.

Every measured call is captured into a HIP graph after a warm-up (a call that cannot be captured is timed eagerly and
marked); one graph holds the call once per input buffer, and the buffers of a shape are as many as it takes to move
600 MiB through a replay (at least two, at most eight).  The graphs of a shape are replayed in turn between HIP events,
``--iters`` replays in each of ``--rounds`` alternating rounds (two per round for a variant whose replay takes longer than
a quarter of a second; a variant that takes seconds per call is timed eagerly, once); reported are the median over all replays, per call, the medians of the rounds, and their spread.
One JSON line per shape is appended to --out.

    python scripts/nd_complex_bench.py [--iters 20] [--rounds 3] [--out profiles/nd_complex.jsonl] [--only SUBSTRING]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

DEV = "cuda:0"
C64 = torch.complex64
# (name, batch, cin, cout, spatial, kernel)
SHAPES = [
    ("cfgB 2-D B16 8->8 512^2 k31", 16, 8, 8, (512, 512), (31, 31)),
    ("2-D B4 8->8 256^2 k15", 4, 8, 8, (256, 256), (15, 15)),
    ("cfgC 3-D B8 8->8 64^3 k9", 8, 8, 8, (64, 64, 64), (9, 9, 9)),
]
ROTATE_BYTES = 600 << 20
SLOW_US = 250e3


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
    return g.replay


def timed(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def run_shape(fca, name, B, ci, co, size, k, iters, rounds):
    torch.manual_seed(0)
    nd = len(size)
    out_sp = tuple(s - q + 1 for s, q in zip(size, k))
    vol = lambda t: int(torch.tensor(t).prod())      # noqa: E731
    nbuf = max(2, min(8, -(-ROTATE_BYTES // (8 * B * (ci * vol(size) + co * vol(out_sp))))))
    xs = [torch.randn((B, ci) + size, device=DEV, dtype=C64) for _ in range(nbuf)]
    gys = [torch.randn((B, co) + out_sp, device=DEV, dtype=C64) for _ in range(nbuf)]
    conv = (fca.FFTConv2d, fca.FFTConv3d)[nd - 2]
    layer = conv(ci, co, k, bias=False, dtype=C64).to(DEV)
    lr, li = (conv(ci, co, k, bias=False).to(DEV) for _ in range(2))
    with torch.no_grad():
        lr.weight.copy_(layer.weight.real)
        li.weight.copy_(layer.weight.imag)
    w = layer.weight.detach()
    # The training steps run on modules of their own.  A captured inference call reads the kernel spectrum its module
    # caches; a call in train() mode drops that cache, and the next capture returns freed blocks to the device
    # (torch.cuda.graph empties the allocator's cache on entry): a replay of the inference graph would then read
    # unmapped memory.  No module here changes its mode after its first call.
    layer_t, lr_t, li_t = conv(ci, co, k, bias=False, dtype=C64).to(DEV), conv(ci, co, k, bias=False).to(DEV), conv(ci, co, k, bias=False).to(DEV)
    for dst, src in ((layer_t, layer), (lr_t, lr), (li_t, li)):
        dst.load_state_dict(src.state_dict())
        dst.train()
        src.eval()

    def four_real(x):
        planes = torch.view_as_real(x)
        xr, xi = planes[..., 0].contiguous(), planes[..., 1].contiguous()
        rr, ii, ri, ir = lr(xr), li(xi), li(xr), lr(xi)
        out = torch.empty(rr.shape, device=DEV, dtype=C64)
        o = torch.view_as_real(out)
        torch.sub(rr, ii, out=o[..., 0])
        torch.add(ri, ir, out=o[..., 1])
        return out

    def four_real_autograd(x):      # (the same with differentiable combining passes)
        xr, xi = x.real.contiguous(), x.imag.contiguous()
        return torch.complex(lr_t(xr) - li_t(xi), li_t(xr) + lr_t(xi))

    tconv = (F.conv2d, F.conv3d)[nd - 2]
    dims = tuple(range(2, 2 + nd))

    def torch_fft(x):
        xf = torch.fft.fftn(x, dim=dims)
        wf = torch.fft.fftn(w.flip(dims), s=size, dim=dims)
        yf = torch.einsum("bi...,oi...->bo...", xf, wf)
        y = torch.fft.ifftn(yf, dim=dims)
        return y[(Ellipsis,) + tuple(slice(q - 1, None) for q in k)].contiguous()

    row = {"shape": name, "B": B, "cin": ci, "cout": co, "size": list(size), "kernel": list(k), "buffers": nbuf,
           "device": torch.cuda.get_device_name(0), "iters": iters, "rounds": rounds}
    with torch.no_grad():
        ya, yb = layer(xs[0]), four_real(xs[0])
        scale = ya.abs().max()
        row["route"] = next(p for key, p in fca._native._plans.items() if key[-1] == fca._native.FC_C64).route
        row["b_vs_a_max_rel"] = float((yb - ya).abs().max() / scale)
        try:
            row["d_vs_a_max_rel"] = float((torch_fft(xs[0]) - ya).abs().max() / scale)
        except Exception as exc:
            row["d_torch_fft_note"] = f"failed: {str(exc)[:160]}"
        del ya, yb

    def inference(fn):
        def step():
            with torch.no_grad():
                return [fn(x) for x in xs]
        return step

    xg = [x.detach().requires_grad_() for x in xs]

    def train_a():
        return [torch.autograd.grad(layer_t(x), (x, layer_t.weight), gy) for x, gy in zip(xg, gys)]

    def train_b():
        return [torch.autograd.grad(four_real_autograd(x), (x, lr_t.weight, li_t.weight), gy) for x, gy in zip(xg, gys)]

    steps = {"a_complex": inference(layer), "b_four_real": inference(four_real),
             "c_torch": inference(lambda x: tconv(x, w)), "d_torch_fft": inference(torch_fft),
             "a_complex_step": train_a, "b_four_real_step": train_b}
    runs = {}
    for key, fn in steps.items():
        try:
            fn()                                   # (plans, library warm-up)
            torch.cuda.synchronize()
            if timed(fn) > 8 * SLOW_US * nbuf:     # seconds per call: one more eager sample stands for the variant
                row[key + "_us"], row[key + "_n"] = round(timed(fn) / nbuf, 1), 1
                row[key + "_note"] = "one eager sample (seconds per call)"
                continue
            runs[key] = capture(fn)
        except Exception as exc:
            torch.cuda.synchronize()
            row[key + "_note"] = f"not captured ({str(exc)[:120]}): timed eagerly"
            try:
                fn()
                torch.cuda.synchronize()
                runs[key] = fn
            except Exception as exc2:
                row[key + "_us"] = None
                row[key + "_note"] = f"failed: {str(exc2)[:160]}"
                torch.cuda.synchronize()
    n_of = {key: (iters if timed(run) < SLOW_US else 2) for key, run in runs.items()}
    per_round = {key: [] for key in runs}
    samples = {key: [] for key in runs}
    for _ in range(rounds):
        this = {key: [] for key in runs}
        for i in range(iters):
            for key, run in runs.items():          # in turn
                if i < n_of[key]:
                    this[key].append(timed(run) / nbuf)
        for key, vals in this.items():
            per_round[key].append(round(statistics.median(vals), 1))
            samples[key] += vals
    for key, vals in samples.items():
        if not vals:
            continue
        row[key + "_us"] = round(statistics.median(vals), 1)
        row[key + "_rounds_us"] = per_round[key]
        row[key + "_spread_us"] = round(max(per_round[key]) - min(per_round[key]), 1)
        row[key + "_n"] = len(vals)
    for num, den, what in (("a_complex", "b_four_real", "a_over_b"), ("a_complex_step", "b_four_real_step", "a_over_b_step"),
                           ("a_complex", "c_torch", "a_over_c"), ("a_complex", "d_torch_fft", "a_over_d")):
        if row.get(num + "_us") and row.get(den + "_us"):
            row[what] = round(row[num + "_us"] / row[den + "_us"], 3)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "nd_complex.jsonl"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--tag", default=None, help="free text recorded with every row")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import fft_conv_pytorch_amd as fca
    for name, B, ci, co, size, k in SHAPES:
        if a.only and a.only not in name:
            continue
        fca._native.clear_plan_cache()
        res = run_shape(fca, name, B, ci, co, size, k, a.iters, a.rounds)
        if a.tag:
            res["tag"] = a.tag
        line = json.dumps(res)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()
