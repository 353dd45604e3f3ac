#!/usr/bin/env python3
"""complex64 ``fft_long_conv`` (one batch item per row of the transform) against what it replaces, on three
shapes of scripts/long_conv_bench.py, forward (cached kernel spectra) and one training step (forward + dX + dW) each:

  complex     (a) complex64 fft_long_conv, batch B
  real_2b     (b) float32 fft_long_conv at batch 2B on the same shape: the yardstick that can be derived -- a complex plan of
              B items launches the grids of a real plan of 2B items over the same bytes
  four_real   (c) what a caller wrote before: contiguous real / imaginary planes of x and w, four float32 calls, the two
              combining passes and the interleaving into a complex tensor, copies included
  torch_fft   (d) torch.fft.fft / ifft on the zero-padded row (reported, not gated)

Every step is captured into a HIP graph after a warm-up; the graphs of a shape are replayed in turn between HIP events of
their own and the median replay is reported, in ``--rounds`` alternating rounds, with (a) / (b) per round and the spread of
(b) across the rounds.  (a) is compared with (c) and (d) value for value.  One JSON line per shape is appended to --out.

    python scripts/long_complex_bench.py [--iters 20] [--rounds 3] [--out profiles/long_complex.jsonl] [--only SUBSTRING]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fft_conv_pytorch_amd as fca  # noqa: E402
from fft_conv_pytorch_amd import functional as fc  # noqa: E402
from long_conv_bench import DEV, capture, timed  # noqa: E402

# (name, batch, cin, cout, groups, L, K): padding K // 2 on both sides
SHAPES = [("depthwise B4 C256 K=L=65536", 4, 256, 256, 256, 65536, 65536),
          ("depthwise B8 C64 L65536 K4096", 8, 64, 64, 64, 65536, 4096),
          ("dense B4 8->8 K=L=32768", 4, 8, 8, 1, 32768, 32768)]


def _randc(*shape):
    return torch.view_as_complex(torch.randn(*shape, 2, device=DEV))


def run_shape(name, B, ci, co, g, L, K, iters, rounds, train):
    torch.manual_seed(0)
    p = K // 2
    x, w = _randc(B, ci, L), _randc(co, ci // g, K) / K ** 0.5
    x2 = torch.randn(2 * B, ci, L, device=DEV)
    plan = fc._long_plan(x, co, g, K, p, p, False, 0, False)
    row = {"shape": name, "B": B, "cin": ci, "cout": co, "groups": g, "L": L, "K": K, "padding": p,
           "device": torch.cuda.get_device_name(0), "iters": iters, "rounds": rounds,
           "long_plan": {k: plan.info[k] for k in ("N1", "N2", "slabs", "out_block")}}

    def module(dtype, weight):
        layer = fca.FFTLongConv1d(ci, co, K, padding=p, groups=g, bias=False, dtype=dtype).to(DEV).eval()
        with torch.no_grad():
            layer.weight.copy_(weight)
        return layer
    layer_c = module(torch.complex64, w)
    layer_re, layer_im = module(torch.float32, w.real), module(torch.float32, w.imag)

    def four_real(xc):
        xr, xi = xc.real.contiguous(), xc.imag.contiguous()
        return torch.complex(layer_re(xr) - layer_im(xi), layer_im(xr) + layer_re(xi))

    nfft = L + 2 * p
    wspec = torch.fft.fft(torch.nn.functional.pad(w.flip(-1), (0, nfft - K)), dim=-1)      # cached, as the others' spectra

    def torch_fft(xc):
        xs = torch.fft.fft(torch.nn.functional.pad(xc, (p, p)), dim=-1)
        if g == ci == co:
            ys = xs * wspec[:, 0]
        else:
            ys = torch.einsum("bgif,goif->bgof", xs.view(B, g, ci // g, nfft),
                              wspec.view(g, co // g, ci // g, nfft)).reshape(B, co, nfft)
        return torch.fft.ifft(ys, dim=-1)[..., K - 1:nfft].contiguous()

    steps = {"fwd_complex": lambda: layer_c(x), "fwd_real_2b": lambda: layer_re(x2),
             "fwd_four_real": lambda: four_real(x), "fwd_torch_fft": lambda: torch_fft(x)}
    if train:
        xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
        x2g, wrg = x2.clone().requires_grad_(), w.real.contiguous().requires_grad_()
        with torch.no_grad():
            gy = _randc(*layer_c(x).shape)
            gy2 = torch.randn_like(layer_re(x2))
        conv = lambda a, b: fca.fft_long_conv(a, b, padding=p, groups=g)      # noqa: E731

        def four_real_train():
            xr, xi = xg.real.contiguous(), xg.imag.contiguous()
            wr, wi = wg.real.contiguous(), wg.imag.contiguous()
            y = torch.complex(conv(xr, wr) - conv(xi, wi), conv(xr, wi) + conv(xi, wr))
            return torch.autograd.grad(y, (xg, wg), gy)

        def torch_fft_train():
            ws = torch.fft.fft(torch.nn.functional.pad(wg.flip(-1), (0, nfft - K)), dim=-1)
            xs = torch.fft.fft(torch.nn.functional.pad(xg, (p, p)), dim=-1)
            if g == ci == co:
                ys = xs * ws[:, 0]
            else:
                ys = torch.einsum("bgif,goif->bgof", xs.view(B, g, ci // g, nfft),
                                  ws.view(g, co // g, ci // g, nfft)).reshape(B, co, nfft)
            return torch.autograd.grad(torch.fft.ifft(ys, dim=-1)[..., K - 1:nfft], (xg, wg), gy)
        steps.update({"train_complex": lambda: torch.autograd.grad(conv(xg, wg), (xg, wg), gy),
                      "train_real_2b": lambda: torch.autograd.grad(conv(x2g, wrg), (x2g, wrg), gy2),
                      "train_four_real": four_real_train, "train_torch_fft": torch_fft_train})

    def call(key):
        if key.startswith("fwd"):
            with torch.no_grad():
                return steps[key]()
        return steps[key]()

    ya = call("fwd_complex")
    for other in ("fwd_four_real", "fwd_torch_fft"):
        yo = call(other)
        row[other + "_rel_diff"] = float((ya - yo).abs().max() / yo.abs().max())
        del yo
    del ya
    if train:
        ga = call("train_complex")
        gc = call("train_four_real")
        row["train_four_real_rel_diff"] = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(ga, gc))
        del ga, gc
    graphs = {key: capture(lambda: call(key)) for key in steps}
    per_round = {key: [] for key in graphs}
    for _ in range(rounds):
        samples = {key: [] for key in graphs}
        for _ in range(iters):
            for key, gr in graphs.items():          # in turn: complex, real_2b, four_real, torch_fft, ...
                samples[key].append(timed(gr))
        for key, vals in samples.items():
            per_round[key].append(round(statistics.median(vals), 1))
    for key, vals in per_round.items():
        row[key + "_us"] = vals
    for phase in ("fwd", "train") if train else ("fwd",):
        a, b = per_round[phase + "_complex"], per_round[phase + "_real_2b"]
        row[phase + "_complex_over_real_2b"] = [round(u / v, 3) for u, v in zip(a, b)]
        row[phase + "_real_2b_spread"] = round((max(b) - min(b)) / min(b), 3)
        row[phase + "_complex_over_four_real"] = round(statistics.median(a) / statistics.median(per_round[phase + "_four_real"]), 3)
        row[phase + "_complex_over_torch_fft"] = round(statistics.median(a) / statistics.median(per_round[phase + "_torch_fft"]), 3)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "long_complex.jsonl"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    for shape in SHAPES:
        if a.only and a.only not in shape[0]:
            continue
        res = run_shape(*shape, iters=a.iters, rounds=a.rounds, train=not a.no_train)
        line = json.dumps(res)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()
