#!/usr/bin/env python3
"""Times of ``fft_long_conv`` with a stride, a dilation or a padding mode against ``fft_conv`` on the same
arguments and against the torch.fft formulation a caller would write (zero-stuffed kernel, ``F.pad`` in the mode, rfft /
irfft over the padded row, strided slice), per variant of depthwise B4 C256 L = 65536 K = 16384:

  a   fft_long_conv, cached kernel spectrum                       a_train   forward + backward (dX, dW), --train variants
  b   fft_conv, cached kernel spectrum                            b_train   forward + backward
  c   torch.fft, kernel spectrum precomputed

The protocol is the one of scripts/long_conv_bench.py (its capture and timing helpers are used): HIP-graph replays, the
steps of a variant replayed in turn, the median reported; a step slower than --cap-ms is replayed three times only.

    python scripts/long_conv_general_bench.py [--iters 20] [--out profiles/long_conv_general.jsonl] [--only SUBSTRING]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fft_conv_pytorch_amd as fca  # noqa: E402
from fft_conv_pytorch_amd import _native, functional as fc  # noqa: E402
from long_conv_bench import DEV, capture, timed  # noqa: E402

B, C, L, K = 4, 256, 65536, 16384
# (name, stride, dilation, padding, padding_mode, with a training step)
VARIANTS = [
    ("dilation 4, zero padding 2 (K - 1)", 1, 4, 2 * (K - 1), "constant", True),
    ("stride 4, zero padding K // 2", 4, 1, K // 2, "constant", False),
    ("circular padding K // 2", 1, 1, K // 2, "circular", False),
    ("stride 1, dilation 1, zero padding K // 2 (the plain build)", 1, 1, K // 2, "constant", False),
]


def run_variant(name, s, d, p, mode, train, iters, cap_ms):
    torch.manual_seed(0)
    x = torch.randn(B, C, L, device=DEV)
    w = torch.randn(C, 1, K, device=DEV) / K ** 0.5
    row = {"variant": name, "B": B, "C": C, "L": L, "K": K, "stride": s, "dilation": d, "padding": p, "padding_mode": mode,
           "device": torch.cuda.get_device_name(0), "iters": iters}
    long_plan = fc._long_plan(x, C, C, K, p, p, False, 0, False, pad_mode=_native.PAD_MODES[mode], tap_dil=d, out_step=s)
    row["long_plan"] = {k: long_plan.info[k] for k in ("N1", "N2", "slabs", "out_len")}
    spec_a = fc.transform_kernel(long_plan, w)
    try:
        seg_plan = fc._plan_for(x, w, None, s, p, d, C, mode)
        row["fft_conv_route"] = {k: seg_plan.route[k] for k in ("T", "ntiles", "nseg")}
        spec_b = fc.transform_kernel(seg_plan, w)
    except (NotImplementedError, ValueError) as exc:
        seg_plan, row["b_note"] = None, f"no fft_conv plan: {str(exc)[:120]}"
    n = L + 2 * p
    n += n % 2
    span = L + 2 * p - d * (K - 1)
    wd = torch.zeros(C, d * (K - 1) + 1, device=DEV)
    wd[:, ::d] = w[:, 0]
    wf = torch.fft.rfft(wd, n).conj()
    del wd

    def step_c():
        xp = F.pad(x, (p, p), mode=mode)
        return torch.fft.irfft(torch.fft.rfft(xp, n) * wf, n)[..., :span:s]

    steps = {"a": lambda: fc._fft_long_conv_impl(x, w, None, p, C, False, spec_a, s, d, mode), "c": step_c}
    if seg_plan is not None:
        steps["b"] = lambda: fc._fft_conv_impl(x, w, None, s, p, d, C, mode, spec_b, seg_plan)
    kw = dict(stride=s, padding=p, dilation=d, groups=C, padding_mode=mode)
    if train:
        xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
        steps["a_train"] = lambda: torch.autograd.grad(fca.fft_long_conv(xg, wg, **kw).square().sum(), (xg, wg))
        if seg_plan is not None:
            steps["b_train"] = lambda: torch.autograd.grad(fca.fft_conv(xg, wg, **kw).square().sum(), (xg, wg))
    with torch.no_grad():
        ya, yc = steps["a"](), steps["c"]()
        assert ya.shape == yc.shape, (ya.shape, yc.shape)
        row["a_vs_c_max_rel"] = float((ya - yc).abs().max() / yc.abs().max())
        if seg_plan is not None:
            yb = steps["b"]()
            row["a_vs_b_max_rel"] = float((ya - yb).abs().max() / yb.abs().max())
            del yb
        del ya, yc
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
        for key, gr in graphs.items():
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
    ap.add_argument("--out", default=os.path.join("profiles", "long_conv_general.jsonl"))
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    for variant in VARIANTS:
        if a.only and a.only not in variant[0]:
            continue
        res = run_variant(*variant, iters=a.iters, cap_ms=a.cap_ms)
        line = json.dumps(res)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()
