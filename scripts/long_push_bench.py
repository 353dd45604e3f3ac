#!/usr/bin/env python3
"""Appending T tokens to a stream of a causal long filter ("Pushing many tokens at once"): microseconds per
append, four ways, on the four shapes of ``scripts/long_stream_bench.py`` (a causal layer with bias, K = max_len, head 64):

  a_push        ``FFTLongConvStream.push`` of the T tokens;
  b_push_nobulk the same call under FFTCONV_LONG_PUSH_BULK=0: windows and the step's own blocks only;
  c_steps       T calls of ``step`` on the same stream -- ``step`` as it was before ``push`` existed, what a caller does
                without ``push``;
  d_prefill     (T >= 1024 only) ``reset()`` and ``prefill`` of all p + T samples, the only other way to append a chunk.

Every append starts at the mid-row position p = max_len / 2 - T / 2 + 5, which is no multiple of the head (the +5: without
it p is one for every T >= 128), behind a prefill of p samples that is not timed.  An append's time is the span between
two HIP events recorded around it (for c_steps around all T steps), host launch cost included.  The variants of a (shape,
T) run in turn in ``--rounds`` (3) alternating rounds of ``--reps`` appends each, after one untimed append per variant
(plans and bulk levels exist by then); reported per variant are the median over all appends, the round medians and three
times their spread.  One JSON line per (shape, T, variant) is appended to --out, then one line of ratios per (shape, T):
a/c and a/b with the verdict of each (a is "ahead" only if the medians differ by more than three times the larger spread).

    python scripts/long_push_bench.py [--rounds 3] [--reps 5] [--out profiles/long_push.jsonl] [--only SUBSTRING] [--max-t N]"""
import argparse
import json
import os
import statistics
import sys

import torch

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
HEAD = 64
TOKENS = (4, 16, 64, 1024, 16384)
# (name, batch, cin, cout, groups, K = max_len, dtype): the shapes of scripts/long_stream_bench.py
SHAPES = [
    ("depthwise B4 C256 K65536 f32", 4, 256, 256, 256, 65536, F32),
    ("depthwise B4 C256 K65536 bf16", 4, 256, 256, 256, 65536, BF16),
    ("depthwise B8 C768 K8192 bf16", 8, 768, 768, 768, 8192, BF16),
    ("dense B4 8->8 K32768 f32", 4, 8, 8, 1, 32768, F32),
]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def run_point(fca, base, emit, stream, x, p, T, rounds, reps):
    chunk = x[:, :, p:p + T].contiguous()
    cols = [x[:, :, j].contiguous() for j in range(p, p + T)]
    whole = x[:, :, :p + T].contiguous()

    def rewind():                                   # untimed: the stream stands at p again, behind a prefill of p samples
        stream.reset()
        stream.prefill(x[:, :, :p])

    def push(bulk):
        os.environ["FFTCONV_LONG_PUSH_BULK"] = "1" if bulk else "0"
        stream.push(chunk)

    def steps():
        for col in cols:
            stream.step(col)

    def prefill():
        stream.reset()
        stream.prefill(whole)

    variants = {"a_push": lambda: push(True), "b_push_nobulk": lambda: push(False), "c_steps": steps}
    if T >= 1024:
        variants["d_prefill"] = prefill
    per_round = {name: [] for name in variants}
    for r in range(rounds + 1):                     # round 0 warms up and is dropped
        for name, fn in variants.items():
            vals = []
            for _ in range(reps if r else 1):
                rewind()
                vals.append(timed(fn))
            if r:
                per_round[name].append(vals)
    os.environ.pop("FFTCONV_LONG_PUSH_BULK", None)
    rows = {}
    for name, rounds_ in per_round.items():
        medians = [statistics.median(v) for v in rounds_]
        rows[name] = dict(base, variant=name, T=T, position=p, us_median=round(statistics.median([v for r_ in rounds_ for v in r_]), 1),
                          round_medians_us=[round(m, 1) for m in medians], spread3_us=round(3 * (max(medians) - min(medians)), 1),
                          n=sum(len(v) for v in rounds_))
        emit(rows[name])
    ops = fca.functional._long_push_plan(p, T, stream.head, stream.taps, p)
    a = rows["a_push"]
    ratios = dict(base, variant="ratios", T=T, position=p, ops={k: sum(op[0] == k for op in ops) for k in ("window", "block", "bulk")},
                  bulk_spectrum_bytes=stream.bulk_spectrum_bytes)
    for key, other in (("a_over_c", "c_steps"), ("a_over_b", "b_push_nobulk"), ("a_over_d", "d_prefill")):
        if other in rows:
            o = rows[other]
            gap, noise = o["us_median"] - a["us_median"], max(a["spread3_us"], o["spread3_us"])
            ratios[key] = round(a["us_median"] / o["us_median"], 4)
            ratios[key + "_verdict"] = "a ahead" if gap > noise else "a behind" if -gap > noise else "inside the spread"
    emit(ratios)


def run_shape(fca, name, B, ci, co, g, K, dtype, rounds, reps, out, max_t):
    torch.manual_seed(0)
    L = K
    x = torch.randn(B, ci, L, device=DEV).to(dtype)
    w = (torch.randn(co, ci // g, K, device=DEV) / (ci // g * K) ** 0.5).to(dtype)
    b = torch.randn(co, device=DEV).to(dtype)
    base = {"shape": name, "dtype": str(dtype).replace("torch.", ""), "B": B, "cin": ci, "cout": co, "groups": g, "K": K,
            "max_len": L, "head": HEAD, "rounds": rounds, "reps": reps, "device": torch.cuda.get_device_name(0)}

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        with open(out, "a") as f:
            f.write(line + "\n")

    stream = fca.FFTLongConvStream(w, b, g, batch=B, max_len=L, head=HEAD)
    for T in TOKENS:
        if T > max_t or T > L // 2:                  # capped at what fits around the middle of the row
            emit(dict(base, variant="not measured", T=T, reason="T past --max-t or past max_len / 2"))
            continue
        p = L // 2 - T // 2 + 5
        assert p % HEAD and p >= 1 and p + T <= L
        run_point(fca, base, emit, stream, x, p, T, rounds, reps)
    del stream
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "long_push.jsonl"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--max-t", type=int, default=max(TOKENS))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import fft_conv_pytorch_amd as fca
    assert torch.cuda.is_available(), "long_push_bench.py measures on a GPU; there is no CPU path"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for shape in SHAPES:
        if a.only and a.only not in shape[0]:
            continue
        run_shape(fca, *shape, a.rounds, a.reps, a.out, a.max_t)
        fca._native.clear_plan_cache()
        torch.cuda.empty_cache()
