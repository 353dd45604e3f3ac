#!/usr/bin/env python3
"""Token-by-token decoding of a causal long filter ("Decoding one token at a time"): microseconds per token,
three ways, on a causal layer with bias whose filter is as long as the row (K = max_len):

  a_stream    ``FFTLongConvStream.step`` for head in 16, 32, 64, 128, 256: a prefill of max_len / 2 - 2048 samples, then a
              decode of ``--tokens`` (4096) tokens, so that the window crosses position max_len / 2, where every block level
              up to max_len / 2 falls due at once (the worst single step of a row) and each larger level is met once.
  b_rerun     ``fft_long_conv(x[..., :t + 1], k, b, causal=True)[..., -1]`` for the prefix, what a caller can do without a
              stream -- the code of that function is the parent commit's, unchanged here -- at three positions of the window:
              the first call at a length (it creates the plan of that length) and the median of five repeats.
  c_einsum    a torch ``einsum`` of the last K history samples against the taps, the O(K) direct line, at 64 positions
              spread over the window (the history window is a view; what ``einsum`` launches for it is torch's choice: for
              the depthwise contraction "bck,ck->bc" it is a batched matrix product that hipBLASLt refuses, and the
              fallback is slow).
  c_mulsum    the same line written ``(window * taps).sum(-1)``, depthwise shapes only: what a caller would write when the
              einsum is that slow; it forms the product tensor.

A token's time is the span between two HIP events recorded on the stream around its ``step`` (blocks included), after the
whole decode has been enqueued and synchronised once: it is the pace of the decode as a caller sees it, host launch cost
included, not a kernel time.  The variants of a shape run in turn in ``--rounds`` (3) alternating rounds; reported per
variant are the median over all tokens of all rounds, the round medians and their spread, the mean (the amortised cost:
block steps included), the worst single step, and the share of steps that were one launch.  One JSON line per (shape,
variant) is appended to --out.

    python scripts/long_stream_bench.py [--tokens 4096] [--rounds 3] [--out profiles/long_stream.jsonl] [--only SUBSTRING]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
HEADS = (16, 32, 64, 128, 256)
# (name, batch, cin, cout, groups, K = max_len, dtype)
SHAPES = [
    ("depthwise B4 C256 K65536 f32", 4, 256, 256, 256, 65536, F32),
    ("depthwise B4 C256 K65536 bf16", 4, 256, 256, 256, 65536, BF16),
    ("depthwise B8 C768 K8192 bf16", 8, 768, 768, 768, 8192, BF16),
    ("dense B4 8->8 K32768 f32", 4, 8, 8, 1, 32768, F32),
]


def spans(events):
    return [a.elapsed_time(b) * 1e3 for a, b in zip(events[:-1], events[1:])]


def decode(stream, x, start, tokens):
    """Per-token spans (us) and the wall time per token of ``tokens`` steps from ``start`` (the prefill is not timed)."""
    stream.reset()
    stream.prefill(x[:, :, :start])
    cols = [x[:, :, j].contiguous() for j in range(start, start + tokens)]
    events = [torch.cuda.Event(enable_timing=True) for _ in range(tokens + 1)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    events[0].record()
    for j in range(tokens):
        stream.step(cols[j])
        events[j + 1].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e6 / tokens
    return spans(events), wall


def summarise(row, per_round):
    """``per_round``: one list of per-token spans per round."""
    everything = [v for vals in per_round for v in vals]
    medians = [round(statistics.median(vals), 2) for vals in per_round]
    row["us_per_token_median"] = round(statistics.median(everything), 2)
    row["round_medians_us"] = medians
    row["spread_us"] = round(max(medians) - min(medians), 2)
    row["us_per_token_mean"] = round(statistics.fmean(everything), 2)
    row["worst_step_us"] = round(max(everything), 1)
    row["n"] = len(everything)
    return row


def einsum_line(hist, w, groups, t):
    """y_t of the direct line: the last min(K, t + 1) samples against the taps (depthwise or one group)."""
    K = w.shape[2]
    m = min(K, t + 1)
    window, taps = hist[:, :, t + 1 - m:t + 1], w[:, :, K - m:]        # (w is stored flipped: its last m are taps m-1 ... 0)
    if groups == 1:
        return torch.einsum("bik,oik->bo", window, taps)
    return torch.einsum("bck,ck->bc", window, taps[:, 0])


def mulsum_line(hist, w, groups, t):
    K = w.shape[2]
    m = min(K, t + 1)
    return (hist[:, :, t + 1 - m:t + 1] * w[:, 0, K - m:]).sum(-1)


def run_shape(fca, name, B, ci, co, g, K, dtype, tokens, rounds, out, variants="abc"):
    torch.manual_seed(0)
    L = K
    start = L // 2 - tokens // 2
    assert start >= 1 and start + tokens <= L
    x = torch.randn(B, ci, L, device=DEV).to(dtype)
    w = (torch.randn(co, ci // g, K, device=DEV) / (ci // g * K) ** 0.5).to(dtype)
    b = torch.randn(co, device=DEV).to(dtype)
    base = {"shape": name, "dtype": str(dtype).replace("torch.", ""), "B": B, "cin": ci, "cout": co, "groups": g, "K": K,
            "max_len": L, "prefill": start, "tokens": tokens, "rounds": rounds, "device": torch.cuda.get_device_name(0)}

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        with open(out, "a") as f:
            f.write(line + "\n")

    if "a" in variants:
        run_streams(fca, base, emit, x, w, b, g, K, L, start, tokens, rounds, dtype)
    if "c" in variants:
        run_direct(base, emit, x, w, g, start, tokens, rounds)
    if "b" in variants:
        run_rerun(fca, base, emit, x, w, b, g, start, tokens)


def run_streams(fca, base, emit, x, w, b, g, K, L, start, tokens, rounds, dtype):
    """a: the stream, every head; the variants alternate inside a round."""
    B, name = base["B"], base["shape"]
    streams = {h: fca.FFTLongConvStream(w, b, g, batch=B, max_len=L, head=h) for h in HEADS}
    for s in streams.values():                      # warm-up: every level's launch has run once
        decode(s, x, start, tokens)
    per_round = {h: [] for h in HEADS}
    walls = {h: [] for h in HEADS}
    for _ in range(rounds):
        for h, s in streams.items():
            vals, wall = decode(s, x, start, tokens)
            per_round[h].append(vals)
            walls[h].append(round(wall, 2))
    last = {}
    for h, s in streams.items():
        blocks = sum(1 for i in range(start + 1, start + tokens + 1) if fca.functional._long_stream_blocks(i, h, K, start))
        row = dict(base, variant="a_stream", head=h, state_bytes=s.state_bytes, levels=len(s._levels),
                   one_launch_share=round(1.0 - blocks / tokens, 4), wall_us_per_token_rounds=walls[h])
        emit(summarise(row, per_round[h]))
        last[h] = s.step(x[:, :, start + tokens].contiguous()).float() if start + tokens < L else None
    # (the heads agree with each other on the next token: different schedules of the same sum)
    ref = last[64]
    if ref is not None:
        for h, y in last.items():
            assert float((y - ref).abs().max() / ref.abs().max()) < (2e-2 if dtype == BF16 else 1e-4), (name, h)
    del streams
    torch.cuda.empty_cache()


def run_direct(base, emit, x, w, g, start, tokens, rounds):
    """c: the O(K) line over the history (the row itself in float32 stands for it), the two spellings in turn."""
    hist, wf = x.float(), w.float().flip(-1).contiguous()
    positions = [start + (tokens * i) // 64 for i in range(64)]
    lines = {"c_einsum": einsum_line}
    if g > 1:
        lines["c_mulsum"] = mulsum_line
    for line in lines.values():
        for t in positions[:4]:
            line(hist, wf, g, t)
    per_round = {key: [] for key in lines}
    for _ in range(rounds):
        for key, line in lines.items():
            events = [torch.cuda.Event(enable_timing=True) for _ in range(len(positions) + 1)]
            torch.cuda.synchronize()
            events[0].record()
            for j, t in enumerate(positions):
                line(hist, wf, g, t)
                events[j + 1].record()
            torch.cuda.synchronize()
            per_round[key].append(spans(events))
    for key in lines:
        emit(summarise(dict(base, variant=key, note="float32 history and taps; bias and rounding not included"), per_round[key]))
    del hist, wf
    torch.cuda.empty_cache()


def run_rerun(fca, base, emit, x, w, b, g, start, tokens):
    """b: the causal call on the whole prefix, per token."""
    for t in (start, start + tokens // 2 + 1, start + tokens - 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            fca.fft_long_conv(x[:, :, :t + 1], w, b, groups=g, causal=True)[:, :, -1]
        torch.cuda.synchronize()
        first_ms = (time.perf_counter() - t0) * 1e3
        vals = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            with torch.no_grad():
                fca.fft_long_conv(x[:, :, :t + 1], w, b, groups=g, causal=True)[:, :, -1]
            e1.record()
            torch.cuda.synchronize()
            vals.append(e0.elapsed_time(e1) * 1e3)
        emit(dict(base, variant="b_rerun", position=t, first_call_ms=round(first_ms, 2),
                  us_per_token_median=round(statistics.median(vals), 1), repeats_us=[round(v, 1) for v in vals]))
        fca._native.clear_plan_cache()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "long_stream.jsonl"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--variants", default="abc", help="which of a (stream), b (rerun), c (direct lines) to run")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import fft_conv_pytorch_amd as fca
    assert torch.cuda.is_available(), "long_stream_bench.py measures on a GPU; there is no CPU path"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for shape in SHAPES:
        if a.only and a.only not in shape[0]:
            continue
        run_shape(fca, *shape, a.tokens, a.rounds, a.out, a.variants)
        fca._native.clear_plan_cache()
        torch.cuda.empty_cache()
