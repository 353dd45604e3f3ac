#!/usr/bin/env python3
"""One round of speculative decoding on a stream of a causal long filter ("Verifying draft tokens"):
T draft tokens are verified and a = T / 2 of them accepted.  Microseconds per round, four ways, on the four shapes of
``scripts/long_stream_bench.py`` (a causal layer with bias, K = max_len, head 64):

  a_spec_accept   ``speculate`` of the T drafts, then ``accept(a)``: what the round costs with the two methods;
  b_push_T        ``push`` of all T drafts on the same tree: the verification alone, with no way back;
  c_push_a        ``push`` of the a accepted tokens on the same tree: the committed work alone;
  d_clone_push    the only workaround without the two methods: ``acc.clone()``, ``push`` of the T drafts, ``acc.copy_()`` of
                  the clone, and the position set back to p + a -- which REACHES INTO A PRIVATE ATTRIBUTE (``_position``)
                  and leaves ``acc`` without the blocks of the accepted tokens, so it is a lower bound on a correct
                  workaround, not one.

Positions, with M the multiple of the head the draft passes: (i) "no multiple" p = max_len / 2 + 192, on the grid, so that
no multiple of the head lies inside a draft of up to 64; (ii) "head only" M = max_len / 2 + 192, which 64 divides and 128
does not: one level is due; (iii) "all levels" M = max_len / 2: every level is due and the kernel's late sum is at its
longest.  In (ii) and (iii) p = M - max(1, T / 4), so the accepted tokens pass M and ``accept`` runs the blocks.

The stream is brought to p once per point by a prefill of 64 samples and one push of the rest (so that ``first`` = 64 and
the blocks at M are whole), untimed; before every timed round the bench puts the state back, untimed, by copying a saved
``acc`` and setting the position (the history below p never changes).  A round's time is the span between two HIP events
recorded around it, host cost included.  The variants of a point run in turn in ``--rounds`` (3) alternating rounds of
``--reps`` samples each, after one untimed sample per variant; reported per variant are the median over all samples, the
round medians and three times their spread.  One JSON line per (shape, position, T, variant) is appended to --out, then
one line of ratios per point: a/b, a/c, a/d with the verdict of each (a is "ahead" only if the medians differ by more than
three times the larger spread).

    python scripts/long_spec_bench.py [--rounds 3] [--reps 5] [--out profiles/long_spec.jsonl] [--only SUBSTRING]"""
import argparse
import json
import os
import statistics
import sys

import torch

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
HEAD = 64
TOKENS = (4, 16, 64)
# (name, batch, cin, cout, groups, K = max_len, dtype): the shapes of scripts/long_stream_bench.py
SHAPES = [
    ("depthwise B4 C256 K65536 f32", 4, 256, 256, 256, 65536, F32),
    ("depthwise B4 C256 K65536 bf16", 4, 256, 256, 256, 65536, BF16),
    ("depthwise B8 C768 K8192 bf16", 8, 768, 768, 768, 8192, BF16),
    ("dense B4 8->8 K32768 f32", 4, 8, 8, 1, 32768, F32),
]


def positions(L, T):
    back = max(1, T // 4)
    return (("no multiple", L // 2 + 192), ("head only", L // 2 + 192 - back), ("all levels", L // 2 - back))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def run_point(fca, base, emit, stream, x, where, p, T, rounds, reps):
    a = T // 2
    stream.reset()
    stream.prefill(x[:, :, :HEAD])
    stream.push(x[:, :, HEAD:p])
    acc0 = stream.acc.clone()
    drafts, accepted = x[:, :, p:p + T].contiguous(), x[:, :, p:p + a].contiguous()

    def rewind():                                   # untimed: the state at p again (hist below p has not changed)
        stream.acc.copy_(acc0)
        stream._position, stream._draft = p, None

    def spec_accept():
        stream.speculate(drafts)
        stream.accept(a)

    def clone_push():
        saved = stream.acc.clone()
        stream.push(drafts)
        stream.acc.copy_(saved)
        stream._position = p + a                    # a private attribute: the public interface has no way back

    variants = {"a_spec_accept": spec_accept, "b_push_T": lambda: stream.push(drafts), "c_push_a": lambda: stream.push(accepted),
                "d_clone_push": clone_push}
    per_round = {name: [] for name in variants}
    for r in range(rounds + 1):                     # round 0 warms up and is dropped
        for name, fn in variants.items():
            vals = []
            for _ in range(reps if r else 1):
                rewind()
                vals.append(timed(fn))
            if r:
                per_round[name].append(vals)
    M, blocks = fca.functional._long_spec_plan(p, T, stream.head, stream.taps, HEAD, stream.max_len)
    rows = {}
    for name, rounds_ in per_round.items():
        medians = [statistics.median(v) for v in rounds_]
        rows[name] = dict(base, variant=name, where=where, T=T, accepted=a, position=p,
                          us_median=round(statistics.median([v for r_ in rounds_ for v in r_]), 1),
                          round_medians_us=[round(m, 1) for m in medians], spread3_us=round(3 * (max(medians) - min(medians)), 1),
                          n=sum(len(v) for v in rounds_))
        emit(rows[name])
    mine = rows["a_spec_accept"]
    ratios = dict(base, variant="ratios", where=where, T=T, accepted=a, position=p, M=M, levels_due=len(blocks),
                  late_columns=0 if M is None else p + T - M, acc_bytes=stream.acc.numel() * 4)
    for key, other in (("a_over_b", "b_push_T"), ("a_over_c", "c_push_a"), ("a_over_d", "d_clone_push")):
        o = rows[other]
        gap, noise = o["us_median"] - mine["us_median"], max(mine["spread3_us"], o["spread3_us"])
        ratios[key] = round(mine["us_median"] / o["us_median"], 4)
        ratios[key + "_verdict"] = "a ahead" if gap > noise else "a behind" if -gap > noise else "inside the spread"
    emit(ratios)


def run_shape(fca, name, B, ci, co, g, K, dtype, rounds, reps, out):
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
        for where, p in positions(L, T):
            run_point(fca, base, emit, stream, x, where, p, T, rounds, reps)
    del stream
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "long_spec.jsonl"))
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import fft_conv_pytorch_amd as fca
    assert torch.cuda.is_available(), "long_spec_bench.py measures on a GPU; there is no CPU path"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for shape in SHAPES:
        if a.only and a.only not in shape[0]:
            continue
        run_shape(fca, *shape, a.rounds, a.reps, a.out)
        fca._native.clear_plan_cache()
        torch.cuda.empty_cache()
