#!/usr/bin/env python3
"""Times of float64 ``fft_conv`` with kernels past 1025 taps: the long route (one transform of N1 x N2 points per row,
csrc/long_f64.hip) against the direct kernel and against the reference's torch.fft formulation.

  new      this tree's library, the plan the planner picks, cached kernel spectrum
  a        another build of the library (``--base-lib``, the parent commit's: the direct kernel), same call
  b        torch.fft.rfft / irfft on the padded row in float64, kernel spectrum precomputed (the reference's algorithm)

The library is chosen when the package is imported (FFTCONV_LIB), so each build is timed in a child process of its own;
the children of ``new`` and ``a`` alternate over ``--rounds`` rounds.  In a child every step is captured into a HIP graph
after a warm-up and replayed between HIP events; the median of ``--iters`` replays is one round's figure (3 replays for a
step slower than ``--cap-ms``).  A shape's figure is the median of its rounds; ``spread`` is (max - min) / median over the
rounds.  One JSON line per shape is appended to ``--out``.

``--sweep`` times both routes of this tree's library (FFTCONV_F64_LONG=0 / 2) at shapes on both sides of the planner's
crossover and reports, per shape, the ratio  nout * Cin/g * K / (ntiles * N * log2 N)  its rule compares with a constant.

    python scripts/f64_long_bench.py --base-lib /path/to/parent/libfftconv_amd.so [--only SUBSTRING]
    python scripts/f64_long_bench.py --sweep"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
# (name, batch, cin, cout, groups, L, K): padding K // 2 on both sides
SHAPES = [
    ("depthwise B4 C64 K=L=16384", 4, 64, 64, 64, 16384, 16384),
    ("depthwise B4 C64 K=L=65536", 4, 64, 64, 64, 65536, 65536),
    ("dense B4 8->8 K=L=32768", 4, 8, 8, 1, 32768, 32768),
    ("depthwise B8 C64 L65536 K2048", 8, 64, 64, 64, 65536, 2048),
    ("depthwise B8 C64 L65536 K4096", 8, 64, 64, 64, 65536, 4096),
]
# (batch, cin, cout, groups, L, K, padding): both sides of the crossover -- few kept outputs ('valid' calls with K near L),
# few taps, one and several input channels per group
SWEEP = [(4, 16, 16, 16, 8192, K, 0) for K in (8192 - 15, 8192 - 63, 8192 - 255, 8192 - 1023)]
SWEEP += [(4, 16, 16, 16, 32768, K, 0) for K in (32768 - 63, 32768 - 255, 32768 - 1023, 32768 - 4095)]
SWEEP += [(4, 16, 16, 16, L, 1100, 0) for L in (1200, 1600, 2400, 4000)]
SWEEP += [(4, 8, 8, 1, 8192, K, 0) for K in (8192 - 3, 8192 - 15, 8192 - 63, 8192 - 255)]
SWEEP += [(2, 16, 16, 16, 262144, K, 0) for K in (262144 - 255, 262144 - 1023, 262144 - 4095)]


def child_main(a):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from fft_conv_pytorch_amd import _native
    from fft_conv_pytorch_amd import functional as fc

    def capture(step):
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side), torch.no_grad():
            step()                                   # warm: the plan exists before the capture
        torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(g):
            step()
        return g

    def timed(g):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def measure(graphs):
        samples = {k: [timed(g)] for k, g in graphs.items()}
        reps = {k: (a.iters if samples[k][0] <= a.cap_ms * 1e3 else 3) for k in graphs}
        for i in range(1, a.iters):
            for k, g in graphs.items():              # in turn
                if i < reps[k]:
                    samples[k].append(timed(g))
        return {k: (round(statistics.median(v), 1), len(v)) for k, v in samples.items()}

    def conv_step(x, w, p, g):
        plan = fc._plan_for(x, w, None, 1, p, 1, g, "constant")
        spec = fc.transform_kernel(plan, w)
        return plan, (lambda: fc._fft_conv_impl(x, w, None, 1, p, 1, g, "constant", spec, plan))

    def rule_ratio(r, nout, cig, K):
        N = r["N1"] * r["N2"]
        return nout * cig * K / (r["ntiles"] * N * math.log2(N))

    out = []
    if a.sweep:
        for (B, ci, co, g, L, K, p) in SWEEP:
            torch.manual_seed(0)
            x = torch.randn(B, ci, L, device=DEV, dtype=torch.float64)
            w = torch.randn(co, ci // g, K, device=DEV, dtype=torch.float64) / K ** 0.5
            graphs, plans = {}, {}
            for knob, name in (("0", "direct"), ("2", "long")):
                os.environ["FFTCONV_F64_LONG"] = knob     # (read at plan creation)
                _native.clear_plan_cache()
                plans[name], step = conv_step(x, w, p, g)
                graphs[name] = capture(step)
            del os.environ["FFTCONV_F64_LONG"]
            _native.clear_plan_cache()
            picked = fc._plan_for(x, w, None, 1, p, 1, g, "constant").route["kind"]
            with torch.no_grad():
                ya, yb = (fc._forward_native(x, fc.transform_kernel(plans[n], w), None) for n in ("direct", "long"))
            res = measure(graphs)
            r = plans["long"].route
            nout = L + 2 * p - K + 1
            row = {"sweep": True, "B": B, "cin": ci, "cout": co, "groups": g, "L": L, "K": K, "padding": p, "nout": nout,
                   "route": r, "rule_ratio": round(rule_ratio(r, nout, ci // g, K), 3), "planner_picks": picked,
                   "direct_us": res["direct"][0], "long_us": res["long"][0],
                   "long_over_direct": round(res["long"][0] / res["direct"][0], 3),
                   "max_rel": float((ya - yb).abs().max() / ya.abs().max()), "device": torch.cuda.get_device_name(0)}
            out.append(row)
            print(json.dumps(row), flush=True)
            del graphs, x, w, ya, yb
            torch.cuda.empty_cache()
        return
    for (name, B, ci, co, g, L, K) in SHAPES:
        if a.only and a.only not in name:
            continue
        torch.manual_seed(0)
        p = K // 2
        x = torch.randn(B, ci, L, device=DEV, dtype=torch.float64)
        w = torch.randn(co, ci // g, K, device=DEV, dtype=torch.float64) / K ** 0.5
        plan, step = conv_step(x, w, p, g)
        graphs = {"conv": capture(step)}
        if a.with_torch_fft:
            n = L + 2 * p
            n += n % 2
            wf = torch.fft.rfft(w, n).conj()

            def step_b():
                xf = torch.fft.rfft(F.pad(x, (p, p)), n)
                yf = torch.einsum("bgif,goif->bgof", xf.view(B, g, ci // g, -1), wf.view(g, co // g, ci // g, -1))
                return torch.fft.irfft(yf.reshape(B, co, -1), n)[..., :L + 2 * p - K + 1]
            try:
                graphs["torch_fft"] = capture(step_b)
            except Exception as exc:                 # (recorded, not hidden: the figure is then missing from the line)
                print(json.dumps({"shape": name, "torch_fft_note": f"not captured: {str(exc)[:160]}"}), flush=True)
                torch.cuda.synchronize()
        res = measure(graphs)
        row = {"shape": name, "route": plan.route, "conv_us": res["conv"][0], "conv_n": res["conv"][1],
               "device": torch.cuda.get_device_name(0)}
        if "torch_fft" in res:
            with torch.no_grad():
                row["vs_torch_fft_max_rel"] = float((step() - step_b()).abs().max() / step_b().abs().max())
            row["torch_fft_us"], row["torch_fft_n"] = res["torch_fft"]
        print(json.dumps(row), flush=True)
        del graphs, x, w
        torch.cuda.empty_cache()


def run_child(a, lib, extra):
    env = dict(os.environ)
    env.pop("FFTCONV_LIB", None)
    if lib:
        env["FFTCONV_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters), "--cap-ms", str(a.cap_ms)] + extra
    if a.only:
        cmd += ["--only", a.only]
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=a.child_timeout)
    if proc.returncode != 0:
        raise SystemExit(f"child failed with status {proc.returncode} (library: {lib or 'this tree'})")
    return [json.loads(line) for line in proc.stdout.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cap-ms", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f64_long.jsonl"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--base-lib", default=None, help="libfftconv_amd.so of the parent commit (yardstick a)")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--with-torch-fft", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-timeout", type=float, default=900.0)
    a = ap.parse_args()
    if a.child:
        return child_main(a)
    if a.sweep:
        rows = run_child(a, None, ["--sweep"])
        with open(a.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")
        for row in rows:
            print(json.dumps(row))
        return
    if not a.base_lib or not os.path.exists(a.base_lib):
        raise SystemExit("--base-lib: the parent commit's libfftconv_amd.so is needed for yardstick (a)")
    rounds = {"new": [], "a": []}
    for _ in range(a.rounds):                        # alternating: new, a, new, a, ...
        rounds["new"].append(run_child(a, None, ["--with-torch-fft"]))
        rounds["a"].append(run_child(a, os.path.abspath(a.base_lib), []))
    names = [r["shape"] for r in rounds["new"][0] if "conv_us" in r]
    with open(a.out, "a") as f:
        for name in names:
            def pick(which, key):
                return [r[key] for rnd in rounds[which] for r in rnd if r.get("shape") == name and key in r]
            first = {w: next(r for r in rounds[w][0] if r.get("shape") == name and "conv_us" in r) for w in rounds}
            new, base, tf = pick("new", "conv_us"), pick("a", "conv_us"), pick("new", "torch_fft_us")
            med = statistics.median
            row = {"shape": name, "device": first["new"]["device"], "iters": a.iters, "rounds": a.rounds,
                   "route": first["new"]["route"], "a_route": first["a"]["route"],
                   "new_us": med(new), "new_rounds_us": new, "a_us": med(base), "a_rounds_us": base,
                   "a_spread": round((max(base) - min(base)) / med(base), 4),
                   "new_over_a": round(med(new) / med(base), 4),
                   "b_us": med(tf) if tf else None, "b_rounds_us": tf,
                   "new_over_b": round(med(new) / med(tf), 4) if tf else None,
                   "vs_torch_fft_max_rel": first["new"].get("vs_torch_fft_max_rel")}
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
