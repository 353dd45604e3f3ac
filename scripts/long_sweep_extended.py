#!/usr/bin/env python3
"""The cross-feature sweep of the long-filter family (tests/long_sweep_util.py) for any seed: the tables of that seed, every
case printed before it runs and held to the checks of tests/test_gpu_long_sweep.py (routes, values against the exact truth
within the bound of the float32 baseline, layouts, the promised bit relations, untouched inputs).  One JSON line per case --
id, predicted and observed launches, N1 x N2, slabs, e_rms and e_max of y, dX, dW and db with their ratios to the
baseline's -- goes to --out (default: standard output).  Exits non-zero on the first mismatch (--keep-going: after the last case, having listed them all).

    python scripts/long_sweep_extended.py [SEED] [--out profiles/long_sweep.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import long_sweep_util as su  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("seed", nargs="?", type=int, default=su.SEED)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--keep-going", action="store_true", help="list every mismatch instead of stopping at the first")
    args = ap.parse_args()
    fwd, tr = su.tables(args.seed)
    print(f"long sweep, seed {args.seed}: {len(fwd)} forward and {len(tr)} transposed cases", flush=True)
    out = open(args.out, "w") if args.out else None
    worst, failed = {}, []
    for c in fwd + tr:
        try:
            rec = su.run_case(c, args.device, su.os_setenv, log=lambda s: print(s, flush=True))
        except AssertionError as exc:
            print(f"MISMATCH in {c.id}: {exc}", flush=True)
            if not args.keep_going:
                sys.exit(1)
            failed.append(c.id)
            continue
        line = json.dumps(rec)
        if out:
            out.write(line + "\n")
            out.flush()
        else:
            print(line, flush=True)
        for name in ("y", "dX", "dW", "db"):
            if name in rec:
                for k in ("rms_ratio", "max_ratio"):
                    if rec[name][k] > worst.get((name, k), (0.0, ""))[0]:
                        worst[name, k] = (rec[name][k], c.id)
    for (name, k), (v, cid) in sorted(worst.items()):
        print(f"worst {name} {k}: {v:.3f} ({cid})")
    if failed:
        print(f"long sweep, seed {args.seed}: {len(failed)} cases MISMATCH: {failed}")
        sys.exit(1)
    print(f"long sweep, seed {args.seed}: all cases within the bound")


if __name__ == "__main__":
    main()
